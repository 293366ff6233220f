"""The batched commit phase (stark_mlwe_amd/csrc/fri_batch.hpp) on the CPU: the layer loops of fri_build_transcript over B traces side by side,
run through the host instantiation of the stream bodies the device runs (leaf_pair_body over the concatenated layers, hash_ds_body over
DsBatchStream and the new DsBatchPairStream).  Every root must equal the oracle's for that trace alone.  The pair-leaf stream is also checked
on its own against hc_hash_ds_level mode 1 tree by tree.  The first [128] case derives the t = 129 kernel constants on the host once per process
(about 100 s; the host-check library caches them for the later cases).  The GPU build of the same driver is tested in tests/test_gpu_prove_batch_tail.py."""
import ctypes as C
import random

import numpy as np
import pytest

vp = C.c_void_p

# (k, schedule, r): the smallest shapes at which each part of the commit phase can go wrong
SHAPES = [
    (6, [4, 2], 4),       # unhashed arities 4 and 2 with cp_div 4 and 2: pair leaves only
    (10, [16, 8], 8),     # hashed 16 (t = 17) and 8 (t = 9); ragged upper levels 1024 -> 64 -> 4 -> 1
    (7, [128], 4),        # width 129, a one-node tree
    (8, [], 4),           # L = 0: one layer, arity 2, zero partners
]


def ptr(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def tparams(hostcheck):
    h = hostcheck.params(1)
    yield h
    hostcheck.params_free(h)


def commit_batch_rc(hostcheck, tparams, f0s, n0, sched, seed_z):
    """-> (the export's status, (B, L + 1, 4) roots)"""
    B, L = len(f0s), len(sched)
    fs = [np.ascontiguousarray(f, dtype=np.uint64) for f in f0s]
    tab = (vp * B)(*[ptr(f) for f in fs])
    sch = np.ascontiguousarray(sched, dtype=np.uint64)
    roots = np.zeros((B, L + 1, 4), np.uint64)
    rc = hostcheck.l.hc_fri_commit_batch(tparams, C.c_size_t(B), tab, C.c_size_t(n0), ptr(sch), C.c_size_t(L), C.c_uint64(seed_z), ptr(roots))
    return rc, roots


def commit_batch(hostcheck, tparams, f0s, n0, sched, seed_z):
    rc, roots = commit_batch_rc(hostcheck, tparams, f0s, n0, sched, seed_z)
    assert rc == 0, rc
    return roots


@pytest.fixture(scope="module")
def references(oracle):
    """shape index -> (five f0 traces, their oracle roots): computed once, shared by the B = 1, 3, 5 cases"""
    out = {}
    for i, (k, sched, r) in enumerate(SHAPES):
        n0 = 1 << k
        f0s = oracle.rand_fr_columns(0xF0 + i, n0, 5)
        want = np.zeros((5, len(sched) + 1, 4), np.uint64)
        for b in range(5):
            pr = oracle.deep_fri_prove(None, None, None, None, n0, sched, r, 0xDEEFBAAD + i, f0=f0s[b])
            for l in range(len(sched) + 1):
                want[b, l] = pr.root(l)
            pr.free()
        out[i] = (f0s, want)
    return out


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_commit_batch_roots_equal_oracle(hostcheck, tparams, references, shape, B):
    k, sched, _ = SHAPES[shape]
    f0s, want = references[shape]
    got = commit_batch(hostcheck, tparams, f0s[:B], 1 << k, sched, 0xDEEFBAAD + shape)
    for b in range(B):
        assert (got[b] == want[b]).all(), (b, got[b], want[b])
    if B > 1:
        assert len({got[b].tobytes() for b in range(B)}) == B


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("arity,n,cp_div", [(4, 64, 4), (2, 16, 2), (2, 8, 1), (4, 12, 3), (2, 1, 1)])
def test_batch_pairs_level_equals_tree_by_tree(hostcheck, oracle, arity, n, cp_div, B):
    params = hostcheck.params(0, 9)
    try:
        rng = random.Random(B * 1000 + n)
        labels = np.array([rng.choice([0, 1, 2, 1 << 40]) for _ in range(B)], dtype=np.uint64)
        f = np.ascontiguousarray(oracle.rand_fr_columns(B + n, n, B).reshape(B * n, 4))
        ncp = n // cp_div
        cp = np.ascontiguousarray(oracle.rand_fr_columns(7 * B + n, ncp, B).reshape(B * ncp, 4))
        for with_cp in (True, False):
            out = np.zeros((B * n, 4), np.uint64)
            assert hostcheck.l.hc_hash_ds_batch_pairs_level(params, C.c_size_t(arity), ptr(labels), ptr(f), ptr(cp) if with_cp else None, C.c_size_t(n), C.c_size_t(cp_div),
                                                            C.c_size_t(B), ptr(out)) == 0
            for b in range(B):
                fb = f[b * n:(b + 1) * n]
                in1 = np.repeat(cp[b * ncp:(b + 1) * ncp], cp_div, axis=0) if with_cp else None      # the view s[i] = cp[i / cp_div]
                want = hostcheck.hash_ds_level(params, 1, arity, 0xFFFFFFFF, 0, int(labels[b]), fb, in1)
                assert (out[b * n:(b + 1) * n] == want).all(), (with_cp, b)
    finally:
        hostcheck.params_free(params)
