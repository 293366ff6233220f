"""Mixed-size batches on the CPU: the ragged DS stream (csrc/poseidon_streams.hpp DsRaggedStream) and the driver of stark_merkle_build_mixed_batch_dev
(csrc/merkle_batch.hpp merkle_build_mixed_batch), instantiated over the host bodies of the DS streams (hostcheck.cpp hc_hash_ds_ragged_level,
hc_merkle_build_mixed_batch), against the single-tree stream (hc_hash_ds_level), the same-shape driver (hc_merkle_build_batch) and the oracle's
MerkleTree (oracle/merkle.hpp); and the sum-check provers with a k per witness (csrc/sumcheck_batch.hpp, hc_sumcheck_prove_mixed_batch) against the
oracle's proof of each witness alone and against the same-size export (hc_sumcheck_prove_batch)."""
import ctypes as C

import numpy as np
import pytest

import merkle_batch_cases as mc
import mixed_batch_cases as xc
import test_merkle_batch_host as mb
from test_pool_poison_host import FILLS, alloc_fill

vp = C.c_void_p
P = mb.P
hc_params = mb.hc_params


def ragged_level(hostcheck, params, mode, arity, level, pos0, labels, ins, in1s=None):
    """one launch of the ragged stream -> the hashes of all segments back to back (hc_hash_ds_ragged_level), or None when it is refused"""
    S = len(ins); ins = [np.ascontiguousarray(a, dtype=np.uint64) for a in ins]
    tab = (vp * S)(*[a.ctypes.data for a in ins])
    tab1 = None if in1s is None else (vp * S)(*[None if a is None else a.ctypes.data for a in in1s])
    n_in = np.array([a.shape[0] for a in ins], np.uint64); lab = np.ascontiguousarray(labels, dtype=np.uint64)
    total = sum(a.shape[0] if mode == 1 else (a.shape[0] + arity - 1) // arity for a in ins)
    out = np.zeros((total, 4), np.uint64)
    hostcheck.l.hc_hash_ds_ragged_level.restype = C.c_long
    got = hostcheck.l.hc_hash_ds_ragged_level(params, mode, C.c_size_t(arity), C.c_uint32(level), C.c_uint64(pos0), C.c_size_t(S), P(lab), tab, tab1, P(n_in), P(out))
    if got < 0:
        return None
    assert got == total
    return out


def hc_build_mixed_rc(hostcheck, params, arity, labels, cols, cps=None):
    """-> (the export's return value, [levels of tree b] or None when it is negative) through hc_merkle_build_mixed_batch"""
    B = len(cols); ns = np.array([c.shape[0] for c in cols], np.uint64)
    tab = (vp * B)(*[c.ctypes.data for c in cols])
    ctab = None if cps is None else (vp * B)(*[None if c is None else c.ctypes.data for c in cps])
    cap = 2 * int(ns.sum()) + 64 * B
    out = np.zeros((cap, 4), np.uint64); lab = np.ascontiguousarray(labels, dtype=np.uint64)
    nlev = np.zeros(B, np.uint64); lens = np.zeros(64 * B, np.uint64)
    depth = hostcheck.l.hc_merkle_build_mixed_batch(params, C.c_size_t(arity), C.c_size_t(B), P(lab), tab, P(ns), 0 if cps is None else 1, ctab, P(out), C.c_size_t(cap), P(nlev), P(lens))
    if depth < 0:
        return depth, None
    trees = [[] for _ in range(B)]; at = 0
    for v in range(depth):                                                  # level v: the slices of the trees that have it, in tree order
        for b in range(B):
            if v < int(nlev[b]):
                ln = int(lens[64 * b + v]); trees[b].append(out[at:at + ln].copy()); at += ln
    assert depth == max(int(x) for x in nlev)
    return depth, trees


def hc_build_mixed(hostcheck, params, arity, labels, cols, cps=None):
    """-> [levels of tree b] through hc_merkle_build_mixed_batch, or None when the shapes are refused"""
    return hc_build_mixed_rc(hostcheck, params, arity, labels, cols, cps)[1]


def mixed_inputs(oracle, arity, ns, pairs):
    labels = xc.labels_of(len(ns))
    cols = [xc.leaves_of(oracle, b, n) for b, n in enumerate(ns)]
    cps = xc.cps_of(oracle, ns) if pairs else None
    return labels, cols, cps


@pytest.mark.parametrize("mode", [0, 1])
def test_one_ragged_launch_equals_the_single_tree_stream(oracle, hostcheck, hc_params, mode):
    """one launch over segments of 1, 2, 16, 17 and 37 children (and of one tree alone) gives, segment by segment, the hashes of DsStream on that
    tree: the node level under its own label with a ragged last node, the pair leaves with a real and a NULL second column; a non-zero pos0"""
    arity, level, pos0 = 16, (3 if mode == 0 else 0xFFFFFFFF), 5
    n_in = [1, 2, 16, 17, 37, 16, 1]; labels = xc.labels_of(len(n_in))
    ins = [xc.leaves_of(oracle, b, n) for b, n in enumerate(n_in)]
    in1s = None if mode == 0 else [None if xc.cp_is_null(b) else xc.leaves_of(oracle, b + 100, n) for b, n in enumerate(n_in)]
    h = hc_params(arity)
    want = [hostcheck.hash_ds_level(h, mode, arity, level, pos0, labels[b], ins[b], None if in1s is None else in1s[b]) for b in range(len(n_in))]
    got = ragged_level(hostcheck, h, mode, arity, level, pos0, labels, ins, in1s)
    assert got.shape == np.concatenate(want).shape and (got == np.concatenate(want)).all()
    for b in (0, 3, 4):                                                     # B = 1: the search over a table of one segment
        one = ragged_level(hostcheck, h, mode, arity, level, pos0, labels[b:b + 1], ins[b:b + 1], None if in1s is None else in1s[b:b + 1])
        assert (one == want[b]).all(), b
    assert ragged_level(hostcheck, h, mode, arity, level, pos0, labels[:2], [ins[0], ins[1][:0]]) is None      # an empty segment is refused


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("arity", sorted(xc.SETS))
def test_mixed_build_equals_the_oracle_tree_by_tree(oracle, hostcheck, hc_params, arity, pairs):
    """every level of every tree of one mixed call is the oracle's MerkleTree of that column alone, plain and as pairs (real and NULL cp entries)"""
    ns = xc.SETS[arity]; labels, cols, cps = mixed_inputs(oracle, arity, ns, pairs)
    trees = hc_build_mixed(hostcheck, hc_params(arity), arity, labels, cols, cps)
    for b, n in enumerate(ns):
        want = xc.oracle_tree(oracle, arity, b, n, pairs, labels[b])
        assert len(trees[b]) == want.num_levels(), (b, n)
        for v in range(want.num_levels()):
            assert (trees[b][v] == want.level(v)).all(), (b, n, v)


@pytest.mark.parametrize("arity,n,pairs", [(16, 257, False), (16, 1, False), (4, 64, True), (8, 65, False)])
def test_equal_lengths_equal_the_same_shape_driver(oracle, hostcheck, hc_params, arity, n, pairs):
    """with every n[b] equal the mixed driver gives what hc_merkle_build_batch gives"""
    B = 3; labels, cols, cps = mixed_inputs(oracle, arity, [n] * B, pairs)
    lens, want = mb.hc_build(hostcheck, hc_params(arity), arity, labels, cols, n, cps)
    got = hc_build_mixed(hostcheck, hc_params(arity), arity, labels, cols, cps)
    for b in range(B):
        assert len(got[b]) == len(lens) and all((g == w).all() for g, w in zip(got[b], want[b])), b


@pytest.mark.parametrize("pairs", [False, True])
def test_mixed_build_does_not_read_what_its_blocks_held(oracle, hostcheck, hc_params, pairs):
    """the arity-16 set under hc_set_alloc_fill 0x5A and 0x00: equal bytes, and the oracle's"""
    arity = 16; ns = xc.SETS[arity]; labels, cols, cps = mixed_inputs(oracle, arity, ns, pairs)
    runs = []
    for fill in FILLS:
        with alloc_fill(hostcheck, fill):
            runs.append(hc_build_mixed(hostcheck, hc_params(arity), arity, labels, cols, cps))
    for b, n in enumerate(ns):
        want = xc.oracle_tree(oracle, arity, b, n, pairs, labels[b])
        for v in range(want.num_levels()):
            assert (runs[0][b][v] == runs[1][b][v]).all() and (runs[0][b][v] == want.level(v)).all(), (b, v)


def test_refused_shapes(oracle, hostcheck, hc_params):
    """the driver's shape guards: an empty tree, an arity of another width, arity 1 with more than one leaf in some tree, pairs without a cp table"""
    cols = [xc.leaves_of(oracle, 0, 8), xc.leaves_of(oracle, 1, 1)]
    assert hc_build_mixed(hostcheck, hc_params(16), 8, [1, 2], cols) is None           # arity 8 needs t = 9
    assert hc_build_mixed(hostcheck, hc_params(8), 1, [1, 2], cols) is None            # arity 1, some n > 1
    assert hc_build_mixed(hostcheck, hc_params(8), 8, [1, 2], [cols[0], cols[1][:0]]) is None
    one = hc_build_mixed(hostcheck, hc_params(8), 1, [1, 2], [cols[1], cols[1]])       # arity 1, one leaf each: the roots are the leaves
    assert [len(t) for t in one] == [1, 1] and (one[0][0] == cols[1]).all()


# ---- mixed-size sum-check prove (csrc/sumcheck_batch.hpp ScBatch with a k per instance) --------------------------------------------------------
import test_sumcheck_batch_host as sb

tparams = sb.tparams
cparams = sb.cparams


def prove_mixed(hostcheck, tparams, cparams, mf, ks, labels, witnesses, q=0):
    """-> the proofs of one mixed call in the caller's order (hc_sumcheck_prove_mixed_batch)"""
    B = len(witnesses)
    ws = [np.ascontiguousarray(w, dtype=np.uint64) for w in witnesses]
    wp = (vp * B)(*[w.ctypes.data for w in ws]); kk = (C.c_size_t * B)(*ks)
    lab = np.ascontiguousarray(labels, dtype=np.uint64); lens = (C.c_size_t * B)()
    f = hostcheck.l.hc_sumcheck_prove_mixed_batch
    f.restype = C.c_size_t
    args = (tparams, cparams, mf, C.c_size_t(B), wp, kk, P(lab), C.c_size_t(q))
    tot = f(*args, None, C.c_size_t(0), lens)
    assert tot > 0
    buf = (C.c_uint8 * tot)()
    assert f(*args, buf, C.c_size_t(tot), lens) == tot
    out, o = [], 0
    for b in range(B):
        out.append(bytes(buf[o:o + lens[b]])); o += lens[b]
    return out


@pytest.fixture(scope="module")
def sumcheck_case(oracle):
    """the witnesses of xc.SUMCHECK_K and, per (mf, q), the oracle's proof of each alone (computed once)"""
    ws = xc.witnesses_of(oracle, xc.SUMCHECK_K); memo = {}

    def want(mf, q):
        if (mf, q) not in memo:
            memo[(mf, q)] = [oracle.sumcheck_prove(mf, k, lab, w, q=q) if mf else oracle.sumcheck_prove(0, k, lab, w) for k, lab, w in zip(xc.SUMCHECK_K, xc.SUMCHECK_LABELS, ws)]
        return memo[(mf, q)]
    return ws, want


@pytest.mark.parametrize("mf,q", [(0, 0), (1, 1), (1, 2), (1, 8)])
def test_mixed_sumcheck_equals_the_oracle_witness_by_witness(hostcheck, tparams, cparams, sumcheck_case, mf, q):
    """every proof of one mixed call (k = 0, 1, 5, 3, 5, 0, 2) is the oracle's on that witness alone, plain and mf; with q = 8 the redraws and the
    fill-in rule run for the small instances only; the same witnesses in another order give the same proof each"""
    ws, want = sumcheck_case; ks, labels = xc.SUMCHECK_K, xc.SUMCHECK_LABELS
    got = prove_mixed(hostcheck, tparams, cparams, mf, ks, labels, ws, q)
    for b in range(len(ks)):
        assert got[b] == want(mf, q)[b], (b, ks[b])
    sh = xc.SUMCHECK_SHUFFLE
    got2 = prove_mixed(hostcheck, tparams, cparams, mf, [ks[i] for i in sh], [labels[i] for i in sh], [ws[i] for i in sh], q)
    assert got2 == [got[i] for i in sh]


@pytest.mark.parametrize("mf,k,q", [(0, 0, 0), (0, 3, 0), (1, 0, 2), (1, 3, 2), (1, 3, 8)])
def test_equal_k_equals_the_same_size_driver_entry(hostcheck, tparams, cparams, oracle, mf, k, q):
    """with every k[b] equal the mixed export gives what hc_sumcheck_prove_batch gives"""
    labels = [11, 6060, 11]; ws = oracle.rand_fr_columns(0x77 + k, 1 << k, 3)
    assert prove_mixed(hostcheck, tparams, cparams, mf, [k] * 3, labels, ws, q) == sb.prove_batch(hostcheck, tparams, cparams, mf, k, labels, ws, q)


@pytest.mark.parametrize("mf,q", [(0, 0), (1, 2), (1, 8)])
def test_mixed_sumcheck_does_not_read_what_its_blocks_held(hostcheck, tparams, cparams, sumcheck_case, mf, q):
    """under hc_set_alloc_fill 0x5A and 0x00: equal bytes, and the oracle's"""
    ws, want = sumcheck_case
    for fill in FILLS:
        with alloc_fill(hostcheck, fill):
            got = prove_mixed(hostcheck, tparams, cparams, mf, xc.SUMCHECK_K, xc.SUMCHECK_LABELS, ws, q)
        assert got == want(mf, q), "fill 0x%02X" % fill
