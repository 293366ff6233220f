"""Many Merkle trees in one pass (stark_mlwe_amd/csrc/merkle_batch.hpp) on the CPU: the build, open and verify drivers the device entry points
run (stark_merkle_build_batch_dev, stark_merkle_open_batch, stark_merkle_verify_many_ds_batch), instantiated over the host bodies of the DS
streams (hostcheck.cpp hc_merkle_*), against the oracle's MerkleTree / open / verify_many_ds (oracle/merkle.hpp)."""
import ctypes as C

import numpy as np
import pytest

import merkle_batch_cases as mc

vp = C.c_void_p
SEED = 0xB47C


def P(a):
    return None if a is None else a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def hc_params(hostcheck):
    made = {}

    def get(arity):
        t = 9 if arity <= 8 else 17 if arity <= 16 else 33 if arity <= 32 else 65 if arity <= 64 else 129
        if t not in made:
            made[t] = hostcheck.params(0, t)
        return made[t]
    yield get
    for h in made.values():
        hostcheck.params_free(h)


def hc_build_rc(hostcheck, params, arity, labels, cols, n, cps=None):
    """-> (the export's return value, (lens, [levels of tree b]) or None when it is negative) through hc_merkle_build_batch"""
    B = len(cols); lens = np.zeros(64, np.uint64)
    tab = (vp * B)(*[c.ctypes.data for c in cols])
    ctab = None if cps is None else (vp * B)(*[None if c is None else c.ctypes.data for c in cps])
    cap = 2 * B * n + 64 * B
    out = np.zeros((cap, 4), np.uint64); lab = np.ascontiguousarray(labels, dtype=np.uint64)
    nl = hostcheck.l.hc_merkle_build_batch(params, C.c_size_t(arity), C.c_size_t(B), P(lab), tab, C.c_size_t(n), 0 if cps is None else 1, ctab, P(out), C.c_size_t(cap), P(lens))
    if nl < 0:
        return nl, None
    lens = [int(x) for x in lens[:nl]]; trees = [[] for _ in range(B)]; at = 0
    for ln in lens:
        for b in range(B):
            trees[b].append(out[at + b * ln: at + (b + 1) * ln].copy())
        at += B * ln
    return nl, (lens, trees)


def hc_build(hostcheck, params, arity, labels, cols, n, cps=None):
    """-> (lens, [levels of tree b]) through hc_merkle_build_batch, or None when the shape is refused"""
    return hc_build_rc(hostcheck, params, arity, labels, cols, n, cps)[1]


def hc_open(hostcheck, arities, trees, index_lists):
    """-> list of proof bytes through hc_merkle_open_batch, or None when the arguments are refused; trees[b] = list of level arrays"""
    B = len(trees); hostcheck.l.hc_merkle_open_batch.restype = C.c_long
    flat = [np.ascontiguousarray(l) for t in trees for l in t]
    ltab = (vp * max(1, len(flat)))(*[l.ctypes.data for l in flat]); lens = np.array([l.shape[0] for l in flat], np.uint64)
    ar = np.array(arities, np.uint64); nlev = np.array([len(t) for t in trees], np.uint64)
    off = np.zeros(B + 1, np.uint64); off[1:] = np.cumsum([len(ix) for ix in index_lists])
    ix = np.array([i for l in index_lists for i in l], np.uint64); out_lens = np.zeros(B, np.uint64)
    tot = hostcheck.l.hc_merkle_open_batch(C.c_size_t(B), P(ar), P(nlev), ltab, P(lens), P(ix), P(off), None, C.c_size_t(0), P(out_lens))
    if tot < 0:
        return None
    buf = (C.c_uint8 * max(1, tot))()
    assert hostcheck.l.hc_merkle_open_batch(C.c_size_t(B), P(ar), P(nlev), ltab, P(lens), P(ix), P(off), buf, C.c_size_t(tot), P(out_lens)) == tot
    raw = bytes(buf)[:tot]; res = []; o = 0
    for b in range(B):
        res.append(raw[o:o + int(out_lens[b])]); o += int(out_lens[b])
    return res


def hc_verify(hostcheck, cfg_arity, items, max_slots=0, misalign=False):
    """items: (label, root, idx, values, proof) -> list of 0 / 1 through hc_merkle_verify_batch; misalign: roots and values at addresses 8 mod 16"""
    B = len(items)
    lab = np.array([it[0] for it in items], np.uint64); roots = np.ascontiguousarray(np.stack([np.asarray(it[1], np.uint64).reshape(4) for it in items]))
    off = np.zeros(B + 1, np.uint64); off[1:] = np.cumsum([len(it[2]) for it in items])
    ix = np.array([i for it in items for i in it[2]], np.uint64)
    vals = np.ascontiguousarray(np.concatenate([np.asarray(it[3], np.uint64).reshape(-1, 4) for it in items]))
    if misalign:
        roots, vals = mc.off8(roots), mc.off8(vals)
    bufs = [(C.c_uint8 * max(1, len(it[4]))).from_buffer_copy(it[4] or b"\0") for it in items]
    ptrs = (vp * B)(*[C.cast(b, vp) for b in bufs]); lens = np.array([len(it[4]) for it in items], np.uint64); acc = np.full(B, -7, np.int32)
    rc = hostcheck.l.hc_merkle_verify_batch(C.c_size_t(cfg_arity), C.c_size_t(B), P(lab), P(roots), P(ix), P(off), P(vals), ptrs, P(lens), C.c_size_t(max_slots), P(acc))
    assert rc == 0, rc
    return [int(a) for a in acc]


def batch_inputs(oracle, arity, n, pairs, B):
    labels = mc.labels_of(B)
    cols = [mc.leaves_of(oracle, SEED, b, n) for b in range(B)]
    cps = None if not pairs else [None if b == B - 1 else mc.leaves_of(oracle, SEED, b + 100, n) for b in range(B)]      # the last tree: a NULL cp entry
    want = [mc.oracle_tree(oracle, SEED, b, arity, n, pairs, labels[b], pairs and b == B - 1) for b in range(B)]
    return labels, cols, cps, want


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("arity,n,pairs", mc.SHAPES)
def test_build_open_verify_equal_the_oracle(oracle, hostcheck, hc_params, arity, n, pairs, B):
    """every level of every tree, the opening bytes (duplicates, the last leaf of a ragged tree) and the accept / reject of the honest and every
    tampered opening are the oracle's, tree by tree, with distinct labels (and a NULL cp entry in the pair table)"""
    labels, cols, cps, want = batch_inputs(oracle, arity, n, pairs, B)
    lens, trees = hc_build(hostcheck, hc_params(arity), arity, labels, cols, n, cps)
    for b in range(B):
        assert len(trees[b]) == want[b].num_levels() == len(lens)
        for v in range(len(lens)):
            assert (trees[b][v] == want[b].level(v)).all(), (b, v)
    ixs = [mc.index_lists(n, b) for b in range(B)]
    proofs = hc_open(hostcheck, [arity] * B, trees, ixs)
    items, expect, names = [], [], []
    for b in range(B):
        assert proofs[b] == want[b].open_bytes(ixs[b]), b
        vals = trees[b][0][ixs[b]]
        for name, lab, root, ix, v, pr in mc.tamperings(labels[b], trees[b][-1][0], ixs[b], vals, proofs[b], n):
            items.append((lab, root, ix, v, pr)); names.append((b, name)); expect.append(mc.oracle_verify(arity, lab, root, ix, v, pr))
    assert expect[0] == 1 and all(e == 0 for (b, nm), e in zip(names, expect) if nm != "honest"), list(zip(names, expect))
    assert hc_verify(hostcheck, arity, items) == expect, names
    assert hc_verify(hostcheck, arity, items, max_slots=1) == expect                 # one plan per item: the chunked path gives the same answers
    assert hc_verify(hostcheck, arity, items, misalign=True) == expect               # roots and values behind a uint64_t pointer that is 8 mod 16


def test_open_batch_over_trees_of_different_shapes_and_refusals(oracle, hostcheck, hc_params):
    """one open call over trees of different arity and height equals the oracle's openings; an empty list, an index past the leaves and a
    non-monotone idx_off are refused before anything is read"""
    shapes = [(16, 257, 11), (8, 65, 12), (16, 1, 13)]
    ot = [mc.oracle_tree(oracle, SEED, b, a, n, False, lab, False) for b, (a, n, lab) in enumerate(shapes)]
    trees = [[t.level(v) for v in range(t.num_levels())] for t in ot]
    ixs = [[256, 3, 3, 17], [64, 0], [0, 0]]
    got = hc_open(hostcheck, [s[0] for s in shapes], trees, ixs)
    assert got == [t.open_bytes(ix) for t, ix in zip(ot, ixs)]
    assert hc_open(hostcheck, [s[0] for s in shapes], trees, [[1], [], [0]]) is None
    assert hc_open(hostcheck, [s[0] for s in shapes], trees, [[257], [0], [0]]) is None
    assert hc_open(hostcheck, [s[0] for s in shapes], trees, [[1], [0], [1]]) is None


def test_refused_shapes(oracle, hostcheck, hc_params):
    """the build driver's shape guards: no leaves, an arity of another width, arity 1 with more than one leaf, pairs without a cp table"""
    col = [mc.leaves_of(oracle, SEED, 0, 8)]
    assert hc_build(hostcheck, hc_params(16), 8, [1], col, 8) is None                  # arity 8 needs t = 9
    assert hc_build(hostcheck, hc_params(8), 1, [1], col, 8) is None                   # arity 1, n > 1
    lens, trees = hc_build(hostcheck, hc_params(8), 1, [1], col, 1)                    # arity 1, one leaf: the root is the leaf
    assert lens == [1] and (trees[0][0] == col[0][:1]).all()
