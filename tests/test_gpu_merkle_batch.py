"""Many Merkle trees in one device pass: stark_merkle_build_batch_dev, stark_commitment_commit_batch_dev, stark_merkle_roots_batch,
stark_merkle_open_batch and stark_merkle_verify_many_ds_batch against the single calls (stark_merkle_build_dev, stark_merkle_open,
stark_merkle_verify_many_ds, stark_commitment_commit / _verify) item by item and byte for byte, and against the CPU oracle for one shape per
Poseidon width.  Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import merkle_batch_cases as mc
from test_gpu_guard_bands import Band, SENTINEL

pytestmark = pytest.mark.gpu
vp = C.c_void_p
SEED = 0xB47C
# (arity, n, pairs, B): the shared shapes at B = 1 and 3; 2 x 257 level-1 nodes (one wave per node), 17 x 257 = 4369 (the wave pair), 300 root hashes
# (past the 256 of the five-wave form); t = 33 and t = 129 once each
CASES = [s + (B,) for s in mc.SHAPES for B in mc.BATCHES] + [(16, 4097, False, 2), (16, 4097, False, 17), (16, 16, False, 300), (32, 33, False, 2), (128, 129, True, 2)]
ORACLE_CASES = [(16, 257, False), (8, 65, False), (4, 64, True), (64, 65, False), (32, 33, False), (128, 129, True)]       # one per width (t = 9 plain and as pairs)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def hp(a):
    return None if a is None else a.ctypes.data_as(vp)


def tab(ptrs):
    return (vp * max(len(ptrs), 1))(*[None if p is None else int(p) for p in ptrs])


class Single:
    """stark_merkle_build_dev of one column: its levels, root and openings (the reference of the batch; computed once, under the default options)"""

    def __init__(self, ctx, arity, label, f, cp):
        from stark_mlwe_amd.api import MerkleTree
        h = vp(); fd = dev(f); cd = None if cp is None else dev(cp)
        ctx._chk(ctx.lib.stark_merkle_build_dev(ctx.h, ctx.poseidon_params_for_arity(arity).h, arity, label, vp(fd.data_ptr()), f.shape[0], 0 if cp is None else 1,
                                                None if cp is None else vp(cd.data_ptr()), 0, 0, 0, C.byref(h)))
        t = MerkleTree(ctx, h, None)
        self.levels = t.levels; self.root = t.root(); self.n = f.shape[0]; self.opened = {}; self.tree = t

    def open(self, ix):
        k = tuple(int(i) for i in ix)
        if k not in self.opened:
            self.opened[k] = self.tree.open_many(list(k))
        return self.opened[k]


_singles = {}


def columns(oracle, arity, n, pairs, B):
    """host columns of a batch: f of every tree, cp of every tree of a pair batch (the last one None = zeros)"""
    fs = [mc.leaves_of(oracle, SEED, b, n) for b in range(B)]
    cps = None if not pairs else [None if b == B - 1 else mc.leaves_of(oracle, SEED, b + 100, n) for b in range(B)]
    return fs, cps


def single(ctx, oracle, arity, n, pairs, B, b):
    key = (arity, n, pairs, b, pairs and b == B - 1)
    if key not in _singles:
        f = mc.leaves_of(oracle, SEED, b, n)
        cp = None if not pairs else (np.zeros((n, 4), np.uint64) if b == B - 1 else mc.leaves_of(oracle, SEED, b + 100, n))
        _singles[key] = Single(ctx, arity, mc.labels_of(B)[b], f, cp)
    return _singles[key]


def build_batch(ctx, arity, labels, fd, n, cd=None):
    """-> list of MerkleTree through stark_merkle_build_batch_dev (fd / cd: device tensors or None)"""
    return ctx.merkle_build_batch_dev([t.data_ptr() for t in fd], n, arity, labels, ctx.poseidon_params_for_arity(arity),
                                      None if cd is None else [None if t is None else t.data_ptr() for t in cd])


def check_batch(ctx, oracle, arity, n, pairs, B, with_oracle=False):
    fs, cps = columns(oracle, arity, n, pairs, B); labels = mc.labels_of(B)
    fd = [dev(f) for f in fs]; cd = None if cps is None else [None if c is None else dev(c) for c in cps]
    trees = build_batch(ctx, arity, labels, fd, n, cd)
    refs = [single(ctx, oracle, arity, n, pairs, B, b) for b in range(B)]
    roots = ctx.merkle_roots_batch(trees)
    ixs = [mc.index_lists(n, b) for b in range(B)]
    opened = ctx.merkle_open_batch(trees, ixs)
    for b, (t, r) in enumerate(zip(trees, refs)):
        assert t.num_levels == len(r.levels), b
        for v, want in enumerate(r.levels):
            assert (t.level(v) == want).all(), "tree %d level %d" % (b, v)
        assert (t.root() == r.root).all() and (roots[b] == r.root).all(), b
        assert t.open_many(ixs[b]) == r.open(ixs[b]) == opened[b], b
    if with_oracle:
        for b in range(B):
            o = mc.oracle_tree(oracle, SEED, b, arity, n, pairs, labels[b], pairs and b == B - 1)
            assert all((refs[b].levels[v] == o.level(v)).all() for v in range(o.num_levels())) and opened[b] == o.open_bytes(ixs[b]), b
    for t in trees:
        t.free()


@pytest.mark.parametrize("arity,n,pairs,B", CASES)
def test_batch_build_equals_single_builds(gpu_ctx, oracle, arity, n, pairs, B):
    """every level, root (one by one and through stark_merkle_roots_batch) and opening (stark_merkle_open and stark_merkle_open_batch) of every
    handle of a batch equals stark_merkle_build_dev on that column alone; one shape per width is also the oracle's"""
    check_batch(gpu_ctx, oracle, arity, n, pairs, B, with_oracle=(arity, n, pairs) in ORACLE_CASES and B <= 3)


@pytest.mark.parametrize("option", ["sponge_one_wave", "poseidon_lane_only"])
def test_batch_build_under_the_other_kernel_forms(gpu_ctx, oracle, option):
    """the same comparison with the small levels on the one-wave / wave-pair kernels and with every level on one lane per sponge"""
    gpu_ctx.set_option(option, 1)
    try:
        for arity, n, pairs, B in CASES:
            check_batch(gpu_ctx, oracle, arity, n, pairs, B)
    finally:
        gpu_ctx.set_option(option, 0)


def test_handles_outlive_each_other_and_a_pointer_may_repeat(gpu_ctx, oracle):
    """half the batch freed, other trees built into the pool, then the rest opened: the bytes are what they were; the same column twice in `leaves`
    gives two trees that differ only by their labels"""
    arity, n, B = 16, 257, 6
    fs, _ = columns(oracle, arity, n, False, B); labels = mc.labels_of(B)
    fd = [dev(f) for f in fs]
    trees = build_batch(gpu_ctx, arity, labels, fd, n)
    ixs = [mc.index_lists(n, b) for b in range(B)]
    before = gpu_ctx.merkle_open_batch(trees, ixs)
    for b in (0, 2, 4):
        trees[b].free()
    other = build_batch(gpu_ctx, arity, [99, 98], [fd[5], fd[5]], n)          # same shape: would reuse the blocks had they gone back to the pool
    again = gpu_ctx.merkle_build_batch_dev([fd[0].data_ptr()], n, arity, [labels[0]], gpu_ctx.poseidon_params_for_arity(arity))
    for b in (1, 3, 5):
        assert trees[b].open_many(ixs[b]) == before[b] == single(gpu_ctx, oracle, arity, n, False, B, b).open(ixs[b])
        assert (trees[b].root() == single(gpu_ctx, oracle, arity, n, False, B, b).root).all()
    assert gpu_ctx.merkle_open_batch(again, [ixs[0]])[0] == before[0]
    twin = [Single(gpu_ctx, arity, lab, fs[5], None) for lab in (99, 98)]
    for t, w in zip(other, twin):
        assert all((t.level(v) == w.levels[v]).all() for v in range(len(w.levels)))
    assert not (other[0].root() == other[1].root()).all()
    for t in [trees[1], trees[3], trees[5]] + other + again + [w.tree for w in twin]:
        t.free()


def test_open_batch_over_mixed_trees_and_commit_batch(gpu_ctx, oracle):
    """one stark_merkle_open_batch over batch-built and single-built trees of different shapes equals the single opens; stark_commitment_commit_batch_dev
    equals stark_commitment_commit tree by tree and its openings pass stark_commitment_verify"""
    a = single(gpu_ctx, oracle, 16, 257, False, 3, 1); c = single(gpu_ctx, oracle, 8, 65, False, 3, 0); one = single(gpu_ctx, oracle, 16, 1, False, 3, 2)
    fs, _ = columns(oracle, 64, 65, False, 2); fd = [dev(f) for f in fs]
    wide = build_batch(gpu_ctx, 64, [5, 6], fd, 65)
    mixed = [a.tree, wide[1], c.tree, one.tree, wide[0]]; ixs = [[256, 0, 0, 77], [64, 1], [3, 64, 3], [0], [0, 63, 64]]
    got = gpu_ctx.merkle_open_batch(mixed, ixs)
    assert got == [t.open_many(ix) for t, ix in zip(mixed, ixs)]
    assert (gpu_ctx.merkle_roots_batch(mixed) == np.stack([t.root() for t in mixed])).all()
    for t in wide:
        t.free()
    n, tags = 273, [11, 12, 13]
    cols = [mc.leaves_of(oracle, SEED, 40 + b, n) for b in range(3)]; cd = [dev(x) for x in cols]
    trees = gpu_ctx.commitment_commit_batch_dev(tags, [t.data_ptr() for t in cd], n)
    ix = [272, 5, 5, 16]
    opened = gpu_ctx.merkle_open_batch(trees, [ix] * 3)
    for b in range(3):
        root, ref = gpu_ctx.commitment_commit(tags[b], cols[b])
        assert all((trees[b].level(v) == ref.level(v)).all() for v in range(ref.num_levels)) and (trees[b].root() == root).all()
        assert opened[b] == ref.open_many(ix) and gpu_ctx.commitment_verify(tags[b], root, ix, cols[b][ix], opened[b])
        assert (root == oracle.commitment_root(tags[b], cols[b])).all()
        ref.free(); trees[b].free()


def test_verify_batch_matches_the_single_verifier_item_by_item(gpu_ctx, oracle):
    """16 openings of trees of four heights — honest ones and one of each tampering (value bit, sibling bit, wrong root, truncated, empty, index out of
    range) — in one stark_merkle_verify_many_ds_batch: every decision is stark_merkle_verify_many_ds's on that item alone, and the oracle's"""
    items, names = [], []
    for n, b in ((4097, 0), (257, 1), (17, 2), (1, 2), (257, 0)):
        s = single(gpu_ctx, oracle, 16, n, False, 2 if n == 4097 else 3, b); ix = mc.index_lists(n, b); lab = mc.labels_of(3)[b]
        cases = mc.tamperings(lab, s.root, ix, s.levels[0][ix], s.open(ix), n)
        for c in (cases if (n, b) == (257, 1) else cases[:1]):
            items.append(c[1:]); names.append((n, b, c[0]))
        if (n, b) in ((4097, 0), (17, 2), (257, 0)):
            ix2 = [0, n - 1, 1]
            items.append((lab, s.root, ix2, s.levels[0][ix2], s.open(ix2))); names.append((n, b, "honest 2"))
        if n == 17:
            items.append((lab + 1, s.root, ix, s.levels[0][ix], s.open(ix))); names.append((n, b, "other label"))
            items.append((lab, s.root, [], s.levels[0][:0], s.open(ix))); names.append((n, b, "no index"))
    assert len(items) == 16 and {nm[2] for nm in names} >= {"honest", "value bit", "sibling bit", "wrong root", "truncated", "empty", "index out of range"}
    cfg = gpu_ctx.merkle_cfg(16)
    want = [mc.oracle_verify(16, *it) == 1 for it in items]                 # every item's decision is the oracle's; the single call plans a batch of one
    assert want == [nm[2].startswith("honest") for nm in names]
    alone = [gpu_ctx.merkle_verify_single(cfg.with_tree_label(lab), root, ix, v, pr) for lab, root, ix, v, pr in items]
    assert alone == want, list(zip(names, alone, want))
    got = gpu_ctx.merkle_verify_single_batch(16, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items], [it[3] for it in items], [it[4] for it in items])
    assert got == want, list(zip(names, got, want))


def test_verify_batch_reads_roots_and_values_at_eight_byte_alignment(gpu_ctx, oracle):
    """`roots` and `values` are uint64_t pointers: buffers whose address is 8 mod 16 (a root behind a u64 in a struct, a Rust `&[F]`) give the
    decisions of the single call, which takes the same pointers, and of the oracle"""
    lib, h = gpu_ctx.lib, gpu_ctx.h
    s = single(gpu_ctx, oracle, 16, 257, False, 3, 1); ix = mc.index_lists(257, 1); lab = mc.labels_of(3)[1]; pr = s.open(ix)
    vals = s.levels[0][ix]; bad = mc.flip_bit(vals, 1, 3)
    rt = mc.off8(np.stack([s.root, s.root])); va = mc.off8(np.concatenate([vals, bad]))
    ixa = np.array(ix + ix, np.uint64); off = np.array([0, len(ix), 2 * len(ix)], np.uint64); labs = np.array([lab, lab], np.uint64)
    buf = (C.c_uint8 * len(pr)).from_buffer_copy(pr); ptrs = (vp * 2)(C.cast(buf, vp), C.cast(buf, vp)); lens = np.array([len(pr)] * 2, np.uint64)
    acc = np.full(2, 7, np.int32)
    gpu_ctx._chk(lib.stark_merkle_verify_many_ds_batch(h, 16, 2, hp(labs), hp(rt), hp(ixa), hp(off), hp(va), ptrs, hp(lens), hp(acc)))
    want = []
    for b in range(2):
        ok = C.c_int32(7)
        gpu_ctx._chk(lib.stark_merkle_verify_many_ds(h, 16, lab, hp(rt[b]), hp(ixa), len(ix), hp(va[b * len(ix):(b + 1) * len(ix)]), buf, len(pr), C.byref(ok)))
        want.append(ok.value)
    assert [int(a) for a in acc] == want == [1, 0]
    assert want == [int(mc.oracle_verify(16, lab, s.root, ix, v, pr) == 1) for v in (vals, bad)]
    roots = mc.off8(np.zeros((2, 4), np.uint64))                             # and the roots come back into such a buffer
    gpu_ctx._chk(lib.stark_merkle_roots_batch(tab([s.tree.h.value, s.tree.h.value]), 2, hp(roots)))
    assert (roots == s.root).all()


def test_guard_bands_and_pool_contents(gpu_ctx, oracle):
    """`leaves` and `cp` between sentinel bands (the columns of a batch consecutive payloads of one allocation, a sentinel row apart) stay intact, bands
    included, and the levels do not depend on what the pooled blocks held: they are overwritten with the sentinel, released and built into again"""
    from stark_mlwe_amd.api import MerkleTree
    for arity, n, pairs, B in ((16, 257, False, 3), (4, 64, True, 3)):
        fs, cps = columns(oracle, arity, n, pairs, B); labels = mc.labels_of(B)
        fb = Band(fs, band=512); cb = None if not pairs else Band([c for c in cps if c is not None], band=512)
        cptrs = None if not pairs else [None if cps[b] is None else cb.ptr(b).value for b in range(B)]
        refs = [single(gpu_ctx, oracle, arity, n, pairs, B, b) for b in range(B)]
        for round_ in range(2):
            trees = gpu_ctx.merkle_build_batch_dev([fb.ptr(b).value for b in range(B)], n, arity, labels, gpu_ctx.poseidon_params_for_arity(arity), cptrs)
            for b in range(B):
                assert all((trees[b].level(v) == refs[b].levels[v]).all() for v in range(len(refs[b].levels))), (round_, b)
            fb.check_unchanged("stark_merkle_build_batch_dev leaves")
            if cb is not None:
                cb.check_unchanged("stark_merkle_build_batch_dev cp")
            for v in range(trees[0].num_levels):                           # tree 0's level pointer is the start of the batch's block of that level
                ln = gpu_ctx.lib.stark_merkle_level_len(trees[0].h, v); junk = np.full((B * ln, 4), SENTINEL, np.uint64)
                gpu_ctx._chk(gpu_ctx.lib.stark_memcpy_h2d(gpu_ctx.h, vp(gpu_ctx.lib.stark_merkle_level_dev(trees[0].h, v)), hp(junk), junk.nbytes))
            for t in trees:
                t.free()


def test_refused_arguments(gpu_ctx, oracle):
    """the refused-argument list of include/stark_mlwe.h: the stated code, every out[i] NULL and every accepted[i] 0, nothing launched"""
    lib, h = gpu_ctx.lib, gpu_ctx.h
    n, B = 17, 2
    fd = [dev(mc.leaves_of(oracle, SEED, b, n)) for b in range(B)]
    p17, p9 = gpu_ctx.poseidon_params_for_arity(16).h, gpu_ctx.poseidon_params_for_arity(8).h
    lab = np.array([1, 2], np.uint64); leaves = tab([t.data_ptr() for t in fd])

    def build(ctx=h, p=p17, arity=16, batch=B, labels=lab, lv=leaves, n_=n, pairs=0, cp=None, null_out=False):
        out = (vp * B)(*[vp(0xDEAD)] * B)
        rc = lib.stark_merkle_build_batch_dev(ctx, p, arity, batch, hp(labels), lv, n_, pairs, cp, None if null_out else out)
        return rc, [out[b] for b in range(B)]
    assert build(batch=0)[0] == 0
    for kw in (dict(ctx=None), dict(p=None), dict(labels=None), dict(lv=None), dict(lv=tab([fd[0].data_ptr(), None])), dict(pairs=1), dict(n_=0), dict(arity=8), dict(arity=0), dict(p=p9)):
        rc, out = build(**kw)
        assert rc == -1 and out == [None, None], kw
    assert build(null_out=True)[0] == -1
    rc, out = build(p=p9, arity=1)
    assert rc == -5 and out == [None, None]                                  # arity 1 with n > 1: STARK_ERR_UNSUPPORTED, as the single build
    out = (vp * B)(*[vp(0xDEAD)] * B)
    assert lib.stark_commitment_commit_batch_dev(h, B, None, leaves, n, out) == -1 and [out[b] for b in range(B)] == [None, None]
    assert lib.stark_commitment_commit_batch_dev(h, B, hp(lab), leaves, 0, out) == -1
    # open: trees of one context, monotone offsets, no empty list, indices in range
    trees = gpu_ctx.merkle_build_batch_dev([t.data_ptr() for t in fd], n, 16, [1, 2], gpu_ctx.poseidon_params_for_arity(16))
    tt = tab([t.h.value for t in trees])

    def open_(tr=tt, idx=(0, 16, 3), off=(0, 2, 3), null_out=False):
        ix = np.array(idx, np.uint64); of = np.array(off, np.uint64); out = (vp * B)(*[vp(0xDEAD)] * B)
        rc = lib.stark_merkle_open_batch(tr, B, hp(ix), hp(of), None if null_out else out)
        return rc, [out[b] for b in range(B)]
    rc, out = open_()
    assert rc == 0 and all(out)
    for o in out:
        lib.stark_proof_free(vp(o))
    for kw in (dict(off=(0, 2, 2)), dict(off=(0, 3, 2)), dict(idx=(0, 17, 3)), dict(tr=None), dict(tr=tab([trees[0].h.value, None])), dict(off=(0, 0, 3))):
        rc, out = open_(**kw)
        assert rc == -1 and out == [None, None], kw
    assert open_(null_out=True)[0] == -1
    from stark_mlwe_amd.api import Context
    ctx2 = Context(0)
    try:
        f2 = dev(mc.leaves_of(oracle, SEED, 0, n))
        t2 = ctx2.merkle_build_batch_dev([f2.data_ptr()], n, 16, [1], ctx2.poseidon_params_for_arity(16))
        rc, out = open_(tr=tab([trees[0].h.value, t2[0].h.value]))
        assert rc == -1 and out == [None, None]
        roots = np.zeros((2, 4), np.uint64)
        assert lib.stark_merkle_roots_batch(tab([trees[0].h.value, t2[0].h.value]), 2, hp(roots)) == -1
        ctx2.sync(); t2[0].free()
    finally:
        ctx2.close()
    # verify: null tables, a non-monotone idx_off, an unsupported cfg_arity
    ix = [0, 16]; pr = trees[0].open_many(ix); root = trees[0].root(); vals = trees[0].level(0)[ix]
    buf = (C.c_uint8 * len(pr)).from_buffer_copy(pr); ptrs = (vp * 2)(C.cast(buf, vp), C.cast(buf, vp)); lens = np.array([len(pr)] * 2, np.uint64)
    rt = np.stack([root, root]); ixa = np.array(ix + ix, np.uint64); va = np.concatenate([vals, vals]); labs = np.array([1, 1], np.uint64)

    def verify(ctx=h, arity=16, labels=labs, roots=rt, off=(0, 2, 4), pp=ptrs, ln=lens):
        acc = np.full(2, 7, np.int32)
        rc = lib.stark_merkle_verify_many_ds_batch(ctx, arity, 2, hp(labels), hp(roots), hp(ixa), hp(np.array(off, np.uint64)), hp(va), pp, hp(ln), hp(acc))
        return rc, [int(a) for a in acc]
    assert verify() == (0, [1, 1])
    for kw in (dict(ctx=None), dict(labels=None), dict(roots=None), dict(off=(0, 3, 2)), dict(pp=None), dict(ln=None)):
        assert verify(**kw) == (-1, [0, 0]), kw
    assert verify(arity=129) == (-5, [0, 0]) and verify(arity=0) == (-5, [0, 0])
    assert lib.stark_merkle_verify_many_ds_batch(h, 16, 0, None, None, None, None, None, None, None, None) == 0
    for t in trees:
        t.free()
