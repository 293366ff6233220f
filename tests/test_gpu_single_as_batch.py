"""One trace is a batch of one: stark_deep_fri_prove_dev runs the batch provers with one trace (columns: prove_batch_impl, given f0:
prove_f0_batch_impl), stark_merkle_open is merkle_open_batch over one tree, stark_merkle_gather and the query phases share the one row gather, and
stark_build_f0_dev runs the batched challenge stage with one trace.  The smallest shapes that reach each driver, against the CPU oracle.
Needs an MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from stark_mlwe_amd.api import DeepFriParams, MerkleTree, StarkError

pytestmark = pytest.mark.gpu
vp = C.c_void_p
SEED_Z = 0xDEEFBAAD
INVALID_ARG = -1
# (n0, schedule, r): one layer pair with a one-element last layer; two folds; r * L = 0 (nothing is gathered); L = 0 (one layer, no query)
PROVE_SHAPES = [(16, [16], 3), (64, [8, 8], 4), (64, [8, 8], 0), (8, [], 3)]
# The oracle refuses r = 0 ("open_many: empty indices" from its first layer opening).  What the library answers for that call is pinned to what the
# commit BEFORE the single prove became a batch of one returned, for both entry forms, observed by running that commit once on an MI355X: literals.
PARENT_REFUSAL = {(64, (8, 8), 0): (INVALID_ARG, "query phase: bad index")}


@pytest.mark.parametrize("form", ["columns", "f0"])
@pytest.mark.parametrize("n0,sched,r", PROVE_SHAPES)
def test_single_prove_both_entry_forms(gpu_ctx, oracle, n0, sched, r, form):
    cols = oracle.rand_fr_columns(0x51C0 + n0, n0, 4)
    args = list(cols) if form == "columns" else [None] * 4
    f0 = None if form == "columns" else cols[0]
    prm = DeepFriParams(sched, r, SEED_Z)
    refusal = PARENT_REFUSAL.get((n0, tuple(sched), r))
    if refusal is not None:
        with pytest.raises(RuntimeError):
            oracle.deep_fri_prove(*args, n0, sched, r, SEED_Z, f0=f0)
        with pytest.raises(StarkError) as ei:
            gpu_ctx.deep_fri_prove(*args, n0, prm, f0=f0)
        print(n0, sched, r, form, ei.value.code, str(ei.value))
        assert ei.value.code == refusal[0] and str(ei.value) == "stark_mlwe error %d: %s" % refusal
        return
    ref = oracle.deep_fri_prove(*args, n0, sched, r, SEED_Z, f0=f0)
    got, est, ms = gpu_ctx.deep_fri_prove(*args, n0, prm, f0=f0)
    assert got == ref.bytes() and est == ref.size_estimate()
    assert all(m >= 0 for m in ms)
    ref.free()


OPEN_SHAPES = [(16, 55), (16, 1), (16, 4096), (8, 19), (2, 8)]          # ragged, one leaf (no sibling, nothing gathered), three full levels, t = 9 twice
REFERENCE_INDICES = [63, 0, 15, 16, 31, 47, 15]                         # merkle/src/lib.rs:948: unsorted, one duplicate


@pytest.fixture(scope="module")
def open_trees(gpu_ctx, oracle):
    """(arity, n) -> (device tree, oracle tree), built once"""
    out = {}
    for arity, n in OPEN_SHAPES:
        leaves = oracle.synth_column(0x0BE7, 3, 0, n)
        out[(arity, n)] = (gpu_ctx.merkle_new(leaves, gpu_ctx.merkle_cfg(arity, 9)), oracle.merkle_build(arity, 9, leaves))
    yield out
    for t, o in out.values():
        t.free(); o.free()


@pytest.mark.parametrize("arity,n", OPEN_SHAPES)
def test_single_open_is_the_batch_of_one_and_the_oracles(gpu_ctx, open_trees, arity, n):
    t, o = open_trees[(arity, n)]
    for idx in ([i % n for i in REFERENCE_INDICES], [n - 1]):
        got = t.open_many(idx)
        assert got == gpu_ctx.merkle_open_batch([t], [idx])[0], idx
        assert got == o.open_bytes(idx), idx


def last_error(ctx):
    return ctx.lib.stark_last_error(ctx.h).decode()


def test_single_open_refusals_and_the_two_call_protocol(gpu_ctx, oracle, open_trees):
    import torch
    lib = gpu_ctx.lib
    t, o = open_trees[(16, 55)]
    ln = C.c_size_t(12345)
    ix = np.array([54, 3], np.uint64); ixp = ix.ctypes.data_as(vp)
    assert lib.stark_merkle_open(t.h, None, 0, None, 0, C.byref(ln)) == INVALID_ARG and last_error(gpu_ctx) == "open_many: empty indices"
    bad = np.array([3, 55], np.uint64)
    assert lib.stark_merkle_open(t.h, bad.ctypes.data_as(vp), 2, None, 0, C.byref(ln)) == INVALID_ARG and last_error(gpu_ctx) == "leaf index out of range"
    # a partial tree: 64 leaves climbed to a level of four nodes
    leaves = torch.from_numpy(oracle.synth_column(0x0BE7, 3, 0, 64).view(np.int64)).cuda()
    h = vp()
    gpu_ctx._chk(lib.stark_merkle_build_dev(gpu_ctx.h, gpu_ctx.poseidon_params_for_arity(16).h, 16, 9, vp(leaves.data_ptr()), 64, 0, None, 0, 0, 4, C.byref(h)))
    part = MerkleTree(gpu_ctx, h, None)
    assert lib.stark_merkle_open(part.h, ixp, 2, None, 0, C.byref(ln)) == INVALID_ARG and last_error(gpu_ctx) == "cannot open a partial tree"
    part.free()
    assert ln.value == 12345                                                # no refusal wrote the length
    # length first, then the bytes; a buffer one byte short is refused after the length was written
    assert lib.stark_merkle_open(t.h, ixp, 2, None, 0, C.byref(ln)) == 0
    want = o.open_bytes([54, 3])
    assert ln.value == len(want)
    buf = (C.c_uint8 * len(want))(); ln2 = C.c_size_t(0)
    assert lib.stark_merkle_open(t.h, ixp, 2, buf, len(want), C.byref(ln2)) == 0 and ln2.value == len(want) and bytes(buf) == want
    ln3 = C.c_size_t(0)
    assert lib.stark_merkle_open(t.h, ixp, 2, buf, len(want) - 1, C.byref(ln3)) == INVALID_ARG and last_error(gpu_ctx) == "buffer too small" and ln3.value == len(want)


def test_gather_every_level(gpu_ctx, open_trees):
    t, _ = open_trees[(16, 55)]
    assert t.num_levels == 3
    for lvl in range(t.num_levels):
        level = t.level(lvl); n = level.shape[0]
        assert t.gather(lvl, []).shape == (0, 4)                            # k = 0
        idx = [n - 1, 0, n - 1, n // 2, 0]                                  # repeated indices
        assert (t.gather(lvl, idx) == level[idx]).all(), lvl
        with pytest.raises(StarkError) as ei:
            t.gather(lvl, [0, n])                                           # one past the level
        assert ei.value.code == INVALID_ARG and "gather index out of range" in str(ei.value)


@pytest.mark.parametrize("n0", [16, 1 << 10])
def test_build_f0_aux_of_one_trace(gpu_ctx, oracle, n0):
    """the challenge stage with one trace: column digests, seed_f, z, beta (aux7) and f0 are the oracle's; 16 rows are one absorbed block per column"""
    cols = oracle.rand_fr_columns(0xF0A + n0, n0, 4)
    f0, aux = gpu_ctx.build_f0(cols[0], cols[1], cols[2], cols[3], n0)
    w0, waux = oracle.build_f0(cols[0], cols[1], cols[2], cols[3], n0)
    assert (aux == waux).all() and (f0 == w0).all()
