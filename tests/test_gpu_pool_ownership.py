"""Pool accounting of refused calls on the GPU: a call that is refused AFTER it has taken pooled blocks (tree levels, FRI layers, z-powers, the
buffers of the sharded commit) returns every one of them.  Each case warms the pool with a succeeding call whose rounded block sizes cover the
failing one's and frees its handle, records stark_ctx_cached_bytes, makes the refused call, and asserts the code, the message and that the cached
bytes are unchanged (smaller: a block leaked; larger: the warm-up did not cover the sizes); the succeeding call then still returns the oracle's
roots.  Every refusal is an argument check: nothing is launched that could fault.  A context of its own, so the counts are exact.
Needs an MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED_Z = 0xDEEFBAAD
INVALID_ARG, UNSUPPORTED = -1, -5
ARITY_ONE = "arity 1 with more than one leaf"
vp = C.c_void_p
WARM = (8, [2])                                                    # the succeeding FRI shape: its blocks cover those of (6, [2]) and (3, [])


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


@pytest.fixture(scope="module")
def ctx():
    from stark_mlwe_amd.api import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data(oracle):
    """inputs and the oracle's roots, made once: 256 Merkle leaves; two f0 vectors of 8 elements with the layer roots of WARM"""
    leaves = oracle.rand_fr_columns(0xB10C, 256, 1)[0]
    t = oracle.merkle_build(16, 7, leaves); merkle_root = t.root().copy(); t.free()
    f = oracle.rand_fr_columns(0xB10D, 8, 2)
    n0, sched = WARM; roots = np.zeros((2, len(sched) + 1, 4), np.uint64)
    for b in range(2):
        pr = oracle.deep_fri_prove(None, None, None, None, n0, sched, 1, SEED_Z, f0=f[b])
        for l in range(len(sched) + 1):
            roots[b, l] = pr.root(l)
        pr.free()
    return {"leaves": dev(leaves), "merkle_root": merkle_root, "f": [dev(f[0]), dev(f[1])], "f_whole": dev(f[0]), "roots": roots}


def sched_ptr(sched):
    s = np.ascontiguousarray(sched if sched else [0], dtype=np.uint64)
    return s, s.ctypes.data_as(vp)


def merkle_call(ctx, data, first_pos):
    """stark_merkle_build_dev, arity 16, 256 leaves -> (rc, root or None); the tree is freed"""
    p = ctx.poseidon_params_for_width(17); h = vp(); root = np.zeros(4, np.uint64)
    rc = ctx.lib.stark_merkle_build_dev(ctx.h, p.h, 16, 7, vp(data["leaves"].data_ptr()), 256, 0, None, first_pos, 0, 0, C.byref(h))
    if rc != 0:
        assert not h.value
        return rc, None
    try:
        ctx._chk(ctx.lib.stark_merkle_root(h, root.ctypes.data_as(vp)))
    finally:
        ctx.lib.stark_merkle_free(h)
    return rc, root


def fri_build_call(ctx, data, n0, sched):
    s, sp = sched_ptr(sched); h = vp(); L = len(sched); roots = np.zeros((L + 1, 4), np.uint64)
    rc = ctx.lib.stark_fri_build_dev(ctx.h, vp(data["f"][0].data_ptr()), n0, sp, L, SEED_Z, C.byref(h))
    if rc != 0:
        assert not h.value
        return rc, None
    try:
        for l in range(L + 1):
            ctx._chk(ctx.lib.stark_fri_layer_root(h, l, roots[l].ctypes.data_as(vp)))
    finally:
        ctx.lib.stark_fri_state_free(h)
    return rc, roots


def commit_batch_call(ctx, data, n0, sched):
    s, sp = sched_ptr(sched); L = len(sched); roots = np.zeros((2, L + 1, 4), np.uint64)
    tab = (vp * 2)(data["f"][0].data_ptr(), data["f"][1].data_ptr())
    rc = ctx.lib.stark_fri_commit_batch_dev(ctx.h, 2, tab, n0, sp, L, SEED_Z, roots.ctypes.data_as(vp))
    return rc, roots if rc == 0 else None


def sharded_call(ctx, data, n0, sched):
    s, sp = sched_ptr(sched); L = len(sched); roots = np.zeros((2, L + 1, 4), np.uint64)                   # W = 2: every virtual rank's roots
    rc = ctx.lib.stark_diag_fri_build_sharded_emulated_dev(ctx.h, 2, vp(data["f_whole"].data_ptr()), n0, sp, L, SEED_Z, roots.ctypes.data_as(vp))
    return rc, roots if rc == 0 else None


# name -> (the succeeding call, what it must return, the refused calls, their code and message)
CASES = {
    "merkle_build_dev first_pos=1": (lambda c, d: merkle_call(c, d, 0), lambda d: d["merkle_root"],
                                     [lambda c, d: merkle_call(c, d, 1)], INVALID_ARG, "shard offset not aligned"),
    "fri_build_dev": (lambda c, d: fri_build_call(c, d, *WARM), lambda d: d["roots"][0],
                      [lambda c, d: fri_build_call(c, d, 6, [2]), lambda c, d: fri_build_call(c, d, 3, [])], UNSUPPORTED, ARITY_ONE),
    "fri_commit_batch_dev B=2": (lambda c, d: commit_batch_call(c, d, *WARM), lambda d: d["roots"],
                                 [lambda c, d: commit_batch_call(c, d, 6, [2])], UNSUPPORTED, ARITY_ONE),
    "fri_build_sharded_emulated W=2": (lambda c, d: sharded_call(c, d, *WARM), lambda d: np.stack([d["roots"][0]] * 2),
                                       [lambda c, d: sharded_call(c, d, 6, [2])], UNSUPPORTED, ARITY_ONE),
}


def refusals_return_their_blocks(ctx, data, name):
    good, want_of, bad_calls, want_rc, want_msg = CASES[name]
    lib = ctx.lib; want = want_of(data)
    rc, got = good(ctx, data)                                                              # warms the pool; its handle is freed
    assert rc == 0 and (got == want).all(), (name, rc, lib.stark_last_error(ctx.h))
    for i, bad in enumerate(bad_calls):
        cached = lib.stark_ctx_cached_bytes(ctx.h)
        rc, _ = bad(ctx, data)
        err = lib.stark_last_error(ctx.h).decode(); after = lib.stark_ctx_cached_bytes(ctx.h)
        print(name, i, "rc", rc, repr(err), "cached before", cached, "after", after)
        assert rc == want_rc and want_msg in err, (name, i, rc, err)
        assert after == cached, (name, i, "cached bytes before / after the refused call", cached, after)
        rc, got = good(ctx, data)
        assert rc == 0 and (got == want).all(), (name, i, rc)


@pytest.mark.parametrize("name", list(CASES))
def test_refused_call_returns_every_pooled_block(ctx, data, name):
    refusals_return_their_blocks(ctx, data, name)


def test_trim_after_refusals_empties_the_pool(ctx, data):
    """after every case stark_ctx_trim brings the cached bytes to 0, and the cases run again from the emptied pool cache exactly the bytes they
    cached from an empty pool before (that each refusal returned its blocks is the per-case assertion above)"""
    def all_cases():
        for name in CASES:
            refusals_return_their_blocks(ctx, data, name)
        return ctx.lib.stark_ctx_cached_bytes(ctx.h)
    ctx.trim()
    before = all_cases()
    assert before > 0
    ctx.trim()
    assert ctx.lib.stark_ctx_cached_bytes(ctx.h) == 0
    assert all_cases() == before
