"""stark_sumcheck_verify_plain_batch / _mf_batch on the GPU (capi_sumcheck.hip: the plan of sumcheck_verify_batch.hpp — device decode,
transcript streams, one DS launch per tree depth, the check kernels, one download): every decision equals the single entry point's (the same driver with B = 1) and
the oracle's verify_plain / verify_mf (channel/src/lib.rs:1080-1128, :1176-1240) on that proof alone.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sumcheck_verify_cases as cases
from stark_mlwe_amd.api import Context


def batch_call(ctx, mf, items):
    proofs = [it[0] for it in items]; labels = [it[2] for it in items]
    if mf:
        return ctx.verify_mf_batch(items[0][1], labels, items[0][3], proofs)
    return ctx.verify_plain_batch(items[0][1], None, proofs)


def single_call(ctx, mf, it):
    p, k, label, q = it[:4]
    return ctx.verify_mf(k, label, q, p) if mf else ctx.verify_plain(k, label, p)


@pytest.mark.parametrize("mf", [0, 1])
def test_gpu_mixed_batch_equals_single_and_oracle(gpu_ctx, oracle, mf):
    items, want = cases.mixed_batch(oracle, mf)
    assert all(w for it, w in zip(items, want) if it[4]) and 0 < sum(want) < len(want) // 2
    assert [single_call(gpu_ctx, mf, it) for it in items] == want
    got = batch_call(gpu_ctx, mf, items)
    assert got == want, [i for i in range(len(want)) if got[i] != want[i]]
    assert batch_call(gpu_ctx, mf, items[::-1]) == want[::-1]
    for i in (0, 1, 10, len(items) - 1):
        assert batch_call(gpu_ctx, mf, [items[i]]) == [want[i]], i
    assert gpu_ctx.verify_plain_batch(3, None, []) == [] and gpu_ctx.verify_mf_batch(3, [], 2, []) == []


_cache = {}


def gpu_batch(ctx, oracle, mf, k, B=64):
    """B proofs made on the GPU (8 witnesses, repeated) with a few tampered copies, the ORACLE's decision on each (one oracle call per distinct
    (proof, label): the single entry point is the batch driver with B = 1, so it is no independent witness) and the single entry point's"""
    key = (mf, k)
    if key not in _cache:
        ws = oracle.rand_fr_columns(900 + 2 * k + mf, 1 << k, 8)
        labels8 = [2025 + i for i in range(8)]
        honest = [ctx.prove_mf(k, labels8[i], 2, ws[i]) if mf else ctx.prove_plain(k, labels8[i], ws[i]) for i in range(8)]
        rng = random.Random(k + mf)
        items = [(honest[i % 8], k, labels8[i % 8], 2, True) for i in range(B)]
        for i in rng.sample(range(B), 6):
            bad = bytearray(items[i][0]); bad[rng.randrange(8, len(bad))] ^= 1 << rng.randrange(8)
            items[i] = (bytes(bad), k, items[i][2], 2, False)
        if mf:
            items[1] = (items[1][0], k, items[1][2] + 1, 2, False)
        memo = {}
        for it in items:
            if (it[0], it[2]) not in memo:
                memo[(it[0], it[2])] = oracle.sumcheck_verify(mf, k, it[2], it[0], q=2) == 1
        assert len(memo) <= 15
        want = [memo[(it[0], it[2])] for it in items]
        single = [single_call(ctx, mf, it) for it in items]
        _cache[key] = (items, want, single)
    return _cache[key]


@pytest.mark.parametrize("mf,k", [(0, 12), (0, 14), (1, 12), (1, 14)])
def test_gpu_made_proofs_batch_of_64(gpu_ctx, oracle, mf, k):
    items, want, single = gpu_batch(gpu_ctx, oracle, mf, k)
    assert len(items) == 64 and sum(want) >= 50 and not all(want)
    assert all(w for it, w in zip(items, want) if it[4])
    assert single == want
    assert batch_call(gpu_ctx, mf, items) == want


@pytest.mark.parametrize("option", ["poseidon_lane_only", "sponge_one_wave"])
def test_gpu_batch_under_forced_forms(gpu_ctx, oracle, option):
    c = Context(0)                                                            # a fresh context: the session's options stay as they are
    try:
        c.set_option(option, 1)
        for mf in (0, 1):
            items, want = cases.mixed_batch(oracle, mf)
            assert batch_call(c, mf, items) == want
            items, want, _ = gpu_batch(gpu_ctx, oracle, mf, 12)
            assert batch_call(c, mf, items) == want
    finally:
        c.close()


def test_gpu_batch_cut_into_several_plans(gpu_ctx, oracle):
    c = Context(0)
    try:
        c.set_option("sumcheck_verify_batch_max_slots", 64)                   # a few proofs per plan instead of 2^25 slots
        for mf in (0, 1):
            items, want = cases.mixed_batch(oracle, mf)
            assert batch_call(c, mf, items) == want
        c.set_option("sumcheck_verify_batch_max_slots", 1)                    # one proof per plan
        items, want = cases.mixed_batch(oracle, 1)
        assert batch_call(c, 1, items[:12]) == want[:12]
    finally:
        c.close()


def test_gpu_batch_invalid_arguments(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    p = b"\x01\x02\x03"; buf = (C.c_uint8 * 3).from_buffer_copy(p)
    ptrs = (C.c_void_p * 2)(C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p)); lens = (C.c_size_t * 2)(3, 3)
    lab = np.array([1, 2], np.uint64); L = lab.ctypes.data_as(C.c_void_p)
    acc = (C.c_int32 * 2)(7, 7)
    plain = lambda *a: lib.stark_sumcheck_verify_plain_batch(*a)
    mf = lambda ctx, n, pp, ll, k, labels, out: lib.stark_sumcheck_verify_mf_batch(ctx, n, pp, ll, k, labels, 2, out)
    for f in (plain, mf):
        assert f(h, 0, None, None, 3, None, None) == 0
        acc[0] = acc[1] = 7
        assert f(h, 2, ptrs, lens, 3, L, acc) == 0 and list(acc) == [0, 0]              # undecodable: rejected
        assert f(None, 2, ptrs, lens, 3, L, acc) == -1
        assert f(h, 2, ptrs, lens, 3, L, None) == -1
        acc[0] = acc[1] = 7
        assert f(h, 2, None, lens, 3, L, acc) == -1 and list(acc) == [0, 0]
        assert f(h, 2, ptrs, None, 3, L, acc) == -1
        holes = (C.c_void_p * 2)(C.cast(buf, C.c_void_p), None)
        assert f(h, 2, holes, lens, 3, L, acc) == -1
        lens0 = (C.c_size_t * 2)(3, 0); acc[0] = acc[1] = 7
        assert f(h, 2, holes, lens0, 3, L, acc) == 0 and list(acc) == [0, 0]            # a null, empty proof: rejected
    acc[0] = acc[1] = 7
    assert plain(h, 2, ptrs, lens, 3, None, acc) == 0 and list(acc) == [0, 0]           # the plain call reads no labels
    assert mf(h, 2, ptrs, lens, 3, None, acc) == -1 and list(acc) == [0, 0]
