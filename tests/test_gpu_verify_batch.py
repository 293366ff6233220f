"""stark_deep_fri_verify_batch on the GPU (capi_verify.hip: the plan of fri_verify_batch.hpp, one launch per Poseidon width and depth,
one download of the decisions): every decision equals stark_deep_fri_verify's and the oracle's deep_fri_verify (fri.rs:643-762) on
that proof alone, on GPU-made proofs of every Poseidon width (t = 9 .. 129), honest and tampered, in batches large enough that every
Merkle-level kernel form runs (five waves <= 256 hashes per step, one wave <= 4096, the wave pair above).  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from stark_mlwe_amd.api import Context, DeepFriParams

SEED_Z = 0xDEEFBAAD
SHAPES = [(1 << 10, [16, 8], 8), (1 << 11, [16, 16, 8], 32), (1 << 9, [8, 4, 2], 5), (1 << 10, [32, 32], 40), (1 << 12, [64, 64], 6), (2, [2], 1),
          (1 << 12, [128], 8)]


def plan_groups(hostcheck, proofs, sched, r):
    """(width, depth, hashes) of every DS launch step of the batch plan (host-check build of the same planner)"""
    n = len(proofs); bufs = [(C.c_uint8 * max(1, len(p))).from_buffer_copy(p or b"\0") for p in proofs]
    ptrs = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs]); lens = (C.c_size_t * n)(*[len(p) for p in proofs])
    sch = np.ascontiguousarray(sched, dtype=np.uint64); cap = 4096
    t, d, k = (C.c_int32 * cap)(), (C.c_uint32 * cap)(), (C.c_size_t * cap)()
    hostcheck.l.hc_verify_batch_groups.restype = C.c_size_t
    g = hostcheck.l.hc_verify_batch_groups(C.c_size_t(n), ptrs, lens, sch.ctypes.data_as(C.c_void_p), C.c_size_t(len(sched)), C.c_size_t(r), t, d, k, C.c_size_t(cap))
    return [(t[i], d[i], k[i]) for i in range(min(g, cap))]


def gpu_proof(ctx, oracle, n0, sched, r, seed):
    cols = oracle.rand_fr_columns(seed, n0, 4)
    proof, _, _ = ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, SEED_Z))
    return proof


def tampered(proof, rng, k):
    out = []
    for _ in range(k):
        bad = bytearray(proof); bad[rng.randrange(len(proof))] ^= 1 << rng.randrange(8); out.append(bytes(bad))
    return out


_cache = {}


def shape_batch(ctx, oracle, n0, sched, r):
    """honest, another n0, truncated / extended / empty, 40 bit flips, duplicates — and the oracle's decision on each"""
    key = (n0, tuple(sched), r)
    if key not in _cache:
        proof = gpu_proof(ctx, oracle, n0, sched, r, 2025 + n0)
        other = gpu_proof(ctx, oracle, 2 * n0, sched, r, 7 + n0)
        rng = random.Random(n0 * 31 + r)
        batch = [proof, other, b"", proof[:-1], proof + b"\0", other[:-8]] + tampered(proof, rng, 40)
        batch += [proof, batch[6], batch[-1]]
        want = [oracle.deep_fri_verify(p, sched, r, SEED_Z) == 1 for p in batch]
        _cache[key] = (batch, want)
    return _cache[key]


@pytest.mark.parametrize("n0,sched,r", SHAPES)
def test_gpu_batch_equals_single_and_oracle(gpu_ctx, oracle, n0, sched, r):
    batch, want = shape_batch(gpu_ctx, oracle, n0, sched, r)
    prm = DeepFriParams(sched, r, SEED_Z)
    assert want[0] and want[1] and not any(want[2:6])
    assert [gpu_ctx.deep_fri_verify(prm, p) for p in batch] == want
    got = gpu_ctx.deep_fri_verify_batch(prm, batch)
    assert got == want, [i for i in range(len(batch)) if got[i] != want[i]]
    assert gpu_ctx.deep_fri_verify_batch(prm, batch[::-1]) == want[::-1]
    assert gpu_ctx.deep_fri_verify_batch(prm, [batch[0]]) == [True]
    assert gpu_ctx.deep_fri_verify_batch(DeepFriParams(sched, r + 1, SEED_Z), batch[:2]) == [False, False]


def big_batch(ctx, oracle):
    """96 proofs at [16,16,8], r = 32: four honest ones (two n0), each repeated, and 32 tampered copies — over 4096 hashes of t = 17 at one depth"""
    n0, sched, r = 1 << 11, [16, 16, 8], 32
    if "big" not in _cache:
        honest = [gpu_proof(ctx, oracle, n0, sched, r, 40 + i) for i in range(3)] + [gpu_proof(ctx, oracle, 2 * n0, sched, r, 44)]
        rng = random.Random(96)
        batch = honest * 16 + tampered(honest[0], rng, 16) + tampered(honest[3], rng, 16)
        rng.shuffle(batch)
        want = [oracle.deep_fri_verify(p, sched, r, SEED_Z) == 1 for p in batch]
        _cache["big"] = (DeepFriParams(sched, r, SEED_Z), batch, want)
    return _cache["big"]


def test_gpu_batch_crosses_every_form(gpu_ctx, oracle, hostcheck):
    prm, batch, want = big_batch(gpu_ctx, oracle)
    sizes = {}
    for sub in (batch[:1], batch[:16], batch):
        sizes[len(sub)] = max(k for t, d, k in plan_groups(hostcheck, sub, prm.schedule, prm.r) if t == 17)
    assert sizes[1] <= 256 < sizes[16] <= 4096 < sizes[len(batch)]          # five waves, one wave, wave pair
    for sub in (batch[:1], batch[:16], batch):
        assert gpu_ctx.deep_fri_verify_batch(prm, sub) == want[:len(sub)]
    assert [gpu_ctx.deep_fri_verify(prm, p) for p in batch] == want
    assert 0 < sum(want) < len(want)


@pytest.mark.parametrize("option", ["poseidon_lane_only", "sponge_one_wave"])
def test_gpu_batch_under_forced_forms(gpu_ctx, oracle, option):
    prm, batch, want = big_batch(gpu_ctx, oracle)
    mixed, mwant = shape_batch(gpu_ctx, oracle, 1 << 12, [128], 8)
    c = Context(0)                                                            # a fresh context: the session's options stay as they are
    try:
        c.set_option(option, 1)
        for sub in (batch[:1], batch[:16], batch):
            assert c.deep_fri_verify_batch(prm, sub) == want[:len(sub)]
        assert c.deep_fri_verify_batch(DeepFriParams([128], 8, SEED_Z), mixed) == mwant
    finally:
        c.close()


def test_gpu_batch_at_bench_size(gpu_ctx):
    """two 2^20-row proofs (r = 32, [16,16,8]) made on the GPU from synthetic f0s, and a tampered copy"""
    import torch
    n0, sched, r = 1 << 20, [16, 16, 8], 32
    sch = np.ascontiguousarray(sched, dtype=np.uint64); proofs = []
    for seed in (0x5EED0014, 0x5EED0015):
        f0 = torch.empty((n0, 4), dtype=torch.int64, device="cuda")
        gpu_ctx._chk(gpu_ctx.lib.stark_synth_column_dev(gpu_ctx.h, seed, 5, 0, n0, C.c_void_p(f0.data_ptr())))
        h = C.c_void_p()
        gpu_ctx._chk(gpu_ctx.lib.stark_deep_fri_prove_dev(gpu_ctx.h, None, None, None, None, C.c_void_p(f0.data_ptr()), n0, sch.ctypes.data_as(C.c_void_p), 3, r, SEED_Z, C.byref(h)))
        proofs.append(gpu_ctx._proof_out(h)[0])
    bad = bytearray(proofs[0]); bad[len(bad) // 2] ^= 0x10
    prm = DeepFriParams(sched, r, SEED_Z)
    batch = [proofs[0], bytes(bad), proofs[1]]
    assert [gpu_ctx.deep_fri_verify(prm, p) for p in batch] == [True, False, True]
    assert gpu_ctx.deep_fri_verify_batch(prm, batch) == [True, False, True]


def test_gpu_batch_empty_and_invalid_arguments(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    p = b"\x01\x02\x03"; buf = (C.c_uint8 * 3).from_buffer_copy(p)
    sch = np.ascontiguousarray([16, 8], dtype=np.uint64); S = sch.ctypes.data_as(C.c_void_p)
    ptrs = (C.c_void_p * 2)(C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p)); lens = (C.c_size_t * 2)(3, 3)
    acc = (C.c_int32 * 2)(7, 7)
    assert lib.stark_deep_fri_verify_batch(h, 0, None, None, None, 2, 8, SEED_Z, None) == 0
    assert lib.stark_deep_fri_verify_batch(h, 2, ptrs, lens, S, 2, 8, SEED_Z, acc) == 0 and list(acc) == [0, 0]     # undecodable: rejected
    assert gpu_ctx.deep_fri_verify_batch(DeepFriParams([16, 8], 8, SEED_Z), []) == []
    assert lib.stark_deep_fri_verify_batch(None, 2, ptrs, lens, S, 2, 8, SEED_Z, acc) == -1
    assert lib.stark_deep_fri_verify_batch(h, 2, ptrs, lens, S, 2, 8, SEED_Z, None) == -1
    acc[0] = acc[1] = 7
    assert lib.stark_deep_fri_verify_batch(h, 2, None, lens, S, 2, 8, SEED_Z, acc) == -1 and list(acc) == [0, 0]
    assert lib.stark_deep_fri_verify_batch(h, 2, ptrs, None, S, 2, 8, SEED_Z, acc) == -1
    assert lib.stark_deep_fri_verify_batch(h, 2, ptrs, lens, None, 2, 8, SEED_Z, acc) == -1
    holes = (C.c_void_p * 2)(C.cast(buf, C.c_void_p), None)
    assert lib.stark_deep_fri_verify_batch(h, 2, holes, lens, S, 2, 8, SEED_Z, acc) == -1
    lens0 = (C.c_size_t * 2)(3, 0); acc[0] = acc[1] = 7
    assert lib.stark_deep_fri_verify_batch(h, 2, holes, lens0, S, 2, 8, SEED_Z, acc) == 0 and list(acc) == [0, 0]   # a null, empty proof: rejected
