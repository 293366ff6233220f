"""The sharded commit and prove as one C-ABI call each (stark_fri_build_sharded_dev, stark_fri_shard_prove_queries, stark_deep_fri_prove_sharded_dev):
W > 1 through the diagnostic twins that run the same phase code for W virtual ranks on one GPU (collectives as device copies), W = 1 through the
real entry points without a communicator.  References: the one-GPU build, the oracle's goldens.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _synth(ctx, seed, n, cols=(0,)):
    import torch
    out = []
    for c in cols:
        x = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        ctx._chk(ctx.lib.stark_synth_column_dev(ctx.h, seed, c, 0, n, C.c_void_p(x.data_ptr())))
        out.append(x)
    return out


def _one_gpu_roots(ctx, f0, n0, sched, seed_z):
    from stark_mlwe_amd.api import _ptr
    sch = np.ascontiguousarray(sched, dtype=np.uint64); st = C.c_void_p()
    ctx._chk(ctx.lib.stark_fri_build_dev(ctx.h, C.c_void_p(f0.data_ptr()), n0, _ptr(sch), len(sched), seed_z, C.byref(st)))
    roots = np.zeros((len(sched) + 1, 4), np.uint64)
    for l in range(len(sched) + 1):
        ctx._chk(ctx.lib.stark_fri_layer_root(st, l, _ptr(roots[l])))
    ctx._chk(ctx.lib.stark_fri_state_free(st))
    return roots


@pytest.mark.parametrize("k", [12, 16, 20])
@pytest.mark.parametrize("sched", [[16, 16, 8], [8, 8, 8]], ids=["16x16x8", "8x8x8"])
def test_emulated_sharded_commit_equals_one_gpu_build(gpu_ctx, k, sched):
    """W in {1, 2, 4, 8} virtual ranks: every rank's L+1 roots equal stark_fri_build_dev's on the whole f0, layer by layer — including plans in
    which the number of sharded layers changes with W ([16,16,8] at 2^12: layer 2 is sharded at W = 1, replicated at W = 8)."""
    from stark_mlwe_amd.api import fri_shard_layout
    n0, seed_z = 1 << k, 0xDEEFBAAD
    (f0,) = _synth(gpu_ctx, 0x5EED + k, n0)
    want = _one_gpu_roots(gpu_ctx, f0, n0, sched, seed_z)
    nsharded = set()
    for W in (1, 2, 4, 8):
        got = gpu_ctx.diag_fri_build_sharded_emulated(W, f0, n0, sched, seed_z)
        for q in range(W):
            assert (got[q] == want).all(), (W, q, [l for l in range(len(sched) + 1) if not (got[q][l] == want[l]).all()])
        nsharded.add(sum(fri_shard_layout(n0, sched, W)[0]))
    if k == 12 and sched == [16, 16, 8]:
        assert fri_shard_layout(n0, sched, 1)[0][2] and not fri_shard_layout(n0, sched, 8)[0][2]
        assert len(nsharded) > 1
    del f0; gpu_ctx.trim()


def test_bench_step_on_eight_virtual_ranks_matches_oracle_golden(gpu_ctx):
    """bench.py's step (2^20 rows, blow-up 8, coset 5, z = 0xC0FFEE, [16,16,8]) on 8 virtual ranks from end to end: the sharded LDE of each column
    (stark_diag_lde_sharded_emulated_dev), the block-local merge of each rank's block (stark_ali_merge_shard_dev), the sharded commit
    (stark_diag_fri_build_sharded_emulated_dev).  Every rank's roots equal tests/golden/step_roots_k20.json, which the CPU oracle wrote."""
    import torch
    import bench
    from stark_mlwe_amd.api import _ptr
    k, W = 20, 8
    seed = 0x5EED0000 + k
    gold = json.load(open(os.path.join(GOLD, f"step_roots_k{k}.json")))
    assert bench.golden_step_roots(k, seed) == gold["roots"]
    N = 1 << (k + bench.LOG_BLOWUP); nl = N // W
    cols = _synth(gpu_ctx, seed, 1 << k, cols=range(4))
    shift, z = bench._mont_small(bench.STEP_COSET), bench._mont_small(bench.STEP_Z)
    ext = []
    for c in cols:
        e = torch.empty((N, 4), dtype=torch.int64, device="cuda")
        gpu_ctx._chk(gpu_ctx.lib.stark_diag_lde_sharded_emulated_dev(gpu_ctx.h, 0, W, C.c_void_p(c.data_ptr()), k, bench.LOG_BLOWUP, _ptr(shift), C.c_void_p(e.data_ptr())))
        ext.append(e)
    del cols
    f0 = torch.empty((N, 4), dtype=torch.int64, device="cuda")
    for q in range(W):
        blk = [C.c_void_p(e[q * nl:(q + 1) * nl].data_ptr()) for e in ext]
        gpu_ctx._chk(gpu_ctx.lib.stark_ali_merge_shard_dev(gpu_ctx.h, *blk, None, None, None, _ptr(z), nl, q * nl, N, C.c_void_p(f0[q * nl:(q + 1) * nl].data_ptr()), None))
    del ext
    roots = gpu_ctx.diag_fri_build_sharded_emulated(W, f0, N, bench.SCHEDULE, bench.SEED_Z)
    for q in range(W):
        assert bench.roots_hex(list(roots[q])) == gold["roots"], q
    del f0; gpu_ctx.trim()


GOLDENS = ["proof_k16_r32.json", "proof_k14_r32_hi32_32_16.json", "proof_k14_r32_hi64_32_8.json", "proof_k15_r32_uni32x3.json", "proof_k15_r32_uni64x2x8.json"]


@pytest.mark.parametrize("name", GOLDENS)
def test_emulated_sharded_prove_matches_oracle_golden(gpu_ctx, name):
    """deep_fri_prove from (a, s, e, t) on W in {2, 4, 8} virtual ranks (build_f0 with the columns gathered to their sponge ranks and the digests
    all-reduced, the sharded commit, the query table filled by owners and all-reduced): every rank's bytes are sha256-equal to the oracle's golden,
    and the verifier accepts them."""
    from stark_mlwe_amd.api import DeepFriParams
    gold = json.load(open(os.path.join(GOLD, name)))
    n0, sched, r, seed_z = 1 << gold["log_n0"], gold["schedule"], gold["r"], gold["seed_z"]
    cols = _synth(gpu_ctx, gold["synth_seed"], n0, cols=range(4))
    params = DeepFriParams(sched, r, seed_z)
    for W in (2, 4, 8):
        proofs = gpu_ctx.diag_deep_fri_prove_sharded_emulated(W, *cols, n0, params)
        assert len(proofs) == W
        for q, (b, est) in enumerate(proofs):
            assert len(b) == gold["proof_len"] and est == gold["size_estimate"], (W, q)
            assert hashlib.sha256(b).hexdigest() == gold["sha256"], (W, q)
        assert gpu_ctx.deep_fri_verify(params, proofs[0][0])
    del cols; gpu_ctx.trim()


def test_real_entry_points_on_one_rank_equal_the_one_gpu_prove(gpu_ctx):
    """Without a communicator (W = 1) the real entry points run the phase code with the collectives reduced to copies: stark_deep_fri_prove_sharded_dev
    returns stark_deep_fri_prove_dev's bytes at 2^16, from (a, s, e, t) and from f0; stark_fri_build_sharded_dev's roots are stark_fri_build_dev's and
    stark_fri_shard_prove_queries gives the same proof."""
    import torch
    from stark_mlwe_amd.api import DeepFriParams, _ptr
    gold = json.load(open(os.path.join(GOLD, "proof_k16_r32.json")))
    n0, sched, r, seed_z = 1 << 16, gold["schedule"], gold["r"], gold["seed_z"]
    cols = _synth(gpu_ctx, gold["synth_seed"], n0, cols=range(4))
    sch = np.ascontiguousarray(sched, dtype=np.uint64); h = C.c_void_p()
    gpu_ctx._chk(gpu_ctx.lib.stark_deep_fri_prove_dev(gpu_ctx.h, *[C.c_void_p(c.data_ptr()) for c in cols], None, n0, _ptr(sch), len(sched), r, seed_z, C.byref(h)))
    want, west = gpu_ctx._proof_out(h)
    assert hashlib.sha256(want).hexdigest() == gold["sha256"]
    params = DeepFriParams(sched, r, seed_z)
    got, est, ms = gpu_ctx.deep_fri_prove_sharded(*cols, n0, params)
    assert got == want and est == west
    assert len(ms) == 3 and all(m >= 0 for m in ms)
    f0 = torch.empty((n0, 4), dtype=torch.int64, device="cuda")
    gpu_ctx._chk(gpu_ctx.lib.stark_build_f0_dev(gpu_ctx.h, *[C.c_void_p(c.data_ptr()) for c in cols], n0, C.c_void_p(f0.data_ptr()), None))
    got_f0, _, _ = gpu_ctx.deep_fri_prove_sharded(None, None, None, None, n0, params, f0=f0)
    assert got_f0 == want
    st = gpu_ctx.fri_build_sharded(f0, n0, sched, seed_z)
    try:
        assert st.num_layers == len(sched) + 1
        assert (st.roots() == _one_gpu_roots(gpu_ctx, f0, n0, sched, seed_z)).all()
        assert all(st.is_sharded(l) for l in range(len(sched)))
        assert st.prove_queries(r)[0] == want
    finally:
        st.free()
    del cols, f0; gpu_ctx.trim()


def test_real_entry_points_refuse_bad_arguments_and_stay_usable(gpu_ctx):
    """Argument errors return STARK_ERR_INVALID_ARG before any collective (a schedule that does not divide n0, r = 0, n0 not a power of two, null
    pointers, a rank count that is not a power of two), and the context proves correctly afterwards."""
    from stark_mlwe_amd.api import DeepFriParams, _ptr
    gold = json.load(open(os.path.join(GOLD, "proof_k16_r32.json")))
    n0, sched, r, seed_z = 1 << 16, gold["schedule"], gold["r"], gold["seed_z"]
    cols = _synth(gpu_ctx, gold["synth_seed"], n0, cols=range(4))
    lib = gpu_ctx.lib
    P = [C.c_void_p(c.data_ptr()) for c in cols]

    def prove(sch_list, n, rr, ptrs=P):
        sch = np.ascontiguousarray(sch_list, dtype=np.uint64); h = C.c_void_p()
        rc = lib.stark_deep_fri_prove_sharded_dev(gpu_ctx.h, *ptrs, None, n, _ptr(sch), len(sch_list), rr, seed_z, C.byref(h))
        if rc == 0:
            lib.stark_proof_free(h)
        return rc
    assert prove([16, 16, 7], n0, r) == -1
    assert prove(sched, n0, 0) == -1
    assert prove(sched, n0 - 16, r) == -1
    assert prove(sched, n0, r, [P[0], None, P[2], P[3]]) == -1
    h = C.c_void_p(); sch = np.ascontiguousarray([16, 16, 7], dtype=np.uint64)
    assert lib.stark_fri_build_sharded_dev(gpu_ctx.h, P[0], n0, _ptr(sch), 3, seed_z, C.byref(h)) == -1
    roots = np.zeros((3, 4, 4), np.uint64)
    assert lib.stark_diag_fri_build_sharded_emulated_dev(gpu_ctx.h, 3, P[0], n0, _ptr(np.ascontiguousarray(sched, dtype=np.uint64)), 3, seed_z, _ptr(roots)) == -1
    got, _, _ = gpu_ctx.deep_fri_prove_sharded(*cols, n0, DeepFriParams(sched, r, seed_z))
    assert hashlib.sha256(got).hexdigest() == gold["sha256"]
    del cols; gpu_ctx.trim()
