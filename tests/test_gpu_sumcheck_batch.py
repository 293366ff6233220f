"""Batched sum-check proving on the GPU: stark_sumcheck_prove_plain_batch_dev / stark_sumcheck_prove_mf_batch_dev (stark_mlwe_amd/csrc/
sumcheck_batch.hpp over the device executor of capi_sumcheck.hip).  Every proof of a batch must be byte-identical to the single-proof entry
point on that witness alone, hence to the oracle's restatement of crates/channel/src/lib.rs, and accepted by the verifiers.  Tree labels are
mixed within each batch; one batch has more instances than the chip has CUs; a second context runs the one-wave transcript form.
Needs an MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LABELS = [2025, 7, 5050, 2025, 11]


def upload(ws):
    import torch
    ts = [torch.from_numpy(np.ascontiguousarray(w, dtype=np.uint64).view(np.int64)).to("cuda") for w in ws]
    torch.cuda.synchronize()
    return ts


def single(ctx, mf, k, label, q, t):
    h = C.c_void_p()
    if mf:
        ctx._chk(ctx.lib.stark_sumcheck_prove_mf_dev(ctx.h, C.c_void_p(t.data_ptr()), k, label, q, C.byref(h)))
    else:
        ctx._chk(ctx.lib.stark_sumcheck_prove_plain_dev(ctx.h, C.c_void_p(t.data_ptr()), k, label, C.byref(h)))
    return ctx._proof_out(h)[0]


def check_batch(ctx, oracle, mf, k, B, q, seed):
    ws = oracle.rand_fr_columns(seed, 1 << k, B)
    labels = [LABELS[b % len(LABELS)] for b in range(B)]
    ts = upload(ws)
    ptrs = [t.data_ptr() for t in ts]
    got = ctx.prove_mf_batch_dev(k, labels, q, ptrs) if mf else ctx.prove_plain_batch_dev(k, labels, ptrs)
    assert len(got) == B
    for b in range(B):
        assert got[b] == single(ctx, mf, k, labels[b], q, ts[b]), b
    for b in sorted({0, B // 2, B - 1}):
        assert got[b] == oracle.sumcheck_prove(mf, k, labels[b], ws[b], q=q if mf else 2), b
        ok = ctx.verify_mf(k, labels[b], q, got[b]) if mf else ctx.verify_plain(k, labels[b], got[b])
        assert ok == (oracle.sumcheck_verify(mf, k, labels[b], got[b], q=q if mf else 2) == 1)
        assert ok is True or (k == 0 and not mf)                                   # verify_plain rejects a proof without rounds (:1100-1102)
    if k > 0 and B > 1:
        assert len(set(got)) == B
    return got


def test_k0_single_path_matches_oracle(gpu_ctx, oracle):
    """k = 0 (claim = witness[0], no rounds): no earlier test covers it; the single path is checked against the oracle first."""
    w = oracle.rand_fr_columns(3, 1, 1)[0]
    assert gpu_ctx.prove_plain(0, 9, w) == oracle.sumcheck_prove(0, 0, 9, w)
    assert gpu_ctx.prove_mf(0, 9, 2, w) == oracle.sumcheck_prove(1, 0, 9, w, q=2)


@pytest.mark.parametrize("k,B", [(0, 2), (1, 5), (5, 64), (12, 5), (14, 2), (3, 300)])
def test_plain_batch(gpu_ctx, oracle, k, B):
    check_batch(gpu_ctx, oracle, 0, k, B, 0, 1000 + 17 * k + B)


@pytest.mark.parametrize("k,B,q", [(0, 2, 2), (1, 5, 1), (5, 64, 2), (12, 5, 2), (14, 2, 2), (3, 5, 8), (2, 300, 2)])
def test_mf_batch(gpu_ctx, oracle, k, B, q):
    """(3, 5, 8) and (2, 300, 2): q >= half, so duplicate query draws are redrawn for a subset of the instances and the fill-in rule runs."""
    check_batch(gpu_ctx, oracle, 1, k, B, q, 2000 + 17 * k + B + q)


def test_one_wave_transcript_form(oracle):
    """The same equalities with the option sponge_one_wave: the batched transcript runs its one-wave kernel instead of the five-wave one."""
    from stark_mlwe_amd.api import Context
    ctx = Context(0)
    try:
        ctx.set_option("sponge_one_wave", 1)
        check_batch(ctx, oracle, 0, 5, 5, 0, 31)
        check_batch(ctx, oracle, 1, 5, 5, 2, 32)
        check_batch(ctx, oracle, 1, 3, 3, 8, 33)
    finally:
        ctx.close()


def test_batch_argument_errors(gpu_ctx, oracle):
    from stark_mlwe_amd.api import StarkError
    ts = upload(oracle.rand_fr_columns(4, 8, 2))
    p = [t.data_ptr() for t in ts]
    with pytest.raises(StarkError):
        gpu_ctx.prove_plain_batch_dev(3, [1, 2, 3], [p[0], None, p[1]])
    with pytest.raises(StarkError):
        gpu_ctx.prove_mf_batch_dev(3, [1, 2], 2, [p[0], None])
    with pytest.raises(StarkError):
        gpu_ctx.prove_plain_batch_dev(41, [1, 2], p)
    with pytest.raises(StarkError):
        gpu_ctx.prove_mf_batch_dev(41, [1, 2], 2, p)
    lib = gpu_ctx.lib
    assert lib.stark_sumcheck_prove_plain_batch_dev(gpu_ctx.h, 0, None, 3, None, None) == 0
    assert lib.stark_sumcheck_prove_mf_batch_dev(gpu_ctx.h, 0, None, 3, None, 2, None) == 0
    out = (C.c_void_p * 2)(1, 1)
    w = (C.c_void_p * 2)(p[0], None); lab = np.array([1, 2], np.uint64)
    assert lib.stark_sumcheck_prove_plain_batch_dev(gpu_ctx.h, 2, w, 3, lab.ctypes.data_as(C.c_void_p), out) != 0
    assert out[0] is None and out[1] is None                                       # on any error every out[i] is null
    assert gpu_ctx.prove_plain_batch_dev(3, [], []) == [] and gpu_ctx.prove_mf_batch_dev(3, [], 2, []) == []
