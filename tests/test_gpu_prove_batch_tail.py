"""The side-by-side tail of the batched DEEP-FRI provers on the GPU (capi_fri.hip over fri_batch.hpp): stark_fri_commit_batch_dev,
stark_ali_merge_batch_dev, stark_deep_fri_prove_f0_batch_dev and the tail of stark_deep_fri_prove_batch_dev.  Element i of every result must equal
what the single call returns for trace i alone, byte for byte, and the oracle's where the oracle is cheap.  The host build of the commit driver is
tested in tests/test_fri_batch_host.py.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import json
import os
import statistics
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_Z = 0xDEEFBAAD
SHAPES = {6: ([4, 2], 4), 10: ([16, 8], 8), 7: ([128], 4), 8: ([], 4), 12: ([16, 16, 8], 32)}     # k -> (schedule, r); see the host test for what each reaches
vp = C.c_void_p
INVALID_ARG = -1


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def traces(oracle):
    """k -> 70 (k = 6, 10) or 5 f0 vectors on the host and on the device: made once, shared"""
    out = {}
    for k in SHAPES:
        B = 70 if k in (6, 10) else 5
        h = oracle.rand_fr_columns(0xF00 + k, 1 << k, B)
        d = [dev(h[b]) for b in range(B)]
        out[k] = (h, d)
    return out


@pytest.fixture(scope="module")
def single_roots(gpu_ctx, traces):
    """k -> roots of stark_fri_build_dev per trace (the reference of the batch commit), under the default options"""
    out = {}
    for k, (sched, _) in SHAPES.items():
        sch = np.ascontiguousarray(sched, dtype=np.uint64)
        h, d = traces[k]
        rs = np.zeros((len(d), len(sched) + 1, 4), np.uint64)
        for b, f in enumerate(d):
            st = vp()
            gpu_ctx._chk(gpu_ctx.lib.stark_fri_build_dev(gpu_ctx.h, vp(f.data_ptr()), 1 << k, sch.ctypes.data_as(vp), len(sched), SEED_Z, C.byref(st)))
            for l in range(len(sched) + 1):
                gpu_ctx._chk(gpu_ctx.lib.stark_fri_layer_root(st, l, rs[b, l].ctypes.data_as(vp)))
            gpu_ctx.lib.stark_fri_state_free(st)
        out[k] = rs
    return out


def prove_f0_single(ctx, f, n0, sched, r):
    sch = np.ascontiguousarray(sched, dtype=np.uint64); h = vp()
    ctx._chk(ctx.lib.stark_deep_fri_prove_dev(ctx.h, None, None, None, None, vp(f.data_ptr()), n0, sch.ctypes.data_as(vp), len(sched), r, SEED_Z, C.byref(h)))
    return ctx._proof_out(h)[0]


@pytest.mark.parametrize("opt", [None, ("sponge_one_wave", 1), ("poseidon_lane_only", 1)])
@pytest.mark.parametrize("k", sorted(SHAPES))
def test_commit_batch_roots(gpu_ctx, oracle, traces, single_roots, k, opt):
    sched, r = SHAPES[k]
    h, d = traces[k]
    if opt:
        gpu_ctx.set_option(*opt)
    try:
        for B in (1, 5, 70) if k in (6, 10) else (1, 5):
            got = gpu_ctx.fri_commit_batch_dev([f.data_ptr() for f in d[:B]], 1 << k, sched, SEED_Z)
            assert (got == single_roots[k][:B]).all(), (k, B, opt)
    finally:
        if opt:
            gpu_ctx.set_option(opt[0], 0)
    if k <= 10 and opt is None:
        for b in range(5):
            pr = oracle.deep_fri_prove(None, None, None, None, 1 << k, sched, r, SEED_Z, f0=h[b])
            for l in range(len(sched) + 1):
                assert (single_roots[k][b, l] == pr.root(l)).all(), (k, b, l)
            pr.free()


@pytest.mark.parametrize("n", [2, 64, 4096])
def test_ali_merge_batch(gpu_ctx, oracle, n):
    """B = 3: trace 1 blinded (r_opt, beta), traces 0 and 2 not; distinct z per trace.  n = 4096: two workgroups per trace."""
    import torch
    B = 3
    cols = oracle.rand_fr_columns(0xA11 + n, n, 5 * B).reshape(B, 5, n, 4)
    omega = oracle.domain_omega(n)
    zs = np.stack([oracle.from_u64(1000003 + 17 * b) for b in range(B)]); betas = np.stack([oracle.from_u64(77 + b) for b in range(B)])
    dcols = [[dev(cols[b, c]) for c in range(5)] for b in range(B)]
    outs = [torch.zeros((n, 4), dtype=torch.int64, device="cuda") for _ in range(B)]
    r_opts = [None, dcols[1][4].data_ptr(), None]
    cs = gpu_ctx.ali_merge_batch_dev([[x.data_ptr() for x in dcols[b][:4]] for b in range(B)], omega, zs, n, [o.data_ptr() for o in outs], r_opts, betas)
    for b in range(B):
        blind = b == 1
        want_f0, want_cs = oracle.ali_merge(*cols[b, :4], omega, zs[b], r=cols[b, 4] if blind else None, beta=betas[b] if blind else None)
        assert (host(outs[b]) == want_f0).all(), b
        assert (cs[b] == want_cs).all(), b
        one = torch.zeros((n, 4), dtype=torch.int64, device="cuda"); c1 = np.zeros(4, np.uint64)
        gpu_ctx._chk(gpu_ctx.lib.stark_ali_merge_dev(gpu_ctx.h, *[vp(x.data_ptr()) for x in dcols[b][:4]], vp(dcols[b][4].data_ptr()) if blind else None,
                                                     betas[b].ctypes.data_as(vp) if blind else None, omega.ctypes.data_as(vp), zs[b].ctypes.data_as(vp), n, vp(one.data_ptr()), c1.ctypes.data_as(vp)))
        assert (host(one) == host(outs[b])).all() and (c1 == cs[b]).all(), b
    # without c*, and without any blinding table
    outs2 = [torch.zeros((n, 4), dtype=torch.int64, device="cuda") for _ in range(B)]
    assert gpu_ctx.ali_merge_batch_dev([[x.data_ptr() for x in dcols[b][:4]] for b in range(B)], omega, zs, n, [o.data_ptr() for o in outs2], want_c_star=False) is None
    for b in (0, 2):
        assert (host(outs2[b]) == host(outs[b])).all()


@pytest.mark.parametrize("k,B", [(6, 5), (10, 5), (7, 5), (8, 5), (12, 4), (10, 70)])
def test_prove_f0_batch(gpu_ctx, oracle, traces, k, B):
    from stark_mlwe_amd.api import DeepFriParams
    sched, r = SHAPES[k]; n0 = 1 << k
    h, d = traces[k]
    prm = DeepFriParams(sched, r, SEED_Z)
    got = gpu_ctx.deep_fri_prove_f0_batch_dev([f.data_ptr() for f in d[:B]], n0, prm)
    assert len(got) == B
    for b in (range(B) if B <= 8 else (0, 1, B // 2, B - 1)):
        assert got[b][0] == prove_f0_single(gpu_ctx, d[b], n0, sched, r), (k, b)
    assert len({g[0] for g in got}) == B
    if B > 8:
        assert gpu_ctx.deep_fri_verify_batch(prm, [g[0] for g in got]) == [True] * B
    if k == 10:
        for b in range(min(B, 5)):
            ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, r, SEED_Z, f0=h[b])
            assert got[b][0] == ref.bytes() and got[b][1] == ref.size_estimate(); ref.free()


def synth_traces(ctx, k, B):
    import torch
    n0 = 1 << k; keep, tr = [], []
    for p in range(B):
        cols = [torch.empty((n0, 4), dtype=torch.int64, device="cuda") for _ in range(4)]
        for c in range(4):
            ctx._chk(ctx.lib.stark_synth_column_dev(ctx.h, 0x7A110000 + 16 * k + p, c, 0, n0, vp(cols[c].data_ptr())))
        keep.append(cols); tr.append([c.data_ptr() for c in cols])
    torch.cuda.synchronize()
    return keep, tr


def prove_single(ctx, tr, n0, sched, r):
    sch = np.ascontiguousarray(sched, dtype=np.uint64); h = vp()
    ctx._chk(ctx.lib.stark_deep_fri_prove_dev(ctx.h, *[vp(x) for x in tr], None, n0, sch.ctypes.data_as(vp), len(sched), r, SEED_Z, C.byref(h)))
    return ctx._proof_out(h)[0]


@pytest.mark.parametrize("k,B", [(10, 5), (12, 4)])
def test_prove_batch_tail_equals_singles(gpu_ctx, k, B):
    from stark_mlwe_amd.api import DeepFriParams
    sched, r = SHAPES[k]; n0 = 1 << k
    keep, tr = synth_traces(gpu_ctx, k, B)
    prm = DeepFriParams(sched, r, SEED_Z)
    side = [g[0] for g in gpu_ctx.deep_fri_prove_batch_dev(tr, n0, prm)]
    assert side == [prove_single(gpu_ctx, tr[p], n0, sched, r) for p in range(B)]
    if k == 10:                                                   # passes of 2, 2 and 1 traces: the last one takes the single tail
        gpu_ctx.set_option("prove_batch_max_rows", 2 * n0)
        try:
            assert [g[0] for g in gpu_ctx.deep_fri_prove_batch_dev(tr, n0, prm)] == side
        finally:
            gpu_ctx.set_option("prove_batch_max_rows", 1 << 22)


def test_worker_tail_option_is_gone(gpu_ctx, traces):
    """The worker-context tail was removed: its option is an unknown key like any other, and the context stays usable."""
    from stark_mlwe_amd.api import DeepFriParams
    k = 10; sched, r = SHAPES[k]; n0 = 1 << k
    _, d = traces[k]
    assert gpu_ctx.lib.stark_ctx_set_option(gpu_ctx.h, b"prove_batch_workers", 1) == INVALID_ARG
    err = gpu_ctx.lib.stark_last_error(gpu_ctx.h).decode()
    assert err.startswith("unknown option 'prove_batch_workers' (") and "prove_batch_max_rows" in err, err
    got = gpu_ctx.deep_fri_prove_f0_batch_dev([f.data_ptr() for f in d[:3]], n0, DeepFriParams(sched, r, SEED_Z))
    assert [g[0] for g in got] == [prove_f0_single(gpu_ctx, d[b], n0, sched, r) for b in range(3)]


def test_passes_f0(gpu_ctx, traces):
    from stark_mlwe_amd.api import DeepFriParams
    k = 10; sched, r = SHAPES[k]; n0 = 1 << k
    _, d = traces[k]
    prm = DeepFriParams(sched, r, SEED_Z); ptrs = [f.data_ptr() for f in d[:5]]
    want = [g[0] for g in gpu_ctx.deep_fri_prove_f0_batch_dev(ptrs, n0, prm)]
    want_roots = gpu_ctx.fri_commit_batch_dev(ptrs, n0, sched, SEED_Z)
    gpu_ctx.set_option("prove_batch_max_rows", 2 * n0)                # passes of 2, 2 and 1 traces
    try:
        assert [g[0] for g in gpu_ctx.deep_fri_prove_f0_batch_dev(ptrs, n0, prm)] == want
        assert (gpu_ctx.fri_commit_batch_dev(ptrs, n0, sched, SEED_Z) == want_roots).all()
    finally:
        gpu_ctx.set_option("prove_batch_max_rows", 1 << 22)


def test_argument_errors(gpu_ctx, oracle, traces):
    from stark_mlwe_amd.api import DeepFriParams
    lib, ctx = gpu_ctx.lib, gpu_ctx
    k = 10; sched, r = SHAPES[k]; n0 = 1 << k
    _, d = traces[k]
    sch = np.ascontiguousarray(sched, dtype=np.uint64); sp = sch.ctypes.data_as(vp)
    B = 3
    tab = (vp * B)(*[f.data_ptr() for f in d[:B]])
    holed = (vp * B)(d[0].data_ptr(), None, d[2].data_ptr())

    def prove(ctxh, tabv, n, schp, L, batch=B):
        out = (vp * B)(*[vp(0xDEAD)] * B)
        return lib.stark_deep_fri_prove_f0_batch_dev(ctxh, batch, tabv, n, schp, L, r, SEED_Z, out), [out[i] for i in range(B)]
    for args in [(None, tab, n0, sp, 2), (ctx.h, None, n0, sp, 2), (ctx.h, holed, n0, sp, 2), (ctx.h, tab, 1000, sp, 2), (ctx.h, tab, 1, sp, 0), (ctx.h, tab, n0, None, 2),
                 (ctx.h, tab, 64, sp, 2)]:                      # 64 / 16 = 4 is not divisible by 8
        rc, out = prove(*args)
        assert rc == INVALID_ARG and out == [None] * B, args
    assert prove(ctx.h, tab, n0, sp, 2, batch=0)[0] == 0
    roots = np.zeros((B, 3, 4), np.uint64)
    assert lib.stark_fri_commit_batch_dev(ctx.h, 0, None, n0, sp, 2, SEED_Z, None) == 0
    for args in [(None, B, tab, n0, sp, 2), (ctx.h, B, holed, n0, sp, 2), (ctx.h, B, tab, 0, sp, 2), (ctx.h, B, tab, n0, None, 2), (ctx.h, B, tab, 1000, sp, 2)]:
        assert lib.stark_fri_commit_batch_dev(*args, SEED_Z, roots.ctypes.data_as(vp)) == INVALID_ARG, args
    assert lib.stark_fri_commit_batch_dev(ctx.h, B, tab, n0, sp, 2, SEED_Z, None) == INVALID_ARG
    # merge: a z inside H (omega itself), a null entry, r_opt without beta
    n = 64; omega = oracle.domain_omega(n)
    zs = np.stack([oracle.from_u64(5), omega, oracle.from_u64(9)])
    c4 = [(vp * B)(*[d[b].data_ptr() for b in range(B)]) for _ in range(4)]
    outs = (vp * B)(*[d[10 + b].data_ptr() for b in range(B)])
    before = host(d[10]).copy()
    mg = lambda a, z, ro, bt: lib.stark_ali_merge_batch_dev(ctx.h, B, a, c4[1], c4[2], c4[3], ro, bt, omega.ctypes.data_as(vp), z.ctypes.data_as(vp), n, outs, None)
    assert mg(c4[0], zs, None, None) == INVALID_ARG
    good_z = np.stack([oracle.from_u64(5 + b) for b in range(B)])
    assert mg(holed, good_z, None, None) == INVALID_ARG
    assert mg(c4[0], good_z, c4[0], None) == INVALID_ARG
    assert lib.stark_ali_merge_batch_dev(ctx.h, 0, None, None, None, None, None, None, None, None, n, None, None) == 0
    assert (host(d[10]) == before).all()                           # nothing was launched
    # the context stays usable
    got = ctx.deep_fri_prove_f0_batch_dev([f.data_ptr() for f in d[:B]], n0, DeepFriParams(sched, r, SEED_Z))
    assert got[1][0] == prove_f0_single(ctx, d[1], n0, sched, r)


UNSUPPORTED = -5
SHAPE_INPUTS = [(0, []), (64, [16, 8]), (64, [1]), (3, []), (6, [2])]
SHAPE_ENTRIES = ["fri_build_dev", "commit_batch_dev B=1", "commit_batch_dev B=2", "prove_dev f0", "prove_f0_batch_dev B=2", "build_sharded_emulated W=2", "plan_create"]
UNSET = "unknown option 'no_such_option'"                    # what stark_last_error holds when the refused call did not set it
# (n0, schedule) -> per entry of SHAPE_ENTRIES (return code, stable substring of stark_last_error or None where the entry point leaves it unset).
# Every row is what the commit BEFORE the one layer-shape function (fri_plan.hpp: fri_layers) answers, entry point by entry point; the rows are
# literals, not derived from the code under test.  The two plan_create entries marked LOOPED never returned there: FriShape::make built the level lengths of an
# arity-1 tree (a loop that does not terminate) before it checked the arity.  They were not run on the device; with the shape checked first the
# call is refused with make's own message, which is what these two entries now pin.
LOOPED = (INVALID_ARG, "layer with arity 1")
SHAPE_TABLE = {
    (0, ()): [(INVALID_ARG, "empty layer")] * 3 + [(INVALID_ARG, "power of two")] * 2 + [(INVALID_ARG, "sharded FRI: empty layer"), (INVALID_ARG, "empty layer")],
    (64, (16, 8)): [(INVALID_ARG, "schedule not dividing")] * 5 + [(INVALID_ARG, "sharded FRI: schedule not dividing"), (INVALID_ARG, "schedule not dividing")],
    (64, (1,)): [(INVALID_ARG, "schedule not dividing")] * 5 + [(INVALID_ARG, "sharded FRI: schedule not dividing"), (INVALID_ARG, "schedule not dividing")],
    (3, ()): [(UNSUPPORTED, "arity 1 with more than one leaf")] * 3 + [(INVALID_ARG, "power of two")] * 2 + [(INVALID_ARG, "n0 must divide over the ranks"), LOOPED],
    (6, (2,)): [(UNSUPPORTED, "arity 1 with more than one leaf")] * 3 + [(INVALID_ARG, "power of two")] * 2 + [(UNSUPPORTED, "arity 1 with more than one leaf"), LOOPED],
}


def shape_error_results(ctx, f_ptrs, n0, sched, entries=SHAPE_ENTRIES):
    """(return code, stark_last_error or None when the call left it unset) of every entry point of `entries` for one (n0, schedule);
    f_ptrs: two device vectors of at least max(n0, 1) elements."""
    lib = ctx.lib
    sch = np.ascontiguousarray(sched if sched else [0], dtype=np.uint64); sp = sch.ctypes.data_as(vp); L = len(sched)
    f = vp(f_ptrs[0]); tab = (vp * 2)(*f_ptrs[:2]); r = 4
    roots = np.zeros((2, L + 1, 4), np.uint64); rp = roots.ctypes.data_as(vp)

    def build():
        st = vp(); rc = lib.stark_fri_build_dev(ctx.h, f, n0, sp, L, SEED_Z, C.byref(st))
        if rc == 0: lib.stark_fri_state_free(st)
        return rc

    def prove():
        h = vp(); rc = lib.stark_deep_fri_prove_dev(ctx.h, None, None, None, None, f, n0, sp, L, r, SEED_Z, C.byref(h))
        if rc == 0: lib.stark_proof_free(h)
        return rc

    def prove_batch():
        out = (vp * 2)(); rc = lib.stark_deep_fri_prove_f0_batch_dev(ctx.h, 2, tab, n0, sp, L, r, SEED_Z, out)
        if rc == 0: [lib.stark_proof_free(out[i]) for i in range(2)]
        return rc

    def plan():
        h = vp(); rc = lib.stark_fri_plan_create(ctx.h, rp, n0, sp, L, r, C.byref(h))
        if rc == 0: lib.stark_fri_plan_free(h)
        return rc
    calls = {"fri_build_dev": build,
             "commit_batch_dev B=1": lambda: lib.stark_fri_commit_batch_dev(ctx.h, 1, tab, n0, sp, L, SEED_Z, rp),
             "commit_batch_dev B=2": lambda: lib.stark_fri_commit_batch_dev(ctx.h, 2, tab, n0, sp, L, SEED_Z, rp),
             "prove_dev f0": prove, "prove_f0_batch_dev B=2": prove_batch,
             "build_sharded_emulated W=2": lambda: lib.stark_diag_fri_build_sharded_emulated_dev(ctx.h, 2, f, n0, sp, L, SEED_Z, rp),
             "plan_create": plan}
    for name in entries:
        assert lib.stark_ctx_set_option(ctx.h, b"no_such_option", 0) == INVALID_ARG       # a known last error: a call that sets none leaves it
        rc = calls[name]()
        err = lib.stark_last_error(ctx.h).decode()
        yield name, rc, None if err.startswith(UNSET) else err


def test_shape_errors_by_entry_point(gpu_ctx, traces, single_roots):
    """Empty layers, non-dividing schedules and arity-1 layers through every entry point that derives the layer shape: each keeps its own return code
    and message (SHAPE_TABLE), nothing is launched that could fault, and after every refusal a good stark_fri_build_dev returns the roots it did before."""
    _, d = traces[6]
    ptrs = [d[0].data_ptr(), d[1].data_ptr()]
    sch = np.ascontiguousarray(SHAPES[6][0], dtype=np.uint64)

    def good_roots():
        st = vp(); rs = np.zeros((len(sch) + 1, 4), np.uint64)
        gpu_ctx._chk(gpu_ctx.lib.stark_fri_build_dev(gpu_ctx.h, vp(ptrs[0]), 64, sch.ctypes.data_as(vp), len(sch), SEED_Z, C.byref(st)))
        try:
            for l in range(len(sch) + 1):
                gpu_ctx._chk(gpu_ctx.lib.stark_fri_layer_root(st, l, rs[l].ctypes.data_as(vp)))
        finally:
            gpu_ctx.lib.stark_fri_state_free(st)
        return rs
    assert (good_roots() == single_roots[6][0]).all()
    for n0, sched in SHAPE_INPUTS:
        want = SHAPE_TABLE[(n0, tuple(sched))]
        for (name, rc, err), (want_rc, want_err) in zip(shape_error_results(gpu_ctx, ptrs, n0, sched), want):
            print(n0, sched, name, rc, repr(err))
            assert rc == want_rc, (n0, sched, name, rc, err)
            assert (err is None) if want_err is None else (err is not None and want_err in err), (n0, sched, name, rc, err)
            assert (good_roots() == single_roots[6][0]).all(), (n0, sched, name)


def test_f0_batch_is_not_slower_than_single_calls(gpu_ctx, oracle):
    """k = 12, B = 32: the f0 batch against 32 single f0 proves in the same process, warmed, median of five alternations.  Only "not slower" is
    asserted: the single path is the reference; the ratio is reported in prove_f0_batch.json under the directory STARK_TEST_RECORDS names (default: test_records/ in the repository root, ignored by git)."""
    from stark_mlwe_amd.api import DeepFriParams
    k, B = 12, 32; sched, r = SHAPES[k]; n0 = 1 << k
    h = oracle.rand_fr_columns(0xF0B, n0, B)
    d = [dev(h[b]) for b in range(B)]; ptrs = [f.data_ptr() for f in d]
    prm = DeepFriParams(sched, r, SEED_Z)
    batch = lambda: [g[0] for g in gpu_ctx.deep_fri_prove_f0_batch_dev(ptrs, n0, prm)]
    singles = lambda: [prove_f0_single(gpu_ctx, f, n0, sched, r) for f in d]
    assert batch() == singles()                                   # warms both paths
    tb, ts = [], []
    for _ in range(5):
        t0 = time.perf_counter(); batch(); tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); singles(); ts.append(time.perf_counter() - t0)
    rec = {"log_n0": k, "batch": B, "batch_ms": 1e3 * statistics.median(tb), "singles_ms": 1e3 * statistics.median(ts)}
    rec["ratio_singles_over_batch"] = rec["singles_ms"] / rec["batch_ms"]
    out = os.environ.get("STARK_TEST_RECORDS") or os.path.join(ROOT, "test_records"); os.makedirs(out, exist_ok=True)
    json.dump(rec, open(os.path.join(out, "prove_f0_batch.json"), "w"), indent=1)
    print(rec)
    assert rec["batch_ms"] <= rec["singles_ms"], rec
