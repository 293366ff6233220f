"""stark_mle_evaluate_dev / stark_mle_evaluate_batch_dev on the device: table i at point i must equal the oracle's Mle::evaluate and the host-pointer
stark_mle_evaluate byte for byte, at every pass count (context option "mle_log_tile") and in both lane ownerships, for one table and for many; the
batch equals single calls; nothing outside `out` is written and the tables stay intact; bad arguments are refused before anything is launched.
Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import mle_cases as mc
from test_gpu_guard_bands import SENTINEL, Band, hp

pytestmark = pytest.mark.gpu
vp = C.c_void_p
ERR_INVALID_ARG = -1


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def table(ptrs):
    return (vp * max(len(ptrs), 1))(*[int(p) for p in ptrs])


def same(got, want, what):
    assert got.shape == want.shape and (got == want).all(), "%s: first difference at instance %d" % (what, int(np.nonzero((got != want).any(axis=-1))[0][0]))


def run_batch(ctx, dtabs, k, pts):
    """stark_mle_evaluate_batch_dev on device tables -> (B, 4) host results (out starts as the sentinel)"""
    import torch
    out = torch.full((len(dtabs), 4), SENTINEL, dtype=torch.int64, device="cuda")
    ctx.sync()
    ctx.mle_evaluate_batch_dev([t.data_ptr() for t in dtabs], k, pts, out.data_ptr())
    ctx.sync()
    return host(out)


def run_singles(ctx, dtabs, k, pts):
    import torch
    out = torch.full((len(dtabs), 4), SENTINEL, dtype=torch.int64, device="cuda")
    ctx.sync()
    for b, t in enumerate(dtabs):
        ctx.mle_evaluate_dev(t.data_ptr(), k, pts[b], out.data_ptr() + 32 * b)
    ctx.sync()
    return host(out)


class options:
    """context options for the length of a `with`, restored to their defaults afterwards"""

    def __init__(self, ctx, **kw): self.ctx, self.kw = ctx, kw

    def __enter__(self):
        try:
            for k, v in self.kw.items(): self.ctx.set_option(k, v)
        except Exception:
            self.__exit__(); raise

    def __exit__(self, *a):
        for k in self.kw: self.ctx.set_option(k, -1)


@pytest.mark.parametrize("log_tile", [3, -1])
def test_k_matrix_against_the_oracle_and_the_host_form(gpu_ctx, oracle, log_tile):
    with options(gpu_ctx, mle_log_tile=log_tile):
        for k in mc.K_MATRIX:
            tabs, pts = mc.tables_and_points(oracle, k, 3)
            got = run_batch(gpu_ctx, [dev(t) for t in tabs], k, pts)
            same(got, mc.reference(oracle, tabs, k, pts), "k = %d against the oracle" % k)
            if k:
                same(got, np.stack([gpu_ctx.mle_evaluate(t, pts[b]) for b, t in enumerate(tabs)]), "k = %d against stark_mle_evaluate" % k)


def test_default_tile_around_its_own_size(gpu_ctx, oracle, hostcheck):
    T = mc.default_log_tile(hostcheck)
    for k in (T - 1, T, T + 1):
        tabs, pts = mc.tables_and_points(oracle, k, 3)
        got = run_batch(gpu_ctx, [dev(t) for t in tabs], k, pts)
        same(got, mc.reference(oracle, tabs, k, pts), "k = %d against the oracle" % k)
        same(got, np.stack([gpu_ctx.mle_evaluate(t, pts[b]) for b, t in enumerate(tabs)]), "k = %d against stark_mle_evaluate" % k)


def test_every_tile_and_both_lane_ownerships(gpu_ctx, oracle):
    """k = 13, B = 2: every instantiation of the pass kernel (no, one .. four lane-local rounds, interleaved and contiguous), a full pass and a rest"""
    k = 13; tabs, pts = mc.tables_and_points(oracle, k, 2); want = mc.reference(oracle, tabs, k, pts)
    dt = [dev(t) for t in tabs]
    for T in mc.LOG_TILES:
        for contig in (0, 1):
            with options(gpu_ctx, mle_log_tile=T, mle_lane_contiguous=contig):
                same(run_batch(gpu_ctx, dt, k, pts), want, "tile %d, contig = %d" % (T, contig))
    for t, w in zip(dt, tabs):
        same(host(t), w, "a table after the calls")


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("k,log_tile", [(7, 3), (13, -1)])
def test_batch_equals_single_calls(gpu_ctx, oracle, B, k, log_tile):
    tabs, pts = mc.tables_and_points(oracle, k, B, seed=0xB47C)
    dt = [dev(t) for t in tabs]
    with options(gpu_ctx, mle_log_tile=log_tile):
        got = run_batch(gpu_ctx, dt, k, pts)
        same(got, run_singles(gpu_ctx, dt, k, pts), "B = %d, k = %d: batch against singles" % (B, k))
    same(got[:3], mc.reference(oracle, tabs[:3], k, pts[:3]), "B = %d, k = %d: against the oracle" % (B, k))


def test_more_instances_than_a_grid_dimension(gpu_ctx, oracle):
    """B = 70 000 at k = 1 over four tables: the launches are cut at 65 535 instances.  Instance b takes table b mod 4 and point b mod 7 (65 535 is 3 mod 4
    and 1 mod 7, so an instance offset lost at the cut changes both); the 28 distinct results come from the oracle."""
    B, k = 70000, 1
    tabs, _ = mc.tables_and_points(oracle, k, 4, seed=0x70C)
    pts7 = mc.tables_and_points(oracle, k, 7, seed=0x70D)[1]
    want28 = np.stack([[oracle.mle_evaluate(tabs[t], pts7[p]) for p in range(7)] for t in range(4)])
    b = np.arange(B)
    dt = [dev(t) for t in tabs]
    got = run_batch(gpu_ctx, [dt[i % 4] for i in range(B)], k, pts7[b % 7])
    same(got, want28[b % 4, b % 7], "70 000 instances")


@pytest.mark.parametrize("log_tile", [3, -1])
def test_definition_and_stored_limb_corners(gpu_ctx, oracle, log_tile):
    with options(gpu_ctx, mle_log_tile=log_tile):
        k = 4; tab = mc.tables_and_points(oracle, k, 1)[0][0]; d = dev(tab)
        same(run_batch(gpu_ctx, [d] * (1 << k), k, mc.boolean_points(oracle, k)), tab, "every Boolean point at k = 4")
        for k in (1, 7, 10, 13):
            tab = mc.tables_and_points(oracle, k, 1)[0][0]; d = dev(tab)
            pts = np.stack([np.zeros((k, 4), np.uint64), np.tile(oracle.from_u64(1), (k, 1))])
            same(run_batch(gpu_ctx, [d, d], k, pts), np.stack([tab[0], tab[-1]]), "all zero / all one at k = %d" % k)
        for k in (1, 6, 10):
            tabs, pts = mc.corner_case(k, 3)
            same(run_batch(gpu_ctx, [dev(t) for t in tabs], k, pts), mc.reference(oracle, tabs, k, pts), "corner values, k = %d" % k)


@pytest.mark.parametrize("k,log_tile", [(7, 3), (0, -1), (13, -1)])
def test_between_guard_bands(gpu_ctx, oracle, k, log_tile):
    """B = 3 with a repeated table: out between sentinel rows, the tables one sentinel row apart; nothing outside out is written, the tables keep every
    byte, and the result does not depend on what out held"""
    tabs = mc.tables_and_points(oracle, k, 2, seed=0x6B4D)[0]; pts3 = mc.tables_and_points(oracle, k, 3, seed=0x6B4E)[1]
    use = [0, 1, 0]; want = mc.reference(oracle, [tabs[i] for i in use], k, pts3)
    with options(gpu_ctx, mle_log_tile=log_tile):
        for prefill in (SENTINEL, 0):
            tb = Band(tabs); ob = Band([3], prefill=prefill)
            gpu_ctx.sync()
            rc = gpu_ctx.lib.stark_mle_evaluate_batch_dev(gpu_ctx.h, 3, table([tb.ptr(i).value for i in use]), k, hp(np.ascontiguousarray(pts3)) if k else None, ob.ptr())
            assert rc == 0, gpu_ctx.lib.stark_last_error(gpu_ctx.h)
            gpu_ctx.sync()
            h = ob.host(); ob.check("out, prefill %#x" % prefill, h)
            same(ob.payload(0, h), want, "k = %d between bands, prefill %#x" % (k, prefill))
            tb.check_unchanged("the tables")
        tb = Band([tabs[0]]); ob = Band([1])
        gpu_ctx.sync()
        assert gpu_ctx.lib.stark_mle_evaluate_dev(gpu_ctx.h, tb.ptr(), k, hp(np.ascontiguousarray(pts3[0])) if k else None, ob.ptr()) == 0
        gpu_ctx.sync()
        h = ob.host(); ob.check("out of the single form", h); tb.check_unchanged("the table of the single form")
        same(ob.payload(0, h), want[:1], "k = %d, the single form between bands" % k)


def test_bad_arguments_are_refused_before_any_launch(gpu_ctx, oracle):
    """every STARK_ERR_INVALID_ARG case of the header comment: out keeps its pre-fill and stark_last_error names the reason; batch == 0 is STARK_OK"""
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.h
    k = 4; n = 1 << k
    tabs, pts = mc.tables_and_points(oracle, k, 2)
    buf = torch.full((2 * n + 4, 4), SENTINEL, dtype=torch.int64, device="cuda")       # [table 0 | table 1 | out (2) | spare (2)], written below
    t0, t1, o = buf.data_ptr(), buf.data_ptr() + 32 * n, buf.data_ptr() + 64 * n
    r = np.ascontiguousarray(pts.reshape(-1, 4)); tt = table([t0, t1])
    cases = {"null ctx": (lambda: lib.stark_mle_evaluate_batch_dev(None, 2, tt, k, hp(r), vp(o)), None),
             "null table array": (lambda: lib.stark_mle_evaluate_batch_dev(h, 2, None, k, hp(r), vp(o)), "null table array"),
             "null entry": (lambda: lib.stark_mle_evaluate_batch_dev(h, 2, table([t0, 0]), k, hp(r), vp(o)), "null table entry 1"),
             "null out": (lambda: lib.stark_mle_evaluate_batch_dev(h, 2, tt, k, hp(r), None), "null out"),
             "null r with k > 0": (lambda: lib.stark_mle_evaluate_batch_dev(h, 2, tt, k, None, vp(o)), "null r"),
             "k = 41": (lambda: lib.stark_mle_evaluate_batch_dev(h, 2, tt, 41, hp(r), vp(o)), "k too large"),
             "out inside table 1": (lambda: lib.stark_mle_evaluate_batch_dev(h, 2, tt, k, hp(r), vp(t1 + 32 * 3)), "out overlaps table 1"),
             "the end of out on the first row of table 0": (lambda: lib.stark_mle_evaluate_batch_dev(h, 2, tt, k, hp(r), vp(t0 - 32)), "out overlaps table 0"),
             "out on the last row of table 1": (lambda: lib.stark_mle_evaluate_batch_dev(h, 2, tt, k, hp(r), vp(o - 32)), "out overlaps table 1"),
             "single: null ctx": (lambda: lib.stark_mle_evaluate_dev(None, vp(t0), k, hp(r), vp(o)), None),
             "single: null table": (lambda: lib.stark_mle_evaluate_dev(h, None, k, hp(r), vp(o)), "null table entry 0"),
             "single: null out": (lambda: lib.stark_mle_evaluate_dev(h, vp(t0), k, hp(r), None), "null out"),
             "single: null r with k > 0": (lambda: lib.stark_mle_evaluate_dev(h, vp(t0), k, None, vp(o)), "null r"),
             "single: k = 41": (lambda: lib.stark_mle_evaluate_dev(h, vp(t0), 41, hp(r), vp(o)), "k too large"),
             "single: out is the table's last row": (lambda: lib.stark_mle_evaluate_dev(h, vp(t0), k, hp(r), vp(t0 + 32 * (n - 1))), "out overlaps table 0")}
    for what, (fn, reason) in cases.items():
        gpu_ctx.sync()
        assert fn() == ERR_INVALID_ARG, what
        if reason is not None:
            assert reason in lib.stark_last_error(h).decode(), (what, lib.stark_last_error(h))
        gpu_ctx.sync()
        assert (host(buf) == SENTINEL).all(), "%s: something was written" % what
    assert lib.stark_mle_evaluate_batch_dev(h, 0, None, k, None, None) == 0
    gpu_ctx.sync()
    assert (host(buf) == SENTINEL).all()
    buf[:n] = dev(tabs[0]); buf[n:2 * n] = dev(tabs[1])                                 # the context is usable afterwards; out next to the tables is allowed
    gpu_ctx._chk(lib.stark_mle_evaluate_batch_dev(h, 2, tt, k, hp(r), vp(o))); gpu_ctx.sync()
    same(host(buf)[2 * n:2 * n + 2], mc.reference(oracle, tabs, k, pts), "after the refused calls")
    assert (host(buf)[2 * n + 2:] == SENTINEL).all()


def test_option_range_and_known_keys(gpu_ctx):
    from stark_mlwe_amd.api import StarkError
    for key, bad in (("mle_log_tile", (2, 13, -2, 0)), ("mle_lane_contiguous", (2, -2)), ("pool_poison", (-2, 256))):
        for v in bad:
            with pytest.raises(StarkError) as e:
                gpu_ctx.set_option(key, v)
            assert key in str(e.value), str(e.value)
    for v in (3, 12, -1):
        gpu_ctx.set_option("mle_log_tile", v)
    with pytest.raises(StarkError) as e:
        gpu_ctx.set_option("no_such_option", 1)
    assert "mle_log_tile" in str(e.value) and "mle_lane_contiguous" in str(e.value) and "pool_poison" in str(e.value)
