"""stark_lagrange_eval_on_h / _dev / _batch_dev on the device: column c at point p must equal the oracle's own lagrange_eval_on_h (R1), the definition (R2)
and, inside H, the column's own bytes (R3) of lagrange_cases.py, byte for byte; the single forms equal the batch's elements; calls queued without a
synchronisation are correct; the pass size and the pool fill change no byte; nothing outside `out` is written and the columns stay intact; bad
arguments are refused before anything is launched.  Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import lagrange_cases as lc
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
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=-1))
    assert not bad[0].size, "%s: first difference at (point, column) = %s" % (what, tuple(int(b[0]) for b in bad))


def run_batch(ctx, dcols, n, zs, omega=None):
    """stark_lagrange_eval_on_h_batch_dev on device columns -> (P, C, 4) host results (out starts as the sentinel)"""
    import torch
    zs = np.ascontiguousarray(zs, np.uint64).reshape(-1, 4)
    out = torch.full((zs.shape[0] * len(dcols), 4), SENTINEL, dtype=torch.int64, device="cuda")
    ctx.sync()
    ctx.lagrange_eval_on_h_batch_dev([t.data_ptr() for t in dcols], n, zs, out.data_ptr(), omega)
    ctx.sync()
    return host(out).reshape(zs.shape[0], len(dcols), 4)


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


@pytest.mark.parametrize("n", lc.N_MATRIX)
def test_shape_matrix(gpu_ctx, oracle, n):
    ref = lc.matrix_reference(oracle, n); dcols = [dev(v) for v in lc.columns(oracle, n)]
    for ncols in lc.NCOLS:
        for npoints in lc.NPOINTS:
            same(run_batch(gpu_ctx, dcols[:ncols], n, lc.points(oracle, n, npoints)), ref[:npoints, :ncols], "n = %d, %d columns, %d points against R2" % (n, ncols, npoints))
    if n >= 2:
        cols = lc.columns(oracle, n, 2); zs = lc.points(oracle, n, 2)
        same(run_batch(gpu_ctx, dcols[:2], n, zs), lc.r1(oracle, cols, zs), "n = %d against R1" % n)
    else:
        same(run_batch(gpu_ctx, dcols[:1], n, lc.points(oracle, n)), np.tile(lc.columns(oracle, n, 1)[0][0], (lc.MAX_POINTS, 1, 1)), "n = 1 gives v[0] for every z")
    for t, w in zip(dcols, lc.columns(oracle, n)):
        same(host(t), w, "a column after the calls")


@pytest.mark.parametrize("n", lc.N_MATRIX)
def test_single_forms_equal_the_batch(gpu_ctx, oracle, n):
    import torch
    cols = lc.columns(oracle, n, 3); zs = lc.points(oracle, n, 2); dcols = [dev(v) for v in cols]
    want = run_batch(gpu_ctx, dcols, n, zs)
    out = torch.full((2 * 3, 4), SENTINEL, dtype=torch.int64, device="cuda")
    gpu_ctx.sync()
    for p in range(2):
        for c in range(3):
            gpu_ctx.lagrange_eval_on_h_dev(dcols[c].data_ptr(), n, zs[p], out.data_ptr() + 32 * (3 * p + c))
    gpu_ctx.sync()
    same(host(out).reshape(2, 3, 4), want, "n = %d: stark_lagrange_eval_on_h_dev" % n)
    got = np.stack([np.stack([gpu_ctx.lagrange_eval_on_h(cols[c], zs[p]) for c in range(3)]) for p in range(2)])
    same(got, want, "n = %d: stark_lagrange_eval_on_h" % n)
    same(want, lc.matrix_reference(oracle, n)[:2, :3], "n = %d against R2" % n)


def test_stream_ordering(gpu_ctx, oracle):
    """two batch calls and a download queued without a synchronisation in between; the host arrays of the first call are overwritten before the second
    is made, so a z or a pointer table read after the call returned would show"""
    import torch
    n = 1 << 12; cols = lc.columns(oracle, n, 3); dcols = [dev(v) for v in cols]; zs = lc.points(oracle, n, 5)
    z1 = np.array(zs[:2]); z2 = np.array(zs[2:])
    o1 = torch.full((2 * 3, 4), SENTINEL, dtype=torch.int64, device="cuda"); o2 = torch.full((3 * 2, 4), SENTINEL, dtype=torch.int64, device="cuda")
    lib, h = gpu_ctx.lib, gpu_ctx.h
    gpu_ctx.sync()
    t1 = table([t.data_ptr() for t in dcols])
    gpu_ctx._chk(lib.stark_lagrange_eval_on_h_batch_dev(h, 3, t1, n, None, 2, hp(z1), vp(o1.data_ptr())))
    z1[:] = 0; t1[0] = t1[1] = t1[2] = 0
    t2 = table([dcols[2].data_ptr(), dcols[0].data_ptr()])
    gpu_ctx._chk(lib.stark_lagrange_eval_on_h_batch_dev(h, 2, t2, n, None, 3, hp(z2), vp(o2.data_ptr())))
    z2[:] = 0; t2[0] = t2[1] = 0
    both = torch.cat([o1, o2]).cpu()                                                   # queued behind both calls on the same stream
    got = both.numpy().view(np.uint64)
    ref = lc.matrix_reference(oracle, n)
    same(got[:6].reshape(2, 3, 4), ref[:2, :3], "the first call")
    same(got[6:].reshape(3, 2, 4), ref[2:, [2, 0]], "the second call")


@pytest.mark.parametrize("n", [1, 2, 8, 1 << 11, 1 << 12, 1 << 14])
def test_points_inside_and_outside_h_in_one_call(gpu_ctx, oracle, n):
    cols = lc.columns(oracle, n, 3); dcols = [dev(v) for v in cols]; ins = lc.inside_points(oracle, n); outs = lc.points(oracle, n, 2)
    zs = np.stack([outs[0]] + [z for z, _ in ins] + [outs[1]])
    got = run_batch(gpu_ctx, dcols, n, zs)
    for q, (_, j) in enumerate(ins):
        same(got[1 + q], np.stack([v[j] for v in cols]), "n = %d, z = omega^%d" % (n, j))
    same(got, lc.r2(oracle, cols, zs), "n = %d, mixed points against R2" % n)
    same(run_batch(gpu_ctx, dcols, n, np.stack([z for z, _ in ins])), got[1:-1], "n = %d, only points inside H" % n)


def test_zero_corners_repeats_and_another_root(gpu_ctx, oracle):
    for n in (2, 64, 1 << 12):
        cols = lc.columns(oracle, n, 3)
        same(run_batch(gpu_ctx, [dev(v) for v in cols], n, np.zeros((1, 4), np.uint64))[0], np.stack([lc.coefficients(oracle, v)[0] for v in cols]), "z = 0 at n = %d" % n)
    for n, npoints in ((256, None), (1 << 12, 11)):
        cols = lc.corner_columns(n, 3); zs = lc.corners()[:npoints]
        same(run_batch(gpu_ctx, [dev(v) for v in cols], n, zs), lc.r2(oracle, cols, zs), "corner values at n = %d" % n)
    n = 1 << 11; a, b = [dev(v) for v in lc.columns(oracle, n, 2)]
    same(run_batch(gpu_ctx, [a, b, a, a], n, lc.points(oracle, n, 2)), lc.matrix_reference(oracle, n)[:2, [0, 1, 0, 0]], "a repeated column pointer")
    for n in (8, 1 << 12):
        v = lc.columns(oracle, n, 1)[0]; w3, u = lc.third_power_domain(oracle, v)
        zs = np.concatenate([lc.points(oracle, n, 2), [oracle.pow(w3, 5)]])
        got = run_batch(gpu_ctx, [dev(v)], n, zs, omega=w3)
        same(got, lc.r2(oracle, [u], zs), "omega^3 as the generator at n = %d" % n)
        same(got[2], v[5:6], "z = (omega^3)^5 at n = %d" % n)


def test_option_lagrange_max_partials(gpu_ctx, oracle):
    """passes of one point, of two points, the default and -1: equal bytes (5 points at n = 2^12, 3 columns, two workgroups per column)"""
    from stark_mlwe_amd.api import StarkError
    n, ncols = 1 << 12, 3
    dcols = [dev(v) for v in lc.columns(oracle, n, ncols)]; zs = lc.points(oracle, n, 5); want = lc.matrix_reference(oracle, n)[:, :ncols]
    mixed = np.stack([zs[0], lc.inside_points(oracle, n)[3][0], zs[1]]); want_mixed = lc.r2(oracle, lc.columns(oracle, n, ncols), mixed)
    for v in (1, 2 * ncols * lc.workgroups(n), -1):
        with options(gpu_ctx, lagrange_max_partials=v):
            same(run_batch(gpu_ctx, dcols, n, zs), want, "lagrange_max_partials = %d" % v)
            same(run_batch(gpu_ctx, dcols, n, mixed), want_mixed, "lagrange_max_partials = %d, mixed points" % v)
    same(run_batch(gpu_ctx, dcols, n, zs), want, "the default")
    for acc in (0, 1):
        with options(gpu_ctx, lagrange_wide_acc=acc):
            same(run_batch(gpu_ctx, dcols, n, zs), want, "lagrange_wide_acc = %d" % acc)
    for bad in (0, -2, (1 << 28) + 1):
        with pytest.raises(StarkError) as e:
            gpu_ctx.set_option("lagrange_max_partials", bad)
        assert "lagrange_max_partials" in str(e.value), str(e.value)
    with pytest.raises(StarkError) as e:
        gpu_ctx.set_option("no_such_option", 1)
    assert "lagrange_max_partials" in str(e.value)


def test_against_the_merge(gpu_ctx, oracle):
    """the product's own merge: lagrange_eval_on_h(Phi, z) on a device-resident Phi = a s + e - t equals c* (z^n - 1) of stark_ali_merge_dev on a, s, e, t"""
    import torch
    n = 1 << 12; a, s, e, t = [oracle.synth_column(0xA11, c, 0, n) for c in range(4)]
    phi = np.stack([oracle.sub(oracle.add(oracle.mul(a[i], s[i]), e[i]), t[i]) for i in range(n)])
    omega = oracle.domain_omega(n); z = lc.points(oracle, n, 1)[0]
    d = [dev(x) for x in (a, s, e, t)]; f0 = torch.zeros((n, 4), dtype=torch.int64, device="cuda"); cs = np.zeros(4, np.uint64)
    gpu_ctx.sync()
    gpu_ctx._chk(gpu_ctx.lib.stark_ali_merge_dev(gpu_ctx.h, *[vp(x.data_ptr()) for x in d], None, None, hp(omega), hp(z), n, vp(f0.data_ptr()), hp(cs)))
    want = oracle.mul(cs, oracle.sub(oracle.pow(z, n), oracle.from_u64(1)))
    got = run_batch(gpu_ctx, [dev(phi)], n, z, omega=omega)
    same(got[0], want.reshape(1, 4), "lagrange_eval_on_h(Phi, z) against c* (z^n - 1)")
    same(got, lc.r2(oracle, [phi], z), "and against R2")


@pytest.mark.parametrize("n", [8, 1 << 12])
def test_between_guard_bands(gpu_ctx, oracle, n):
    """3 columns (one repeated) at 4 points, one of them inside H: out between sentinel rows, the columns one sentinel row apart; nothing outside out is
    written, the columns keep every byte, and the result does not depend on what out held"""
    cols = lc.columns(oracle, n, 2); use = [0, 1, 0]
    zs = np.ascontiguousarray(np.stack([lc.points(oracle, n, 3)[0], lc.inside_points(oracle, n)[2][0], lc.points(oracle, n, 3)[1], lc.points(oracle, n, 3)[2]]))
    want = lc.r2(oracle, [cols[i] for i in use], zs).reshape(-1, 4)
    for prefill in (SENTINEL, 0):
        cb = Band(cols); ob = Band([4 * 3], prefill=prefill)
        gpu_ctx.sync()
        rc = gpu_ctx.lib.stark_lagrange_eval_on_h_batch_dev(gpu_ctx.h, 3, table([cb.ptr(i).value for i in use]), n, None, 4, hp(zs), ob.ptr())
        assert rc == 0, gpu_ctx.lib.stark_last_error(gpu_ctx.h)
        gpu_ctx.sync()
        h = ob.host(); ob.check("out, prefill %#x" % prefill, h)
        same(ob.payload(0, h), want, "n = %d between bands, prefill %#x" % (n, prefill))
        cb.check_unchanged("the columns")
    cb = Band([cols[0]]); ob = Band([1])
    gpu_ctx.sync()
    assert gpu_ctx.lib.stark_lagrange_eval_on_h_dev(gpu_ctx.h, cb.ptr(), n, hp(zs[0]), None, ob.ptr()) == 0
    gpu_ctx.sync()
    h = ob.host(); ob.check("out of the single form", h); cb.check_unchanged("the column of the single form")
    same(ob.payload(0, h), want[:1], "n = %d, the single form between bands" % n)


def test_pool_poison(oracle):
    """results byte-equal to the oracle under pool_poison 0x5A and 0x00, twice each (the second run recycles the blocks of the first): one pass, and
    passes of one point with a point inside H between them"""
    from test_gpu_pool_poison import own_context, under_both_fills
    n, ncols = 1 << 12, 3
    cols = lc.columns(oracle, n, ncols); zs = lc.points(oracle, n, 5)
    mixed = np.stack([zs[0], lc.inside_points(oracle, n)[3][0], zs[1]])
    small = lc.columns(oracle, 8, ncols)

    def case(cols, n, zs):
        return (lambda c: run_batch(c, [dev(v) for v in cols], n, zs)), lc.r2(oracle, cols, zs)
    for max_partials in (-1, 1):
        with own_context(lagrange_max_partials=max_partials) as c:
            under_both_fills(c, [("n = 2^12, 5 points, max_partials %d" % max_partials,) + case(cols, n, zs), ("mixed points, max_partials %d" % max_partials,) + case(cols, n, mixed),
                                 ("n = 8, max_partials %d" % max_partials,) + case(small, 8, lc.points(oracle, 8, 2))])


def test_bad_arguments_are_refused_before_any_launch(gpu_ctx, oracle):
    """every STARK_ERR_INVALID_ARG case of the header comment: out keeps its pre-fill and stark_last_error names the reason; empty calls are STARK_OK"""
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.h
    n = 4
    cols = lc.columns(oracle, n, 2); zs = np.ascontiguousarray(lc.points(oracle, n, 2))
    buf = torch.full((2 * n + 4 + 2, 4), SENTINEL, dtype=torch.int64, device="cuda")   # [column 0 | column 1 | out (2 x 2) | spare (2)], written below
    c0, c1, o = buf.data_ptr(), buf.data_ptr() + 32 * n, buf.data_ptr() + 64 * n
    tt = table([c0, c1]); one = oracle.from_u64(1)
    f = lib.stark_lagrange_eval_on_h_batch_dev; g = lib.stark_lagrange_eval_on_h_dev
    cases = {"null ctx": (lambda: f(None, 2, tt, n, None, 2, hp(zs), vp(o)), None),
             "null table": (lambda: f(h, 2, None, n, None, 2, hp(zs), vp(o)), "null column table"),
             "null entry": (lambda: f(h, 2, table([c0, 0]), n, None, 2, hp(zs), vp(o)), "null column entry 1"),
             "null out": (lambda: f(h, 2, tt, n, None, 2, hp(zs), None), "null out"),
             "null z with points": (lambda: f(h, 2, tt, n, None, 2, None, vp(o)), "null z"),
             "n = 0": (lambda: f(h, 2, tt, 0, None, 2, hp(zs), vp(o)), "power of two"),
             "n = 3": (lambda: f(h, 2, tt, 3, None, 2, hp(zs), vp(o)), "power of two"),
             "n = 2^31": (lambda: f(h, 2, tt, 1 << 31, None, 2, hp(zs), vp(o)), "2^30"),
             "omega = 1 at n = 4": (lambda: f(h, 2, tt, n, hp(one), 2, hp(zs), vp(o)), "primitive"),
             "omega of order 2 n": (lambda: f(h, 2, tt, n, hp(oracle.domain_omega(2 * n)), 2, hp(zs), vp(o)), "omega^n != 1"),
             "out inside column 1": (lambda: f(h, 2, tt, n, None, 2, hp(zs), vp(c1 + 32)), "out overlaps column 1"),
             "the end of out on the first row of column 0": (lambda: f(h, 2, tt, n, None, 2, hp(zs), vp(c0 - 32 * 3)), "out overlaps column 0"),
             "out on the last row of column 1": (lambda: f(h, 2, tt, n, None, 2, hp(zs), vp(o - 32)), "out overlaps column 1"),
             "single: null ctx": (lambda: g(None, vp(c0), n, hp(zs), None, vp(o)), None),
             "single: null column": (lambda: g(h, None, n, hp(zs), None, vp(o)), "null column entry 0"),
             "single: null out": (lambda: g(h, vp(c0), n, hp(zs), None, None), "null out"),
             "single: null z": (lambda: g(h, vp(c0), n, None, None, vp(o)), "null z"),
             "single: n = 3": (lambda: g(h, vp(c0), 3, hp(zs), None, vp(o)), "power of two"),
             "single: out is the column's last row": (lambda: g(h, vp(c0), n, hp(zs), None, vp(c0 + 32 * (n - 1))), "out overlaps column 0"),
             "host form: n = 3": (lambda: lib.stark_lagrange_eval_on_h(h, hp(cols[0]), 3, hp(zs), None, hp(np.zeros(4, np.uint64))), "power of two"),
             "host form: omega = 1 at n = 4": (lambda: lib.stark_lagrange_eval_on_h(h, hp(cols[0]), n, hp(zs), hp(one), hp(np.zeros(4, np.uint64))), "primitive")}
    for what, (fn, reason) in cases.items():
        gpu_ctx.sync()
        assert fn() == ERR_INVALID_ARG, what
        if reason is not None:
            assert reason in lib.stark_last_error(h).decode(), (what, lib.stark_last_error(h))
        gpu_ctx.sync()
        assert (host(buf) == SENTINEL).all(), "%s: something was written" % what
    assert f(h, 0, None, n, None, 2, hp(zs), vp(o)) == 0 and f(h, 2, tt, n, None, 0, None, vp(o)) == 0 and f(h, 0, None, 0, None, 0, None, None) == 0
    gpu_ctx.sync()
    assert (host(buf) == SENTINEL).all()
    buf[:n] = dev(cols[0]); buf[n:2 * n] = dev(cols[1])                                 # the context is usable afterwards; out next to the columns is allowed
    gpu_ctx._chk(f(h, 2, tt, n, None, 2, hp(zs), vp(o))); gpu_ctx.sync()
    same(host(buf)[2 * n:2 * n + 4].reshape(2, 2, 4), lc.matrix_reference(oracle, n)[:2, :2] if n in lc.N_MATRIX else lc.r2(oracle, cols, zs), "after the refused calls")
    assert (host(buf)[2 * n + 4:] == SENTINEL).all()
