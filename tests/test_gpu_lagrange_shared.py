"""The options "lagrange_shared_inverse" and "lagrange_share_cosets" on the device (k_lagrange_totals, k_lagrange_invert and the shared / coset forms of
k_lagrange_partials, csrc/lagrange_dev.hpp): under (0, 1), (1, 0) and (1, 1) every Lagrange entry point that reaches the driver gives the bytes of
options (0, 0) and of the definition (R2 of lagrange_cases.py); nothing outside `out` is written, the columns stay intact, stale pool blocks and a busy
stream change nothing, a refused allocation is STARK_ERR_OOM and leaves the context usable.  Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import lagrange_cases as lc
import lagrange_shard_cases as sc
import test_lagrange_shared_host as sh
from test_gpu_guard_bands import SENTINEL, Band, hp
from test_gpu_lagrange_eval import dev, host, options, run_batch, same, table
from test_gpu_lagrange_shard import run_emulated, run_partitioned

pytestmark = pytest.mark.gpu
vp = C.c_void_p
OOM, ERR_INVALID_ARG = -4, -1
_cache = {}


def opts(ctx, opt, **kw):
    return options(ctx, lagrange_shared_inverse=opt[0], lagrange_share_cosets=opt[1], **kw)


def run_single_dev(ctx, dcols, n, zs):
    """stark_lagrange_eval_on_h_dev per (point, column), queued without a synchronisation in between -> (P, C, 4)"""
    import torch
    out = torch.full((len(zs) * len(dcols), 4), SENTINEL, dtype=torch.int64, device="cuda")
    ctx.sync()
    for p in range(len(zs)):
        for c in range(len(dcols)):
            ctx.lagrange_eval_on_h_dev(dcols[c].data_ptr(), n, zs[p], out.data_ptr() + 32 * (len(dcols) * p + c))
    ctx.sync()
    return host(out).reshape(len(zs), len(dcols), 4)


def run_host_form(ctx, cols, zs):
    return np.stack([np.stack([ctx.lagrange_eval_on_h(v, z) for v in cols]) for z in zs])


def coset_reference(oracle, n, ncols=4):
    key = ("cosets", n)
    if key not in _cache:
        zs, _ = sh.coset_points(oracle, n)
        _cache[key] = (zs, lc.r2(oracle, lc.columns(oracle, n, 4), zs))
    zs, ref = _cache[key]
    return zs, ref[:, :ncols]


@pytest.mark.parametrize("n", sh.N_MATRIX)
def test_shape_matrix(gpu_ctx, oracle, n):
    ref = lc.matrix_reference(oracle, n); cols = lc.columns(oracle, n); dcols = [dev(v) for v in cols]
    base = {(c, p): run_batch(gpu_ctx, dcols[:c], n, lc.points(oracle, n, p)) for c in sh.NCOLS for p in sh.NPOINTS}
    for opt in sh.SETTINGS:
        with opts(gpu_ctx, opt):
            for ncols in sh.NCOLS:
                for npoints in sh.NPOINTS:
                    got = run_batch(gpu_ctx, dcols[:ncols], n, lc.points(oracle, n, npoints)); what = "n = %d, %d columns, %d points under %s" % (n, ncols, npoints, opt)
                    same(got, ref[:npoints, :ncols], what + " against R2"); same(got, base[(ncols, npoints)], what + " against (0, 0)")
            zs = lc.points(oracle, n, 2)
            same(run_single_dev(gpu_ctx, dcols[:2], n, zs), ref[:2, :2], "n = %d: stark_lagrange_eval_on_h_dev under %s" % (n, opt))
            same(run_host_form(gpu_ctx, cols[:2], zs), ref[:2, :2], "n = %d: stark_lagrange_eval_on_h under %s" % (n, opt))
    for t, w in zip(dcols, cols):
        same(host(t), w, "a column after the calls")


@pytest.mark.parametrize("n", [1 << 12, 1 << 14])
def test_coset_classes(gpu_ctx, oracle, n):
    """z, z w, z w^(n-1), z w^s in the second workgroup's tile, z again, z2 and z2 w^(n/2), interleaved: one pass, and passes of three points that cut both
    classes with 9 columns in 3 forced groups"""
    zs, ref = coset_reference(oracle, n); cols = lc.columns(oracle, n, 4); dcols = [dev(v) for v in cols]
    base = run_batch(gpu_ctx, dcols, n, zs)
    same(base, ref, "n = %d, the coset points under (0, 0) against R2" % n)
    d9 = [dev(v) for v in lc.columns(oracle, n)]
    with options(gpu_ctx, lagrange_max_partials=3 * 9 * lc.workgroups(n), lagrange_col_groups=3):
        base9 = run_batch(gpu_ctx, d9, n, zs)
    same(base9[:, :4], ref, "n = %d, 9 columns in passes of three under (0, 0) against R2" % n)
    for opt in sh.SETTINGS:
        with opts(gpu_ctx, opt):
            same(run_batch(gpu_ctx, dcols, n, zs), base, "n = %d, the coset points under %s" % (n, opt))
            same(run_single_dev(gpu_ctx, dcols[:1], n, zs), base[:, :1], "n = %d, the coset points one by one under %s" % (n, opt))
            same(run_host_form(gpu_ctx, cols[:1], zs[:3]), base[:3, :1], "n = %d, the host form under %s" % (n, opt))
        with opts(gpu_ctx, opt, lagrange_max_partials=3 * 9 * lc.workgroups(n), lagrange_col_groups=3):
            same(run_batch(gpu_ctx, d9, n, zs), base9, "n = %d, passes of three points, 3 column groups under %s" % (n, opt))
        with opts(gpu_ctx, opt, lagrange_max_partials=1, lagrange_wide_acc=0):
            same(run_batch(gpu_ctx, dcols, n, zs), base, "n = %d, passes of one point, plain accumulator under %s" % (n, opt))


def test_many_totals_per_lane(gpu_ctx, oracle):
    """n = 2^20, one column, two points: 512 totals per point for the 256 lanes of k_lagrange_invert; and (z, z w) as the two points"""
    n = 1 << 20; v = oracle.synth_column(lc.SEED + n, 0, 0, n); z = oracle.synth_column(lc.SEED + 0x100 + n, 0, 0, 2)
    pair = np.ascontiguousarray(np.stack([z[0], oracle.mul(z[0], lc.omega_of(oracle, n))]))
    d = [dev(v)]; want = lc.r2(oracle, [v], np.concatenate([z, pair[1:]]))
    base = run_batch(gpu_ctx, d, n, z); base_pair = run_batch(gpu_ctx, d, n, pair)
    same(base, want[:2], "n = 2^20 under (0, 0) against R2"); same(base_pair, want[[0, 2]], "n = 2^20, (z, z w) under (0, 0) against R2")
    for opt in sh.SETTINGS:
        with opts(gpu_ctx, opt):
            same(run_batch(gpu_ctx, d, n, z), base, "n = 2^20 under %s" % (opt,))
            same(run_batch(gpu_ctx, d, n, pair), base_pair, "n = 2^20, (z, z w) under %s" % (opt,))
    same(host(d[0]), v, "the column after the calls")


def test_shard_and_emulated_paths(gpu_ctx, oracle):
    """the block form ignores the cosets and takes the shared inverse: two uneven blocks plus the combine, and four virtual ranks, at n = 2^12 under (1, 1)"""
    n = 1 << 12; zs, ref = coset_reference(oracle, n); inside = lc.inside_points(oracle, n)[3][0]
    zs = np.ascontiguousarray(np.concatenate([zs[:3], [inside], zs[3:]])); cols = lc.columns(oracle, n, 4); dcols = [dev(v) for v in cols]
    want = lc.r2(oracle, cols, zs); blocks = [(0, n // 4), (n // 4, n - n // 4)]
    got0, shares0 = run_partitioned(gpu_ctx, dcols, n, blocks, zs); emu0 = run_emulated(gpu_ctx, 4, dcols, n, zs)
    same(got0, want, "two blocks under (0, 0) against R2")
    for opt in sh.SETTINGS:
        with opts(gpu_ctx, opt):
            got, shares = run_partitioned(gpu_ctx, dcols, n, blocks, zs); emu = run_emulated(gpu_ctx, 4, dcols, n, zs)
            same(got, want, "two blocks under %s against R2" % (opt,)); same(shares, shares0, "the shares under %s" % (opt,))
            same(emu, emu0, "four virtual ranks under %s" % (opt,))
            for q in range(4):
                same(emu[q], want, "virtual rank %d under %s against R2" % (q, opt))
            same(run_batch(gpu_ctx, dcols, n, zs), want, "the batch call under %s against R2" % (opt,))


@pytest.mark.parametrize("n", [8, 1 << 12])
def test_between_guard_bands(gpu_ctx, oracle, n):
    """3 columns (one repeated) at z, a point inside H, z w and z2: out between sentinel rows, every column between sentinel rows; nothing outside out is
    written, the columns keep every byte, and the result does not depend on what out held"""
    cols = lc.columns(oracle, n, 2); use = [0, 1, 0]; z, z2 = lc.points(oracle, n, 2)
    zs = np.ascontiguousarray(np.stack([z, lc.inside_points(oracle, n)[2][0], oracle.mul(z, lc.omega_of(oracle, n)), z2]))
    want = lc.r2(oracle, [cols[i] for i in use], zs).reshape(-1, 4)
    for opt in sh.SETTINGS:
        with opts(gpu_ctx, opt):
            for prefill in (SENTINEL, 0):
                cb = Band(cols); ob = Band([4 * 3], prefill=prefill)
                gpu_ctx.sync()
                rc = gpu_ctx.lib.stark_lagrange_eval_on_h_batch_dev(gpu_ctx.h, 3, table([cb.ptr(i).value for i in use]), n, None, 4, hp(zs), ob.ptr())
                assert rc == 0, gpu_ctx.lib.stark_last_error(gpu_ctx.h)
                gpu_ctx.sync()
                h = ob.host(); ob.check("out under %s, prefill %#x" % (opt, prefill), h)
                same(ob.payload(0, h), want, "n = %d between bands under %s, prefill %#x" % (n, opt, prefill))
                cb.check_unchanged("the columns")


def test_pool_poison(oracle):
    """pool_poison 0x5A and 0x00 under (1, 1), twice each: the totals, the inverses and the class tables are written before they are read"""
    from test_gpu_pool_poison import own_context, under_both_fills
    n = 1 << 12; zs, ref = coset_reference(oracle, n); cols = lc.columns(oracle, n, 4)
    small = lc.columns(oracle, 8, 3); zsmall = np.ascontiguousarray(np.stack([lc.points(oracle, 8, 1)[0], oracle.mul(lc.points(oracle, 8, 1)[0], lc.omega_of(oracle, 8))]))
    for max_partials in (-1, 3 * 4 * lc.workgroups(n)):
        with own_context(lagrange_shared_inverse=1, lagrange_share_cosets=1, lagrange_max_partials=max_partials) as c:
            under_both_fills(c, [("n = 2^12, the coset points, max_partials %d" % max_partials, lambda c: run_batch(c, [dev(v) for v in cols], n, zs), ref),
                                 ("n = 8, (z, z w), max_partials %d" % max_partials, lambda c: run_batch(c, [dev(v) for v in small], 8, zsmall), lc.r2(oracle, small, zsmall))])


def test_stream_order(gpu_ctx, oracle):
    """behind a long queued sponge the call returns while the stream is still busy; the points and the pointer table are overwritten on return; the
    result is that of the synchronised run"""
    import queued_cases as qc
    n = 1 << 12; zs0, ref = coset_reference(oracle, n); cols = lc.columns(oracle, n, 4)

    def pipeline(run):
        cb = Band(list(cols)); out = Band([zs0.shape[0] * 4])
        lib, h = gpu_ctx.lib, gpu_ctx.h
        gpu_ctx.sync()
        run.begin()
        t, zs = qc.table([cb.ptr(i) for i in range(4)]), np.array(zs0)
        run.call("stark_lagrange_eval_on_h_batch_dev", lambda: lib.stark_lagrange_eval_on_h_batch_dev(h, 4, t, n, None, zs.shape[0], hp(zs), out.ptr(0)), t, zs)
        hst = qc.finish(run, out, [cb], "the coset points under (1, 1), %s run" % run.mode, strict=True)
        return out.payload(0, hst).reshape(zs0.shape[0], 4, 4)

    with opts(gpu_ctx, (1, 1)):
        a = pipeline(qc.Run(gpu_ctx, oracle, "sync")); b = pipeline(qc.Run(gpu_ctx, oracle, "queued"))
    same(a, ref, "the synchronised run against R2"); same(b, a, "the queued run against the synchronised run")


def test_refused_allocations(oracle):
    """stark_diag_alloc_refusal mode 1 swept over every request of one small call under (1, 1): STARK_ERR_OOM, the cached bytes as before, and the next
    call right"""
    from stark_mlwe_amd.api import StarkError
    from test_gpu_pool_poison import own_context
    n = 1 << 12; zs, ref = coset_reference(oracle, n); inside = lc.inside_points(oracle, n)[3][0]
    zs = np.ascontiguousarray(np.concatenate([zs[:2], [inside], zs[2:]])); cols = lc.columns(oracle, n, 4); want = lc.r2(oracle, cols, zs)
    with own_context(lagrange_shared_inverse=1, lagrange_share_cosets=1) as c:
        dcols = [dev(v) for v in cols]
        same(run_batch(c, dcols, n, zs), want, "the warming call")
        c.diag_alloc_refusal(1, 0)
        same(run_batch(c, dcols, n, zs), want, "the counting call")
        total, fired = c.diag_alloc_refusal(0)[:2]
        assert fired == 0 and total >= 13, total                  # the driver's own: the columns' table, 2 tables of the gather, 3 of the points, 4 of the classes, the partials, 2 of the shared inverse
        cached = c.cached_bytes()
        for nth in range(1, total + 1):
            c.diag_alloc_refusal(1, nth)
            with pytest.raises(StarkError) as e:
                run_batch(c, dcols, n, zs)
            assert e.value.code == OOM, "request %d of %d: %s" % (nth, total, e.value)
            assert c.diag_alloc_refusal(0)[1] == 1, nth
            c.sync()
            assert c.cached_bytes() == cached, "request %d: %d bytes cached after the refused call, %d before" % (nth, c.cached_bytes(), cached)
            same(run_batch(c, dcols, n, zs), want, "the call after refused request %d" % nth)
            assert c.cached_bytes() == cached, nth
        c.diag_alloc_refusal(1, total + 1)
        same(run_batch(c, dcols, n, zs), want, "one request past the last")
        assert c.diag_alloc_refusal(0)[1] == 0


def test_option_contract(gpu_ctx):
    from stark_mlwe_amd.api import StarkError
    for key in ("lagrange_shared_inverse", "lagrange_share_cosets"):
        for ok in (1, 0, -1):
            gpu_ctx.set_option(key, ok)
        for bad in (2, -2):
            with pytest.raises(StarkError) as e:
                gpu_ctx.set_option(key, bad)
            assert e.value.code == ERR_INVALID_ARG and key in str(e.value), str(e.value)
    with pytest.raises(StarkError) as e:
        gpu_ctx.set_option("no_such_option", 1)
    assert "lagrange_shared_inverse" in str(e.value) and "lagrange_share_cosets" in str(e.value), str(e.value)
