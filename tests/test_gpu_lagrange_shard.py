"""The sharded lagrange_eval_on_h on the device: stark_lagrange_eval_shard_dev per block plus stark_lagrange_eval_from_partials_dev over the partition
matrix of lagrange_shard_cases.py, the collective call without a communicator, its emulation for 1..8 virtual ranks, and the column groups of
k_lagrange_partials.  Everything must equal the definition (R2 of lagrange_cases.py), the columns' own bytes inside H and the unsharded
stark_lagrange_eval_on_h_batch_dev, byte for byte; nothing outside the outputs is written and bad arguments are refused before anything is launched.
Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import lagrange_cases as lc
import lagrange_shard_cases as sc
from test_gpu_guard_bands import SENTINEL, Band, hp
from test_gpu_lagrange_eval import dev, host, options, run_batch, same, table

pytestmark = pytest.mark.gpu
vp = C.c_void_p
ERR_INVALID_ARG = -1


def sentinel(rows):
    import torch
    return torch.full((rows, 4), SENTINEL, dtype=torch.int64, device="cuda")


def queue_partitioned(ctx, dcols, n, blocks, zs, parts, out, omega=None):
    """one shard call per block and the combine, queued back to back: no synchronisation in between"""
    total = zs.shape[0] * len(dcols)
    for b, (j0, nl) in enumerate(blocks):
        ctx.lagrange_eval_shard_dev([t.data_ptr() + 32 * j0 for t in dcols], nl, j0, n, zs, parts.data_ptr() + 32 * total * b, omega)
    ctx.lagrange_eval_from_partials_dev(len(blocks), parts.data_ptr(), len(dcols), n, zs, out.data_ptr(), omega)


def run_partitioned(ctx, dcols, n, blocks, zs, omega=None):
    """-> ((P, C, 4) result, (W, P, C, 4) shares); both outputs start as the sentinel"""
    zs = np.ascontiguousarray(zs, np.uint64).reshape(-1, 4); P, Cn = zs.shape[0], len(dcols)
    parts = sentinel(len(blocks) * P * Cn); out = sentinel(P * Cn)
    ctx.sync()
    queue_partitioned(ctx, dcols, n, blocks, zs, parts, out, omega)
    ctx.sync()
    return host(out).reshape(P, Cn, 4), host(parts).reshape(len(blocks), P, Cn, 4)


def run_emulated(ctx, W, dcols, n, zs, omega=None):
    zs = np.ascontiguousarray(zs, np.uint64).reshape(-1, 4); P, Cn = zs.shape[0], len(dcols)
    out = sentinel(W * P * Cn)
    ctx.sync()
    ctx.diag_lagrange_eval_sharded_emulated(W, [t.data_ptr() for t in dcols], n, zs, out.data_ptr(), omega)
    ctx.sync()
    return host(out).reshape(W, P, Cn, 4)


def test_partition_matrix(gpu_ctx, oracle):
    """every partition: all shard calls and combines of the whole matrix are queued before the first synchronisation; against R2, the columns' bytes
    inside H (the owner's share; zero bytes elsewhere) and the batch call on the whole columns"""
    runs = []
    gpu_ctx.sync()
    for n, blocks in sc.PARTITIONS:
        dcols = [dev(v) for v in lc.columns(oracle, n, 3)]; zs, _ = sc.mixed_points(oracle, n, blocks)
        parts = sentinel(len(blocks) * zs.shape[0] * 3); out = sentinel(zs.shape[0] * 3)
        runs.append((dcols, parts, out))
    gpu_ctx.sync()
    for (n, blocks), (dcols, parts, out) in zip(sc.PARTITIONS, runs):
        queue_partitioned(gpu_ctx, dcols, n, blocks, sc.mixed_points(oracle, n, blocks)[0], parts, out)
    gpu_ctx.sync()
    for (n, blocks), (dcols, parts, out) in zip(sc.PARTITIONS, runs):
        cols = lc.columns(oracle, n, 3); zs, ins = sc.mixed_points(oracle, n, blocks); what = "n = %d, blocks %s" % (n, blocks)
        got = host(out).reshape(zs.shape[0], 3, 4); shares = host(parts).reshape(len(blocks), zs.shape[0], 3, 4)
        same(got, sc.reference(oracle, n, blocks), what + " against R2")
        for q, j in ins:
            for b, (j0, nl) in enumerate(blocks):
                want = np.stack([v[j] for v in cols]) if j0 <= j < j0 + nl else np.zeros((3, 4), np.uint64)
                same(shares[b, q], want, what + ": the share of block %d at z = omega^%d" % (b, j))
        same(got, run_batch(gpu_ctx, dcols, n, zs), what + " against the batch call")
        for t, w in zip(dcols, cols):
            same(host(t), w, what + ": a column after the calls")


@pytest.mark.parametrize("n", [1 << 12, 1 << 14])
def test_emulated_ranks(gpu_ctx, oracle, n):
    """W = 1, 2, 4, 8 virtual ranks with 1, 3 and 9 columns: every rank's table equals the batch call's (and R2)"""
    zs, _ = sc.mixed_points(oracle, n, sc.even(n, 2)); dcols = [dev(v) for v in lc.columns(oracle, n)]
    want = run_batch(gpu_ctx, dcols, n, zs)
    same(want[:, :3], sc.reference(oracle, n, sc.even(n, 2)), "the batch call against R2")
    for W in (1, 2, 4, 8):
        for ncols in (1, 3, 9):
            got = run_emulated(gpu_ctx, W, dcols[:ncols], n, zs)
            for q in range(W):
                same(got[q], want[:, :ncols], "n = %d, W = %d, %d columns: virtual rank %d" % (n, W, ncols, q))


def test_emulated_one_row_per_rank_and_another_root(gpu_ctx, oracle):
    n = 8; cols = lc.columns(oracle, n, 3); dcols = [dev(v) for v in cols]; zs, _ = sc.mixed_points(oracle, n, sc.even(n, 8))
    got = run_emulated(gpu_ctx, 8, dcols, n, zs); want = run_batch(gpu_ctx, dcols, n, zs)
    same(want, sc.reference(oracle, n, sc.even(n, 8)), "the batch call against R2 at n = 8")
    for q in range(8):
        same(got[q], want, "n = 8, W = 8: virtual rank %d" % q)
    n = 1 << 12; v = lc.columns(oracle, n, 1)[0]; w3, u = lc.third_power_domain(oracle, v)
    zs = np.concatenate([lc.points(oracle, n, 2), [oracle.pow(w3, n // 2 + 5)]])
    got = run_emulated(gpu_ctx, 2, [dev(v)], n, zs, omega=w3)
    same(got[0], lc.r2(oracle, [u], zs), "omega^3 as the generator, W = 2"); same(got[1], got[0], "the second virtual rank")
    same(got[0][2], v[n // 2 + 5:n // 2 + 6], "z = (omega^3)^(n/2 + 5)")
    cols = lc.corner_columns(n, 3); zs = lc.corners()[:11]
    got, _ = run_partitioned(gpu_ctx, [dev(c) for c in cols], n, sc.even(n, 4), zs)
    same(got, lc.r2(oracle, cols, zs), "corner columns and points at n = 2^12, W = 4")


def test_collective_call_without_a_communicator(gpu_ctx, oracle):
    """stark_lagrange_eval_on_h_sharded_dev at W = 1: the bytes of the batch call"""
    for n, ncols in ((8, 3), (1 << 12, 9)):
        dcols = [dev(v) for v in lc.columns(oracle, n, ncols)]; zs, _ = sc.mixed_points(oracle, n, sc.even(n, 2))
        out = sentinel(zs.shape[0] * ncols)
        gpu_ctx.sync()
        gpu_ctx.lagrange_eval_on_h_sharded([t.data_ptr() for t in dcols], n, zs, out.data_ptr())
        gpu_ctx.sync()
        got = host(out).reshape(zs.shape[0], ncols, 4)
        same(got, run_batch(gpu_ctx, dcols, n, zs), "n = %d: the collective call against the batch call" % n)
        same(got[:, :3], sc.reference(oracle, n, sc.even(n, 2)), "n = %d: against R2" % n)


def test_option_lagrange_col_groups(oracle):
    """-1, 1, 2, 9 and 64 groups of 9 and 17 columns, both accumulators, under pool_poison 0x5A and 0x00: the batch call and the shares of two uneven
    blocks keep every byte"""
    from stark_mlwe_amd.api import StarkError
    from test_gpu_pool_poison import own_context
    n = 1 << 12; blocks = [(0, 1000), (1000, 3096)]; zs = lc.points(oracle, n, 2)
    with own_context() as c:
        dall = [dev(v) for v in sc.columns17(oracle, n)]
        for ncols in sc.GROUP_NCOLS:
            want = sc.reference17(oracle, n, zs)[:, :ncols]; first = None
            for fill in (0x5A, 0x00):
                for acc in (1, 0):
                    for g in (-1, 1, 2, 9, 64):
                        with options(c, pool_poison=fill, lagrange_wide_acc=acc, lagrange_col_groups=g):
                            what = "%d columns, lagrange_col_groups = %d, wide_acc = %d, fill %#x" % (ncols, g, acc, fill)
                            same(run_batch(c, dall[:ncols], n, zs), want, what + ": the batch call")
                            got, shares = run_partitioned(c, dall[:ncols], n, blocks, zs)
                            same(got, want, what + ": two blocks")
                            first = shares if first is None else first
                            same(shares, first, what + ": the shares")
        for bad in (0, -2, 65536):
            with pytest.raises(StarkError) as e:
                c.set_option("lagrange_col_groups", bad)
            assert "lagrange_col_groups" in str(e.value), str(e.value)


def test_automatic_column_groups(gpu_ctx, oracle, hostcheck):
    """64 columns of 2^12 rows at two points: 2 tiles x 2 point groups is below the target, so the automatic rule splits the columns (8 groups of 8);
    the bytes are those of one group, of R2 for the distinct columns, and of a sharded run"""
    n = 1 << 12; zs = lc.points(oracle, n, 2); pick = [(5 * i) % 17 for i in range(64)]
    assert sc.hc_col_groups(hostcheck, -1, 64, n, 2) == (8, 8)
    dall = [dev(v) for v in sc.columns17(oracle, n)]; dcols = [dall[i] for i in pick]
    auto = run_batch(gpu_ctx, dcols, n, zs)
    same(auto, sc.reference17(oracle, n, zs)[:, pick], "64 columns under the automatic rule against R2")
    with options(gpu_ctx, lagrange_col_groups=1):
        same(run_batch(gpu_ctx, dcols, n, zs), auto, "one group against the automatic rule")
    same(run_emulated(gpu_ctx, 2, dcols, n, zs)[1], auto, "two virtual ranks of 64 columns")


@pytest.mark.parametrize("n", [8, 1 << 12])
def test_between_guard_bands(gpu_ctx, oracle, n):
    """partials_out and out between sentinel rows, the block's rows inside banded columns: nothing outside is written, the columns keep every byte,
    and the results do not depend on what the outputs held"""
    cols = lc.columns(oracle, n, 3); blocks = sc.even(n, 2); zs, _ = sc.mixed_points(oracle, n, blocks); P = zs.shape[0]
    want = sc.reference(oracle, n, blocks).reshape(-1, 4)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    for prefill in (SENTINEL, 0):
        cb = Band(cols); pb = Band([2 * P * 3], prefill=prefill); ob = Band([P * 3], prefill=prefill); eb = Band([2 * P * 3], prefill=prefill)
        gpu_ctx.sync()
        for b, (j0, nl) in enumerate(blocks):
            rc = lib.stark_lagrange_eval_shard_dev(h, 3, table([cb.ptr(c).value + 32 * j0 for c in range(3)]), nl, j0, n, None, P, hp(zs), vp(pb.ptr().value + 32 * P * 3 * b))
            assert rc == 0, lib.stark_last_error(h)
        gpu_ctx.sync()
        ph = pb.host(); pb.check("partials_out, prefill %#x" % prefill, ph)
        assert lib.stark_lagrange_eval_from_partials_dev(h, 2, pb.ptr(), 3, n, None, P, hp(zs), ob.ptr()) == 0, lib.stark_last_error(h)
        assert lib.stark_diag_lagrange_eval_sharded_emulated_dev(h, 2, 3, table([cb.ptr(c).value for c in range(3)]), n, None, P, hp(zs), eb.ptr()) == 0, lib.stark_last_error(h)
        gpu_ctx.sync()
        oh = ob.host(); ob.check("out, prefill %#x" % prefill, oh); eh = eb.host(); eb.check("out of the emulation, prefill %#x" % prefill, eh)
        same(ob.payload(0, oh), want, "n = %d between bands, prefill %#x" % (n, prefill))
        same(eb.payload(0, eh), np.concatenate([want, want]), "n = %d, the emulation between bands, prefill %#x" % (n, prefill))
        same(pb.host(), ph, "the partials after the combine")
        cb.check_unchanged("the columns")


def test_bad_arguments_are_refused_before_any_launch(gpu_ctx, oracle):
    """every STARK_ERR_INVALID_ARG case of the header comments: the buffer keeps its pre-fill and stark_last_error names the argument; empty calls are
    STARK_OK and write nothing"""
    lib, h = gpu_ctx.lib, gpu_ctx.h
    n = 8; nl = 4
    zs = np.ascontiguousarray(lc.points(oracle, n, 2)); one = oracle.from_u64(1)
    buf = sentinel(2 * n + 16 + 4)                                  # [column 0 | column 1 | out (up to 4 ranks x 2 x 2) | spare]
    c0, c1, o = buf.data_ptr(), buf.data_ptr() + 32 * n, buf.data_ptr() + 64 * n
    tt = table([c0, c1])
    sh, fp, co, em = lib.stark_lagrange_eval_shard_dev, lib.stark_lagrange_eval_from_partials_dev, lib.stark_lagrange_eval_on_h_sharded_dev, lib.stark_diag_lagrange_eval_sharded_emulated_dev
    cases = {"shard: null ctx": (lambda: sh(None, 2, tt, nl, 0, n, None, 2, hp(zs), vp(o)), None),
             "shard: n_local = 0": (lambda: sh(h, 2, tt, 0, 0, n, None, 2, hp(zs), vp(o)), "n_local"),
             "shard: j0 + n_local > n_global": (lambda: sh(h, 2, tt, nl, 5, n, None, 2, hp(zs), vp(o)), "j0 + n_local"),
             "shard: j0 > n_global": (lambda: sh(h, 2, tt, nl, 1 << 40, n, None, 2, hp(zs), vp(o)), "j0 + n_local"),
             "shard: n_global = 12": (lambda: sh(h, 2, tt, nl, 0, 12, None, 2, hp(zs), vp(o)), "power of two"),
             "shard: n_global = 2^31": (lambda: sh(h, 2, tt, nl, 0, 1 << 31, None, 2, hp(zs), vp(o)), "2^30"),
             "shard: omega = 1": (lambda: sh(h, 2, tt, nl, 0, n, hp(one), 2, hp(zs), vp(o)), "primitive"),
             "shard: omega of order 2 n": (lambda: sh(h, 2, tt, nl, 0, n, hp(oracle.domain_omega(2 * n)), 2, hp(zs), vp(o)), "omega^n != 1"),
             "shard: null table": (lambda: sh(h, 2, None, nl, 0, n, None, 2, hp(zs), vp(o)), "null column table"),
             "shard: null entry": (lambda: sh(h, 2, table([c0, 0]), nl, 0, n, None, 2, hp(zs), vp(o)), "null column entry 1"),
             "shard: null z": (lambda: sh(h, 2, tt, nl, 0, n, None, 2, None, vp(o)), "null z"),
             "shard: null partials_out": (lambda: sh(h, 2, tt, nl, 0, n, None, 2, hp(zs), None), "null out"),
             "shard: partials_out on the block's last row": (lambda: sh(h, 2, tt, nl, 0, n, None, 2, hp(zs), vp(c1 + 32 * (nl - 1))), "out overlaps column 1"),
             "shard: partials_out ends on the block's first row": (lambda: sh(h, 2, table([c1, c1]), nl, 0, n, None, 2, hp(zs), vp(c1 - 32 * 3)), "out overlaps column 0"),
             "from_partials: null ctx": (lambda: fp(None, 2, vp(o), 2, n, None, 2, hp(zs), vp(o + 32 * 8)), None),
             "from_partials: nparts = 0": (lambda: fp(h, 0, vp(o), 2, n, None, 2, hp(zs), vp(o + 32 * 8)), "nparts"),
             "from_partials: null partials": (lambda: fp(h, 2, None, 2, n, None, 2, hp(zs), vp(o + 32 * 8)), "null partials"),
             "from_partials: null out": (lambda: fp(h, 2, vp(o), 2, n, None, 2, hp(zs), None), "null out"),
             "from_partials: null z": (lambda: fp(h, 2, vp(o), 2, n, None, 2, None, vp(o + 32 * 8)), "null z"),
             "from_partials: n_global = 12": (lambda: fp(h, 2, vp(o), 2, 12, None, 2, hp(zs), vp(o + 32 * 8)), "power of two"),
             "from_partials: omega = 1": (lambda: fp(h, 2, vp(o), 2, n, hp(one), 2, hp(zs), vp(o + 32 * 8)), "primitive"),
             "from_partials: out is the last part": (lambda: fp(h, 2, vp(o), 2, n, None, 2, hp(zs), vp(o + 32 * 4)), "out overlaps partials"),
             "from_partials: out ends on the first row": (lambda: fp(h, 2, vp(o + 32 * 3), 2, n, None, 2, hp(zs), vp(o)), "out overlaps partials"),
             "collective: null ctx": (lambda: co(None, 2, tt, n, None, 2, hp(zs), vp(o)), None),
             "collective: null table": (lambda: co(h, 2, None, n, None, 2, hp(zs), vp(o)), "null column table"),
             "collective: null entry": (lambda: co(h, 2, table([0, c1]), n, None, 2, hp(zs), vp(o)), "null column entry 0"),
             "collective: null z": (lambda: co(h, 2, tt, n, None, 2, None, vp(o)), "null z"),
             "collective: null out": (lambda: co(h, 2, tt, n, None, 2, hp(zs), None), "null out"),
             "collective: n_global = 12": (lambda: co(h, 2, tt, 12, None, 2, hp(zs), vp(o)), "power of two"),
             "collective: n_global = 0": (lambda: co(h, 2, tt, 0, None, 2, hp(zs), vp(o)), "n_global"),
             "collective: omega = 1": (lambda: co(h, 2, tt, n, hp(one), 2, hp(zs), vp(o)), "primitive"),
             "collective: out inside column 1": (lambda: co(h, 2, tt, n, None, 2, hp(zs), vp(c1 + 32)), "out overlaps column 1"),
             "emulated: null ctx": (lambda: em(None, 2, 2, tt, n, None, 2, hp(zs), vp(o)), None),
             "emulated: nranks = 3": (lambda: em(h, 3, 2, tt, n, None, 2, hp(zs), vp(o)), "nranks"),
             "emulated: nranks = 0": (lambda: em(h, 0, 2, tt, n, None, 2, hp(zs), vp(o)), "nranks"),
             "emulated: nranks = -2": (lambda: em(h, -2, 2, tt, n, None, 2, hp(zs), vp(o)), "nranks"),
             "emulated: nranks above n_global": (lambda: em(h, 16, 2, tt, n, None, 2, hp(zs), vp(o)), "nranks"),
             "emulated: n_global = 12": (lambda: em(h, 4, 2, tt, 12, None, 2, hp(zs), vp(o)), "power of two"),
             "emulated: null table": (lambda: em(h, 2, 2, None, n, None, 2, hp(zs), vp(o)), "null column table"),
             "emulated: null entry": (lambda: em(h, 2, 2, table([c0, 0]), n, None, 2, hp(zs), vp(o)), "null column entry 1"),
             "emulated: null z": (lambda: em(h, 2, 2, tt, n, None, 2, None, vp(o)), "null z"),
             "emulated: null out": (lambda: em(h, 2, 2, tt, n, None, 2, hp(zs), None), "null out"),
             "emulated: the second rank's out on column 0": (lambda: em(h, 2, 2, tt, n, None, 2, hp(zs), vp(c0 - 32 * 7)), "out overlaps column 0")}
    for what, (fn, reason) in cases.items():
        gpu_ctx.sync()
        assert fn() == ERR_INVALID_ARG, what
        if reason is not None:
            assert reason in lib.stark_last_error(h).decode(), (what, lib.stark_last_error(h))
        gpu_ctx.sync()
        assert (host(buf) == SENTINEL).all(), "%s: something was written" % what
    assert sh(h, 0, None, nl, 0, n, None, 2, hp(zs), vp(o)) == 0 and sh(h, 2, tt, nl, 0, n, None, 0, None, vp(o)) == 0
    assert fp(h, 0, None, 0, n, None, 2, hp(zs), vp(o)) == 0 and fp(h, 0, None, 2, n, None, 0, None, vp(o)) == 0
    assert co(h, 0, None, n, None, 2, hp(zs), vp(o)) == 0 and em(h, 2, 2, tt, n, None, 0, None, vp(o)) == 0
    gpu_ctx.sync()
    assert (host(buf) == SENTINEL).all()
    import torch
    cols = lc.columns(oracle, n, 2); buf[:n] = dev(cols[0]); buf[n:2 * n] = dev(cols[1]); torch.cuda.synchronize()     # the context is usable afterwards; out next to the columns is allowed
    gpu_ctx._chk(em(h, 4, 2, tt, n, None, 2, hp(zs), vp(o))); gpu_ctx.sync()
    got = host(buf)[2 * n:2 * n + 16].reshape(4, 2, 2, 4)
    for q in range(4):
        same(got[q], lc.matrix_reference(oracle, n)[:2, :2], "virtual rank %d after the refused calls" % q)
    assert (host(buf)[2 * n + 16:] == SENTINEL).all()
