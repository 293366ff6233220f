"""stark_lde_mixed_batch_dev / stark_ntt_mixed_batch_dev: columns of any lengths, one blow-up and one coset, in one device pass.  Column i of every
result must equal, bit for bit, the CPU oracle and what the single call (stark_lde_dev / stark_ntt_dev) gives for that column alone — on every
first-pass route of the big forward transform (tests/lde_shapes.py), for one-, two- and three-pass plans in ONE call, under every NTT option, across
pass cuts and changes of the cached cosets, with corner inputs, repeated and aliased pointers, between guard bands, under the pool poison, behind a busy
stream with the host arrays destroyed on return, and for every refused argument.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import json
import os
import statistics
import time

import numpy as np
import pytest

import corner_values as cv
import lde_shapes as ls
import pyref
import queued_cases as qc
from test_gpu_guard_bands import Band, SENTINEL, guarded, hp, same, sync
from test_gpu_lde_batch import DEFAULT_MAX_ELEMS, ERR_INVALID_ARG, GEN, PRIMES, dev, host, lde_single, shift_of, table
from test_gpu_lde_blowups import OPTIONS, with_options

pytestmark = pytest.mark.gpu

from stark_mlwe_amd.api import _ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# log_blowup -> log_n list of one call: unsorted, with repeats; together every route and P = 1, 2, 3 (asserted below)
CALLS = {3: [8, 0, 18, 5, 8, 9, 3], 4: [7, 12, 7, 2], 6: [5, 4, 8, 5, 6], 1: [10, 9, 11, 0], 0: [11, 3, 0, 10, 11], 7: [4, 0, 6]}
NTT_SIZES = [11, 0, 3, 10, 1, 12, 11]
SMALL = [8, 5, 11]


def sizes(n):
    return (C.c_size_t * max(len(n), 1))(*n)


def test_call_list_reaches_every_route_and_pass_count():
    keys = {ls.route(ln, lb, pre) for lb, lns in CALLS.items() for ln in lns for pre in (0, 1)}
    assert {name for _, name in keys} == {ls.NO_EXTENSION, ls.PADDED, ls.FAST, ls.FAST_ZERO, ls.FAST_ZERO_ONE, ls.GENERAL, ls.UNIT}
    assert {P for P, _ in keys} == {1, 2, 3}
    assert [ln for ln in CALLS[3] if ls.passes(ln, 3) == 3] == [18] and max(ln + lb for lb, lns in CALLS.items() for ln in lns) == 21


@pytest.fixture(scope="module")
def columns(oracle):
    """(field, log_n, lb, column, shift name) -> (input, oracle LDE), computed once and shared by the tests of this module"""
    memo = {}

    def get(field, log_n, lb, c, sname):
        key = (field, log_n, lb, c, sname)
        if key not in memo:
            x = oracle.synth_column(0x3A7C000 + 64 * log_n + lb, c, 0, 1 << log_n)          # stored values below 2^254: elements of both fields
            memo[key] = (x, oracle.lde(field, x, lb, shift_of(oracle, field, sname)))
        return memo[key]
    return get


def lde_mixed(ctx, field, xs, log_ns, lb, shift, prefill=SENTINEL):
    """stark_lde_mixed_batch_dev on the device columns xs -> list of host results (outputs start as a sentinel pattern: the skip routes never pad)"""
    import torch
    outs = [torch.full((1 << (ln + lb), 4), prefill, dtype=torch.int64, device="cuda") for ln in log_ns]
    sync(ctx)
    ctx.lde_mixed_batch_dev(field, [x.data_ptr() for x in xs], log_ns, lb, [o.data_ptr() for o in outs], shift)
    sync(ctx)
    return [host(o) for o in outs]


def small_case(oracle, columns, lb=3, lns=SMALL, sname="generator"):
    ins = [columns(0, ln, lb, c, sname) for c, ln in enumerate(lns)]
    return ins, [dev(x) for x, _ in ins], shift_of(oracle, 0, sname)


@pytest.mark.parametrize("lb", list(CALLS), ids=lambda v: "lb%d" % v)
def test_lde_mixed_every_route_equals_oracle_and_single_call(gpu_ctx, oracle, columns, lb):
    """one call per blow-up and shift: every column against oracle.lde and stark_lde_dev; the inputs stay intact"""
    lns = CALLS[lb]
    for field in [0] + ([1] if 18 not in lns else []):
        for sname in ("none", "generator"):
            shift = shift_of(oracle, field, sname)
            ins = [columns(field, ln, lb, c, sname) for c, ln in enumerate(lns)]
            xs = [dev(x) for x, _ in ins]
            got = lde_mixed(gpu_ctx, field, xs, lns, lb, shift)
            for c, ln in enumerate(lns):
                what = "field %d, lb = %d, column %d (log_n = %d), %d-pass route '%s', shift '%s'" % ((field, lb, c, ln) + ls.route(ln, lb, sname != "none") + (sname,))
                same(got[c], ins[c][1], what + " against the oracle")
                same(got[c], lde_single(gpu_ctx, field, xs[c], ln, lb, shift), what + " against stark_lde_dev")
            for x, (xin, _) in zip(xs, ins):
                assert (host(x) == xin).all(), "an input was modified"
            del xs, got


@pytest.mark.parametrize("field", [0, 1])
def test_ntt_mixed_equals_oracle_and_single_call(gpu_ctx, oracle, field):
    """stark_ntt_mixed_batch_dev, forward and inverse, with and without coset, against oracle.ntt and stark_ntt_dev; one Pallas call includes 2^21 points"""
    for inverse in (False, True):
        for coset in (None, oracle.from_u64(GEN[field], field)):
            lns = NTT_SIZES + ([21] if field == 0 and inverse and coset is not None else [])
            cols = [oracle.synth_column(0x177C + ln, c, 0, 1 << ln) for c, ln in enumerate(lns)]
            xs = [dev(x) for x in cols]; ys = [dev(x) for x in cols]
            sync(gpu_ctx)
            gpu_ctx.ntt_mixed_batch_dev(field, [x.data_ptr() for x in xs], lns, inverse, coset)
            for y, ln in zip(ys, lns):
                gpu_ctx._chk(gpu_ctx.lib.stark_ntt_dev(gpu_ctx.h, field, C.c_void_p(y.data_ptr()), ln, int(inverse), _ptr(coset)))
            sync(gpu_ctx)
            for c, ln in enumerate(lns):
                what = "field %d, column %d (2^%d), inverse %d, coset %s" % (field, c, ln, inverse, coset is not None)
                same(host(xs[c]), oracle.ntt(field, cols[c], inverse=inverse, coset=coset), what + " against the oracle")
                same(host(xs[c]), host(ys[c]), what + " against stark_ntt_dev")
            del xs, ys


def test_degenerate_batches(gpu_ctx, oracle, columns):
    """B = 1; all columns of one size, byte for byte what stark_lde_batch_dev gives; all columns of one point"""
    import torch
    shift = shift_of(oracle, 0, "generator")
    x, want = columns(0, 8, 3, 0, "generator")
    same(lde_mixed(gpu_ctx, 0, [dev(x)], [8], 3, shift)[0], want, "B = 1")
    ins = [columns(0, 8, 3, c, "generator") for c in range(5)]
    xs = [dev(a) for a, _ in ins]
    got = lde_mixed(gpu_ctx, 0, xs, [8] * 5, 3, shift)
    outs = [torch.full((1 << 11, 4), SENTINEL, dtype=torch.int64, device="cuda") for _ in xs]
    gpu_ctx.lde_batch_dev(0, [a.data_ptr() for a in xs], 8, 3, [o.data_ptr() for o in outs], shift); sync(gpu_ctx)
    for c in range(5):
        same(got[c], ins[c][1], "one size, column %d" % c); same(got[c], host(outs[c]), "one size, column %d against stark_lde_batch_dev" % c)
    pts = [columns(0, 0, 3, c, "generator") for c in range(3)]
    for lb in (3, 0):
        got = lde_mixed(gpu_ctx, 0, [dev(a) for a, _ in pts], [0] * 3, lb, shift)
        for c in range(3):
            same(got[c], np.repeat(pts[c][0], 1 << lb, axis=0), "all columns of one point, lb = %d, column %d" % (lb, c))
    ys = [dev(a) for a, _ in pts]
    gpu_ctx.ntt_mixed_batch_dev(0, [y.data_ptr() for y in ys], [0] * 3, False, shift); sync(gpu_ctx)
    assert all((host(y) == a).all() for y, (a, _) in zip(ys, pts)), "a one-point vector takes no part in the transform"


def test_lde_mixed_corners_repeated_and_aliased_pointers(gpu_ctx, oracle, columns):
    """{8, 5, 11} plus a second 2^5 column, generator shift: the stored-limb corner list as the 2^8 column, one input pointer used for both 2^5 columns,
    and the 2^11 column's output buffer starting as its input"""
    import torch
    lb, lns = 3, [8, 5, 11, 5]
    shift = shift_of(oracle, 0, "generator")
    corners = cv.patterns(PRIMES[0], 1 << 8)["corners by index"]
    x5, w5 = columns(0, 5, lb, 1, "generator"); x11, w11 = columns(0, 11, lb, 2, "generator")
    d8, d5 = dev(corners), dev(x5)
    outs = [torch.full((1 << (ln + lb), 4), SENTINEL, dtype=torch.int64, device="cuda") for ln in lns]
    outs[2][:1 << 11] = dev(x11)                                           # column 2: evals == out
    sync(gpu_ctx)
    gpu_ctx.lde_mixed_batch_dev(0, [d8.data_ptr(), d5.data_ptr(), outs[2].data_ptr(), d5.data_ptr()], lns, lb, [o.data_ptr() for o in outs], shift)
    sync(gpu_ctx)
    for c, want in enumerate((oracle.lde(0, corners, lb, shift), w5, w11, w5)):
        same(host(outs[c]), want, "column %d" % c)
    assert (host(d8) == corners).all() and (host(d5) == x5).all(), "an input that aliases no output was modified"


def test_lde_mixed_pass_cutting_on_the_device(gpu_ctx, oracle, columns):
    """[8, 8, 5, 11, 8] at blow-up 3 with passes of at most 2 * 2^11 outputs: {8, 8}, {5}, {11}, {8} — three passes through the single path"""
    lb, lns = 3, [8, 8, 5, 11, 8]
    ins, xs, shift = small_case(oracle, columns, lb, lns)
    gpu_ctx.set_option("ntt_batch_max_elems", 2 << 11)
    try:
        got = lde_mixed(gpu_ctx, 0, xs, lns, lb, shift)
        cols = [oracle.synth_column(0x9A56, c, 0, 1 << ln) for c, ln in enumerate([10, 10, 11, 3])]
        ys = [dev(x) for x in cols]
        gpu_ctx.ntt_mixed_batch_dev(0, [y.data_ptr() for y in ys], [10, 10, 11, 3], False, shift); sync(gpu_ctx)      # {10, 10, 11}, {3}
    finally:
        gpu_ctx.set_option("ntt_batch_max_elems", DEFAULT_MAX_ELEMS)
    for c in range(5):
        same(got[c], ins[c][1], "passes {8, 8} {5} {11} {8}, column %d" % c)
    for c in range(4):
        same(host(ys[c]), oracle.ntt(0, cols[c], inverse=False, coset=shift), "transform passes {10, 10, 11} {3}, column %d" % c)


# ---- launches of one shape inside the mixed calls: addressed by pointer table or base + pitch instead of the ragged lookup ---------------------------
def test_ntt_mixed_one_shape_launch_over_a_subset_of_the_table(gpu_ctx, oracle):
    """[5, 12, 3, 12]: the first launch is the strided pass of caller columns 1 and 3 alone (one shape over a non-prefix subset of the table), the
    last is ragged.  Forward on the generator's coset (Bls12-381 too) and inverse, against stark_ntt_dev and the oracle"""
    lns = [5, 12, 3, 12]
    for field, inverse, with_coset in ((0, False, True), (1, False, True), (0, True, False), (0, True, True)):
        coset = oracle.from_u64(GEN[field], field) if with_coset else None
        cols = [oracle.synth_column(0x51B5 + ln, c, 0, 1 << ln) for c, ln in enumerate(lns)]
        xs = [dev(x) for x in cols]; ys = [dev(x) for x in cols]
        sync(gpu_ctx)
        gpu_ctx.ntt_mixed_batch_dev(field, [x.data_ptr() for x in xs], lns, inverse, coset)
        for y, ln in zip(ys, lns):
            gpu_ctx._chk(gpu_ctx.lib.stark_ntt_dev(gpu_ctx.h, field, C.c_void_p(y.data_ptr()), ln, int(inverse), _ptr(coset)))
        sync(gpu_ctx)
        for c, ln in enumerate(lns):
            what = "field %d, column %d (2^%d), inverse %d, coset %s" % (field, c, ln, inverse, with_coset)
            same(host(xs[c]), oracle.ntt(field, cols[c], inverse=inverse, coset=coset), what + " against the oracle")
            same(host(xs[c]), host(ys[c]), what + " against stark_ntt_dev")


@pytest.mark.parametrize("ln,B,lb", [(8, 4, 3), (4, 3, 1), (0, 3, 2)], ids=["skip-route", "padded-route", "one-point"])
def test_equal_lengths_through_the_mixed_and_the_same_size_call(gpu_ctx, oracle, columns, ln, B, lb):
    """B columns of 2^ln through stark_lde_mixed_batch_dev and stark_lde_batch_dev into separate outputs: byte-equal, the oracle's and stark_lde_dev's
    per column; then with every input the head of its own output.  (4, 1): pad launch between the transforms; (0, 2): pad launch, then a forward pass
    of one shape reading the scratch at pitch N + n.  Bls12-381 once, on the first case"""
    import torch
    for field in [0] + ([1] if ln == 8 else []):
        for sname in ("none", "generator"):
            shift = shift_of(oracle, field, sname)
            ins = [columns(field, ln, lb, c, sname) for c in range(B)]
            xs = [dev(x) for x, _ in ins]
            for alias in (False, True):
                om = [torch.full((1 << (ln + lb), 4), SENTINEL, dtype=torch.int64, device="cuda") for _ in xs]
                ob = [torch.full((1 << (ln + lb), 4), SENTINEL, dtype=torch.int64, device="cuda") for _ in xs]
                if alias:
                    for o, x in zip(om + ob, xs + xs):
                        o[:1 << ln] = x
                im, ib = ([o.data_ptr() for o in om], [o.data_ptr() for o in ob]) if alias else ([x.data_ptr() for x in xs],) * 2
                sync(gpu_ctx)
                gpu_ctx.lde_mixed_batch_dev(field, im, [ln] * B, lb, [o.data_ptr() for o in om], shift)
                gpu_ctx.lde_batch_dev(field, ib, ln, lb, [o.data_ptr() for o in ob], shift)
                sync(gpu_ctx)
                for c in range(B):
                    what = "field %d, (%d, %d), shift '%s', aliased %d, column %d" % (field, ln, lb, sname, alias, c)
                    same(host(om[c]), host(ob[c]), what + ": mixed call against stark_lde_batch_dev")
                    same(host(ob[c]), ins[c][1], what + " against the oracle")
                    if not alias:
                        same(host(ob[c]), lde_single(gpu_ctx, field, xs[c], ln, lb, shift), what + " against stark_lde_dev")
            for x, (xin, _) in zip(xs, ins):
                assert (host(x) == xin).all(), "an input was modified"


def test_equal_lengths_pass_cutting_on_the_device(gpu_ctx, oracle):
    """three vectors of 2^11 points with passes of at most 2 * 2^11 elements, through stark_ntt_mixed_batch_dev ({11, 11} as one-shape launches, {11}
    through the single path) and through stark_ntt_batch_dev (its own driver, cut by the same rule): both against the oracle and stark_ntt_dev"""
    coset = oracle.from_u64(GEN[0], 0)
    cols = [oracle.synth_column(0x9A57, c, 0, 1 << 11) for c in range(3)]
    ms = [dev(x) for x in cols]; ys = [dev(x) for x in cols]
    gpu_ctx.set_option("ntt_batch_max_elems", 2 << 11)
    try:
        gpu_ctx.ntt_mixed_batch_dev(0, [m.data_ptr() for m in ms], [11] * 3, False, coset)
        gpu_ctx.ntt_batch_dev(0, [y.data_ptr() for y in ys], 11, False, coset); sync(gpu_ctx)
    finally:
        gpu_ctx.set_option("ntt_batch_max_elems", DEFAULT_MAX_ELEMS)
    zs = [dev(x) for x in cols]
    for z in zs:
        gpu_ctx._chk(gpu_ctx.lib.stark_ntt_dev(gpu_ctx.h, 0, C.c_void_p(z.data_ptr()), 11, 0, _ptr(coset)))
    sync(gpu_ctx)
    for c in range(3):
        want = oracle.ntt(0, cols[c], inverse=False, coset=coset)
        for name, got in (("mixed", ms[c]), ("same-size", ys[c])):
            same(host(got), want, "%s call, passes {11, 11} {11}, column %d against the oracle" % (name, c))
            same(host(got), host(zs[c]), "%s call, passes {11, 11} {11}, column %d against stark_ntt_dev" % (name, c))


def test_lde_mixed_option_matrix(gpu_ctx, oracle, columns):
    """{8, 5, 11} at blow-up 3, generator shift under every pre-scale form, tile width and launch shape of the single call's option matrix"""
    ins, xs, shift = small_case(oracle, columns)
    for label, opts in OPTIONS.items():
        got = with_options(gpu_ctx, opts, lambda: lde_mixed(gpu_ctx, 0, xs, SMALL, 3, shift))
        for c in range(3):
            same(got[c], ins[c][1], "%s, column %d" % (label, c))


def test_lde_mixed_coset_cache_across_changes_of_coset(gpu_ctx, oracle, columns):
    """mixed call with shift A, single call at one of its sizes with shift B, mixed call with A again: the cached coset of one plan of the call changes"""
    A = shift_of(oracle, 0, "generator"); Bs = oracle.from_int(pow(3, 1000003, PRIMES[0]), 0)
    ins, xs, _ = small_case(oracle, columns)
    first = lde_mixed(gpu_ctx, 0, xs, SMALL, 3, A)
    same(lde_single(gpu_ctx, 0, xs[2], 11, 3, Bs), oracle.lde(0, ins[2][0], 3, Bs), "single call with the second shift")
    again = lde_mixed(gpu_ctx, 0, xs, SMALL, 3, A)
    for c in range(3):
        same(first[c], ins[c][1], "first mixed call, column %d" % c); same(again[c], ins[c][1], "mixed call after the coset changed, column %d" % c)


@pytest.mark.parametrize("lb", [3, 7])
def test_lde_mixed_between_guard_bands(gpu_ctx, oracle, columns, lb):
    """{8, 4, 0}, every buffer between sentinel bands: nothing outside the outputs is written, the inputs stay intact, the result does not depend on what out held"""
    lns = [8, 4, 0]
    ins = [columns(0, ln, lb, c, "generator") for c, ln in enumerate(lns)]
    shift = shift_of(oracle, 0, "generator")

    def call(inb, ob, pre):
        return gpu_ctx.lib.stark_lde_mixed_batch_dev(gpu_ctx.h, 0, 3, table([b.ptr().value for b in inb]), sizes(lns), lb, hp(shift), table([ob.ptr(i).value for i in range(3)]))
    guarded(gpu_ctx, [x for x, _ in ins], [1 << (ln + lb) for ln in lns], call, [w for _, w in ins], "stark_lde_mixed_batch_dev (lb = %d)" % lb)


def test_ntt_mixed_between_guard_bands(gpu_ctx, oracle):
    """vectors of 2^11, 2^3 and 2^10 points one sentinel row apart, transformed in place on the generator's coset"""
    lns = [11, 3, 10]; coset = oracle.from_u64(GEN[0], 0)
    cols = [oracle.synth_column(0x6B12, c, 0, 1 << ln) for c, ln in enumerate(lns)]
    b = Band(cols)
    sync(gpu_ctx)
    gpu_ctx._chk(gpu_ctx.lib.stark_ntt_mixed_batch_dev(gpu_ctx.h, 0, 3, table([b.ptr(i).value for i in range(3)]), sizes(lns), 0, hp(coset)))
    sync(gpu_ctx)
    h = b.host(); b.check("stark_ntt_mixed_batch_dev", h)
    for c in range(3):
        same(b.payload(c, h), oracle.ntt(0, cols[c], inverse=False, coset=coset), "stark_ntt_mixed_batch_dev between bands, column %d" % c)


def test_mixed_calls_under_the_pool_poison(gpu_ctx, oracle, columns):
    """the {8, 5, 11} LDE and the {11, 3, 10} NTT with every pooled block and the scratch filled with 0x5A, then with 0x00: the oracle's bytes under both"""
    ins, xs, shift = small_case(oracle, columns)
    lns = [11, 3, 10]
    cols = [oracle.synth_column(0x6B13, c, 0, 1 << ln) for c, ln in enumerate(lns)]
    want = [oracle.ntt(0, x, inverse=False, coset=shift) for x in cols]
    try:
        for fill in (0x5A, 0x00):
            gpu_ctx.set_option("pool_poison", fill)
            got = lde_mixed(gpu_ctx, 0, xs, SMALL, 3, shift)
            for c in range(3):
                same(got[c], ins[c][1], "LDE under fill %#04x, column %d" % (fill, c))
            ys = [dev(x) for x in cols]
            gpu_ctx.ntt_mixed_batch_dev(0, [y.data_ptr() for y in ys], lns, False, shift); sync(gpu_ctx)
            for c in range(3):
                same(host(ys[c]), want[c], "NTT under fill %#04x, column %d" % (fill, c))
    finally:
        gpu_ctx.set_option("pool_poison", -1)


def test_host_arrays_may_die_on_return_behind_a_busy_stream(gpu_ctx, oracle, columns):
    """behind the long serial sponge of queued_cases: the mixed LDE is queued, log_n, both tables and the shift are destroyed as soon as it returns, the
    blocker's event is still incomplete at that moment, and the result is the oracle's"""
    import torch
    ins, xs, shift = small_case(oracle, columns)
    lde_mixed(gpu_ctx, 0, xs, SMALL, 3, shift)                             # warm plans and coset tables: a cold plan synchronises while it is built
    b = qc.Blocker(gpu_ctx, oracle, 16).start(); sync(gpu_ctx); b.check()  # the blocker's tag frame
    outs = [torch.full((1 << (ln + 3), 4), SENTINEL, dtype=torch.int64, device="cuda") for ln in SMALL]
    lg, it, ot, sh = sizes(SMALL), table([x.data_ptr() for x in xs]), table([o.data_ptr() for o in outs]), np.array(shift, np.uint64).copy()
    torch.cuda.synchronize()
    blocker = qc.Blocker(gpu_ctx, oracle).start()
    rc = gpu_ctx.lib.stark_lde_mixed_batch_dev(gpu_ctx.h, 0, 3, it, lg, 3, hp(sh), ot)
    busy = blocker.still_busy()
    qc.clobber(lg, it, ot, sh)
    gpu_ctx._chk(rc)
    assert busy, "stark_lde_mixed_batch_dev returned only after the stream had drained (blocker: %.1f ms)" % (sync(gpu_ctx) or blocker.ms())
    sync(gpu_ctx); blocker.check()
    for c in range(3):
        same(host(outs[c]), ins[c][1], "queued behind the blocker, host arrays destroyed, column %d" % c)


def test_mixed_calls_refuse_bad_arguments_before_any_launch(gpu_ctx, oracle):
    """every STARK_ERR_INVALID_ARG case of the header comment: the outputs keep their pre-fill; batch == 0 is STARK_OK; the context stays usable"""
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.h
    lb, lns = 2, [4, 2]; N0, N1 = 1 << (4 + lb), 1 << (2 + lb)
    x = dev(oracle.synth_column(0xE45, 0, 0, 16))
    buf = torch.full((N0 + N1 + 1, 4), SENTINEL, dtype=torch.int64, device="cuda")
    o0, o1 = buf.data_ptr(), buf.data_ptr() + 32 * N0
    ins, outs, lg = table([x.data_ptr(), x.data_ptr()]), table([o0, o1]), sizes(lns)
    lde, ntt = lib.stark_lde_mixed_batch_dev, lib.stark_ntt_mixed_batch_dev
    cases = {"null ctx": lambda: lde(None, 0, 2, ins, lg, lb, None, outs),
             "null input table": lambda: lde(h, 0, 2, None, lg, lb, None, outs),
             "null output table": lambda: lde(h, 0, 2, ins, lg, lb, None, None),
             "null log_n": lambda: lde(h, 0, 2, ins, None, lb, None, outs),
             "null input entry": lambda: lde(h, 0, 2, table([x.data_ptr(), 0]), lg, lb, None, outs),
             "null output entry": lambda: lde(h, 0, 2, ins, lg, lb, None, table([o0, 0])),
             "log_n[1] out of range": lambda: lde(h, 0, 2, ins, sizes([4, 31]), 0, None, outs),
             "log_n[1] + log_blowup = 31": lambda: lde(h, 0, 2, ins, sizes([4, 31 - lb]), lb, None, outs),
             "log_blowup out of range": lambda: lde(h, 0, 2, ins, lg, 31, None, outs),
             "unknown field": lambda: lde(h, 7, 2, ins, lg, lb, None, outs),
             "the same output twice": lambda: lde(h, 0, 2, ins, lg, lb, None, table([o0, o0])),
             "a long output overlapping a short one by one row": lambda: lde(h, 0, 2, ins, lg, lb, None, table([o0, o1 - 32])),
             "a short output inside a long one": lambda: lde(h, 0, 2, ins, lg, lb, None, table([o0, o0 + 64])),
             "ntt: null ctx": lambda: ntt(None, 0, 2, outs, sizes([4 + lb, 2 + lb]), 0, None),
             "ntt: null table": lambda: ntt(h, 0, 2, None, sizes([4 + lb, 2 + lb]), 0, None),
             "ntt: null log_n": lambda: ntt(h, 0, 2, outs, None, 0, None),
             "ntt: null entry": lambda: ntt(h, 0, 2, table([o0, 0]), sizes([4 + lb, 2 + lb]), 0, None),
             "ntt: log_n out of range": lambda: ntt(h, 0, 2, outs, sizes([4 + lb, 31]), 0, None),
             "ntt: unknown field": lambda: ntt(h, 7, 2, outs, sizes([4 + lb, 2 + lb]), 0, None),
             "ntt: the same vector twice": lambda: ntt(h, 0, 2, table([o0, o0]), sizes([4 + lb, 2 + lb]), 0, None),
             "ntt: vectors overlap by one row": lambda: ntt(h, 0, 2, table([o0, o1 - 32]), sizes([4 + lb, 2 + lb]), 0, None)}
    for what, fn in cases.items():
        sync(gpu_ctx)
        assert fn() == ERR_INVALID_ARG, what
        sync(gpu_ctx)
        assert (host(buf) == SENTINEL).all(), "%s: something was written" % what
    assert lde(h, 0, 0, None, None, lb, None, None) == 0 and ntt(h, 0, 0, None, None, 0, None) == 0
    sync(gpu_ctx)
    assert (host(buf) == SENTINEL).all()
    gpu_ctx._chk(lde(h, 0, 2, ins, lg, lb, None, outs)); sync(gpu_ctx)     # the context is usable afterwards; adjacent outputs are fine
    same(host(buf)[:N0], oracle.lde(0, host(x), lb), "after the refused calls, column 0")
    same(host(buf)[N0:N0 + N1], oracle.lde(0, host(x)[:4], lb), "after the refused calls, column 1")
    assert (host(buf)[N0 + N1] == SENTINEL).all()


def test_lde_mixed_is_not_slower_than_one_batch_call_per_size(gpu_ctx, oracle):
    """eight columns per size 2^6 .. 2^12, blow-up 3, generator shift: the mixed call against the seven stark_lde_batch_dev calls in the same process,
    warmed, median of five alternations.  Only "not slower" is asserted: the per-size path is the reference; both times and the ratio are reported in
    lde_mixed_batch.json under the directory STARK_TEST_RECORDS names (default: test_records/ in the repository root, ignored by git)."""
    import torch
    lb, per, logs = 3, 8, list(range(6, 13))
    shift = oracle.from_u64(GEN[0], 0)
    lns = [ln for ln in logs for _ in range(per)]
    xs = [dev(oracle.synth_column(0x64C, c, 0, 1 << ln)) for c, ln in enumerate(lns)]
    om = [torch.empty((1 << (ln + lb), 4), dtype=torch.int64, device="cuda") for ln in lns]
    og = [torch.empty((1 << (ln + lb), 4), dtype=torch.int64, device="cuda") for ln in lns]
    ip, mp, gp = [x.data_ptr() for x in xs], [o.data_ptr() for o in om], [o.data_ptr() for o in og]

    def mixed():
        gpu_ctx.lde_mixed_batch_dev(0, ip, lns, lb, mp, shift); gpu_ctx.sync()

    def grouped():
        for k, ln in enumerate(logs):
            gpu_ctx.lde_batch_dev(0, ip[per * k:per * (k + 1)], ln, lb, gp[per * k:per * (k + 1)], shift)
        gpu_ctx.sync()
    mixed(); grouped()                                                     # warms both paths
    assert all((host(a) == host(b)).all() for a, b in zip(om, og))
    tm, tg = [], []
    for _ in range(5):
        t0 = time.perf_counter(); mixed(); tm.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); grouped(); tg.append(time.perf_counter() - t0)
    rec = {"log_n": logs, "columns_per_size": per, "log_blowup": lb, "mixed_ms": 1e3 * statistics.median(tm), "grouped_ms": 1e3 * statistics.median(tg)}
    rec["ratio_grouped_over_mixed"] = rec["grouped_ms"] / rec["mixed_ms"]
    out = os.environ.get("STARK_TEST_RECORDS") or os.path.join(ROOT, "test_records"); os.makedirs(out, exist_ok=True)
    json.dump(rec, open(os.path.join(out, "lde_mixed_batch.json"), "w"), indent=1)
    print(rec)
    assert rec["mixed_ms"] <= rec["grouped_ms"], rec
