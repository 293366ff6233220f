"""stark_lde_batch_dev / stark_ntt_batch_dev: many columns of one shape and one coset in one device pass.  Column i of every result must equal, bit
for bit, the CPU oracle and what the single call (stark_lde_dev / stark_ntt_dev) gives for that column alone — on every first-pass route of the big
forward transform (tests/lde_shapes.py), for one-, two- and three-pass plans, under every NTT option, across pass cuts and changes of the cached coset,
with corner inputs, repeated and aliased pointers, between guard bands, and for every refused argument.  Needs an MI355X: `pytest -m gpu`."""
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
from test_gpu_guard_bands import Band, SENTINEL, guarded, hp, same, sync
from test_gpu_lde_blowups import OPTIONS, bls_shapes, with_options

pytestmark = pytest.mark.gpu

from stark_mlwe_amd.api import _ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIMES = {0: pyref.P_PALLAS, 1: pyref.P_BLS}
GEN = {0: 5, 1: 7}
ERR_INVALID_ARG = -1
DEFAULT_MAX_ELEMS = 1 << 24
# (log_n, lb): the smallest shape on every route and pass count (the routes are asserted below), and one three-pass shape
SHAPES = [(0, 3), (3, 0), (8, 2), (4, 7), (8, 3), (7, 4), (5, 6), (10, 1), (11, 0), (18, 3)]
BIG = (18, 3)


def test_shape_list_reaches_every_route():
    names = {ls.route(log_n, lb, pre)[1] for log_n, lb in SHAPES for pre in (0, 1)}
    assert names == {ls.NO_EXTENSION, ls.PADDED, ls.FAST, ls.FAST_ZERO, ls.FAST_ZERO_ONE, ls.GENERAL, ls.UNIT}
    keys = {ls.route(log_n, lb, pre) for log_n, lb in SHAPES for pre in (0, 1)}
    assert {(1, ls.PADDED), (2, ls.PADDED), (1, ls.NO_EXTENSION), (2, ls.NO_EXTENSION)} <= keys and any(P == 3 for P, _ in keys)
    assert ls.route(8, 3, 1) == (2, ls.FAST) and ls.route(4, 7, 1) == (2, ls.PADDED)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def table(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*[int(p) for p in ptrs])


def shift_of(oracle, field, name):
    return None if name == "none" else oracle.from_u64(GEN[field], field)


def lde_batch(ctx, field, xs, log_n, lb, shift, prefill=SENTINEL):
    """stark_lde_batch_dev on the device columns xs -> list of host results (outputs start as a sentinel pattern: the skip routes never pad)"""
    import torch
    outs = [torch.full((1 << (log_n + lb), 4), prefill, dtype=torch.int64, device="cuda") for _ in xs]
    sync(ctx)
    ctx.lde_batch_dev(field, [x.data_ptr() for x in xs], log_n, lb, [o.data_ptr() for o in outs], shift)
    sync(ctx)
    return [host(o) for o in outs]


def lde_single(ctx, field, x, log_n, lb, shift):
    import torch
    out = torch.full((1 << (log_n + lb), 4), SENTINEL, dtype=torch.int64, device="cuda")
    sync(ctx)
    ctx._chk(ctx.lib.stark_lde_dev(ctx.h, field, C.c_void_p(x.data_ptr()), log_n, lb, _ptr(shift), C.c_void_p(out.data_ptr())))
    sync(ctx)
    return host(out)


@pytest.fixture(scope="module")
def columns(oracle):
    """(field, log_n, lb, column, shift name) -> (input, oracle LDE), computed once and shared by the tests of this module"""
    memo = {}

    def get(field, log_n, lb, c, sname):
        key = (field, log_n, lb, c, sname)
        if key not in memo:
            x = oracle.synth_column(0xBA7C000 + 64 * log_n + lb, c, 0, 1 << log_n)          # stored values below 2^254: elements of both fields
            memo[key] = (x, oracle.lde(field, x, lb, shift_of(oracle, field, sname)))
        return memo[key]
    return get


@pytest.mark.parametrize("log_n,lb", SHAPES, ids=lambda v: str(v))
def test_lde_batch_every_route_equals_oracle_and_single_call(gpu_ctx, oracle, columns, log_n, lb):
    """B = 1, 2, 5 (the three-pass shape: B = 2, Pallas) under no shift and the generator: every column against oracle.lde and stark_lde_dev; the inputs stay intact"""
    fields = [0] + ([1] if (log_n, lb) in bls_shapes() and (log_n, lb) != BIG else [])
    for field in fields:
        for sname in ("none", "generator"):
            shift = shift_of(oracle, field, sname)
            nb = 2 if (log_n, lb) == BIG else 5
            ins = [columns(field, log_n, lb, c, sname) for c in range(nb)]
            xs = [dev(x) for x, _ in ins]
            single = [lde_single(gpu_ctx, field, x, log_n, lb, shift) for x in xs]
            for B in ((2,) if (log_n, lb) == BIG else (1, 2, 5)):
                got = lde_batch(gpu_ctx, field, xs[:B], log_n, lb, shift)
                for c in range(B):
                    what = "field %d, (log_n = %d, lb = %d), %d-pass route '%s', shift '%s', B = %d, column %d" % ((field, log_n, lb) + ls.route(log_n, lb, sname != "none") + (sname, B, c))
                    same(got[c], ins[c][1], what + " against the oracle")
                    same(got[c], single[c], what + " against stark_lde_dev")
            for x, (xin, _) in zip(xs, ins):
                assert (host(x) == xin).all(), "an input was modified"
            del xs


@pytest.mark.parametrize("lb", [0, 3])
def test_lde_batch_corners_repeated_and_aliased_pointers(gpu_ctx, oracle, columns, lb):
    """(8, lb), generator shift, four columns: the stored-limb corner list, one input pointer used twice, and a column whose output buffer starts as its input"""
    import torch
    log_n, n, N = 8, 1 << 8, 1 << (8 + lb)
    shift = shift_of(oracle, 0, "generator")
    corners = cv.patterns(PRIMES[0], n)["corners by index"]
    x1, w1 = columns(0, log_n, lb, 0, "generator")
    x3, w3 = columns(0, log_n, lb, 1, "generator")
    d0, d1 = dev(corners), dev(x1)
    outs = [torch.full((N, 4), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(4)]
    outs[3][:n] = dev(x3)                                                  # column 3: evals == out
    sync(gpu_ctx)
    gpu_ctx.lde_batch_dev(0, [d0.data_ptr(), d1.data_ptr(), d1.data_ptr(), outs[3].data_ptr()], log_n, lb, [o.data_ptr() for o in outs], shift)
    sync(gpu_ctx)
    for c, want in enumerate((oracle.lde(0, corners, lb, shift), w1, w1, w3)):
        same(host(outs[c]), want, "lb = %d, column %d" % (lb, c))
    assert (host(d0) == corners).all() and (host(d1) == x1).all(), "an input that aliases no output was modified"


def test_lde_batch_pass_cutting_on_the_device(gpu_ctx, oracle, columns):
    """B = 5 at (8, 3) with passes of at most two columns: 2 / 2 / 1, the last one through the single path"""
    log_n, lb = 8, 3
    shift = shift_of(oracle, 0, "generator")
    ins = [columns(0, log_n, lb, c, "generator") for c in range(5)]
    xs = [dev(x) for x, _ in ins]
    gpu_ctx.set_option("ntt_batch_max_elems", 2 << (log_n + lb))
    try:
        got = lde_batch(gpu_ctx, 0, xs, log_n, lb, shift)
    finally:
        gpu_ctx.set_option("ntt_batch_max_elems", DEFAULT_MAX_ELEMS)
    for c in range(5):
        same(got[c], ins[c][1], "passes 2 / 2 / 1, column %d" % c)
    cols = [oracle.synth_column(0x9A55, c, 0, 1 << 11) for c in range(3)]
    ys = [dev(x) for x in cols]
    gpu_ctx.set_option("ntt_batch_max_elems", 2 << 11)                    # the transforms: 2 / 1
    try:
        gpu_ctx.ntt_batch_dev(0, [y.data_ptr() for y in ys], 11, False, shift); sync(gpu_ctx)
    finally:
        gpu_ctx.set_option("ntt_batch_max_elems", DEFAULT_MAX_ELEMS)
    for c in range(3):
        same(host(ys[c]), oracle.ntt(0, cols[c], inverse=False, coset=shift), "transform passes 2 / 1, column %d" % c)
    for bad in (0, (1 << 28) + 1):
        with pytest.raises(Exception) as e:
            gpu_ctx.set_option("ntt_batch_max_elems", bad)
        assert "1..2^28" in str(e.value)
    with pytest.raises(Exception) as e:
        gpu_ctx.set_option("ntt_batch_max_elements", 1)
    assert "ntt_batch_max_elems" in str(e.value)
    same(lde_batch(gpu_ctx, 0, xs[:2], log_n, lb, shift)[1], ins[1][1], "after the refused options")


def test_lde_batch_option_matrix(gpu_ctx, oracle, columns):
    """(8, 3), B = 3, generator shift under every pre-scale form, tile width and launch shape of the single call's option matrix"""
    log_n, lb = 8, 3
    shift = shift_of(oracle, 0, "generator")
    ins = [columns(0, log_n, lb, c, "generator") for c in range(3)]
    xs = [dev(x) for x, _ in ins]
    for label, opts in OPTIONS.items():
        got = with_options(gpu_ctx, opts, lambda: lde_batch(gpu_ctx, 0, xs, log_n, lb, shift))
        for c in range(3):
            same(got[c], ins[c][1], "%s, column %d" % (label, c))


def test_lde_batch_coset_cache_across_changes_of_coset(gpu_ctx, oracle, columns):
    """batch with shift A, single call with shift B, batch with shift A again: the plan's one cached coset changes under both paths"""
    log_n, lb = 8, 3
    A = shift_of(oracle, 0, "generator"); Bs = oracle.from_int(pow(3, 1000003, PRIMES[0]), 0)
    ins = [columns(0, log_n, lb, c, "generator") for c in range(3)]
    xs = [dev(x) for x, _ in ins]
    first = lde_batch(gpu_ctx, 0, xs, log_n, lb, A)
    same(lde_single(gpu_ctx, 0, xs[0], log_n, lb, Bs), oracle.lde(0, ins[0][0], lb, Bs), "single call with the second shift")
    again = lde_batch(gpu_ctx, 0, xs, log_n, lb, A)
    for c in range(3):
        same(first[c], ins[c][1], "first batch, column %d" % c); same(again[c], ins[c][1], "batch after the coset changed, column %d" % c)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n", [0, 1, 3, 10, 11, 12])
def test_ntt_batch_equals_oracle_and_single_call(gpu_ctx, oracle, field, log_n):
    """stark_ntt_batch_dev, B = 3, forward and inverse, with and without coset, against oracle.ntt and stark_ntt_dev"""
    B, n = 3, 1 << log_n
    cols = [oracle.synth_column(0x177B + log_n, c, 0, n) for c in range(B)]
    for inverse in (False, True):
        for coset in (None, oracle.from_u64(GEN[field], field)):
            xs = [dev(x) for x in cols]; ys = [dev(x) for x in cols]
            sync(gpu_ctx)
            gpu_ctx.ntt_batch_dev(field, [x.data_ptr() for x in xs], log_n, inverse, coset)
            for y in ys:
                gpu_ctx._chk(gpu_ctx.lib.stark_ntt_dev(gpu_ctx.h, field, C.c_void_p(y.data_ptr()), log_n, int(inverse), _ptr(coset)))
            sync(gpu_ctx)
            for c in range(B):
                what = "field %d, 2^%d, inverse %d, coset %s, column %d" % (field, log_n, inverse, coset is not None, c)
                same(host(xs[c]), oracle.ntt(field, cols[c], inverse=inverse, coset=coset), what + " against the oracle")
                same(host(xs[c]), host(ys[c]), what + " against stark_ntt_dev")


@pytest.mark.parametrize("log_n,lb", [(8, 3), (4, 7)])
def test_lde_batch_between_guard_bands(gpu_ctx, oracle, columns, log_n, lb):
    """B = 3, every buffer between sentinel bands: nothing outside the outputs is written, the inputs stay intact, the result does not depend on what out held"""
    ins = [columns(0, log_n, lb, c, "generator") for c in range(3)]
    shift = shift_of(oracle, 0, "generator")

    def call(inb, ob, pre):
        return gpu_ctx.lib.stark_lde_batch_dev(gpu_ctx.h, 0, 3, table([b.ptr().value for b in inb]), log_n, lb, hp(shift), table([ob.ptr(i).value for i in range(3)]))
    guarded(gpu_ctx, [x for x, _ in ins], [1 << (log_n + lb)] * 3, call, [w for _, w in ins], "stark_lde_batch_dev (log_n = %d, lb = %d)" % (log_n, lb))


def test_ntt_batch_between_guard_bands(gpu_ctx, oracle):
    """three 2^11-point vectors one sentinel row apart, transformed in place on the generator's coset"""
    log_n = 11; coset = oracle.from_u64(GEN[0], 0)
    cols = [oracle.synth_column(0x6B11, c, 0, 1 << log_n) for c in range(3)]
    b = Band(cols)
    sync(gpu_ctx)
    gpu_ctx._chk(gpu_ctx.lib.stark_ntt_batch_dev(gpu_ctx.h, 0, 3, table([b.ptr(i).value for i in range(3)]), log_n, 0, hp(coset)))
    sync(gpu_ctx)
    h = b.host(); b.check("stark_ntt_batch_dev", h)
    for c in range(3):
        same(b.payload(c, h), oracle.ntt(0, cols[c], inverse=False, coset=coset), "stark_ntt_batch_dev between bands, column %d" % c)


def test_batch_calls_refuse_bad_arguments_before_any_launch(gpu_ctx, oracle):
    """every STARK_ERR_INVALID_ARG case of the header comment: the outputs keep their pre-fill; batch == 0 is STARK_OK"""
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.h
    log_n, lb = 4, 2; n, N = 1 << log_n, 1 << (log_n + lb)
    x = dev(oracle.synth_column(0xE44, 0, 0, n))
    buf = torch.full((2 * N + 1, 4), SENTINEL, dtype=torch.int64, device="cuda")
    o0, o1 = buf.data_ptr(), buf.data_ptr() + 32 * N
    ins, outs = table([x.data_ptr(), x.data_ptr()]), table([o0, o1])
    cases = {"null ctx": lambda: lib.stark_lde_batch_dev(None, 0, 2, ins, log_n, lb, None, outs),
             "null input table": lambda: lib.stark_lde_batch_dev(h, 0, 2, None, log_n, lb, None, outs),
             "null output table": lambda: lib.stark_lde_batch_dev(h, 0, 2, ins, log_n, lb, None, None),
             "null input entry": lambda: lib.stark_lde_batch_dev(h, 0, 2, table([x.data_ptr(), 0]), log_n, lb, None, outs),
             "null output entry": lambda: lib.stark_lde_batch_dev(h, 0, 2, ins, log_n, lb, None, table([o0, 0])),
             "log_n out of range": lambda: lib.stark_lde_batch_dev(h, 0, 2, ins, 31, 0, None, outs),
             "log_n + log_blowup out of range": lambda: lib.stark_lde_batch_dev(h, 0, 2, ins, log_n, 31 - log_n, None, outs),
             "unknown field": lambda: lib.stark_lde_batch_dev(h, 7, 2, ins, log_n, lb, None, outs),
             "the same output twice": lambda: lib.stark_lde_batch_dev(h, 0, 2, ins, log_n, lb, None, table([o0, o0])),
             "outputs overlap by one row": lambda: lib.stark_lde_batch_dev(h, 0, 2, ins, log_n, lb, None, table([o0 + 32, o1])),
             "ntt: null ctx": lambda: lib.stark_ntt_batch_dev(None, 0, 2, outs, log_n + lb, 0, None),
             "ntt: null table": lambda: lib.stark_ntt_batch_dev(h, 0, 2, None, log_n + lb, 0, None),
             "ntt: null entry": lambda: lib.stark_ntt_batch_dev(h, 0, 2, table([o0, 0]), log_n + lb, 0, None),
             "ntt: log_n out of range": lambda: lib.stark_ntt_batch_dev(h, 0, 2, outs, 31, 0, None),
             "ntt: unknown field": lambda: lib.stark_ntt_batch_dev(h, 7, 2, outs, log_n + lb, 0, None),
             "ntt: the same vector twice": lambda: lib.stark_ntt_batch_dev(h, 0, 2, table([o0, o0]), log_n + lb, 0, None),
             "ntt: vectors overlap": lambda: lib.stark_ntt_batch_dev(h, 0, 2, table([o0, o1 - 32]), log_n + lb, 0, None)}
    for what, fn in cases.items():
        sync(gpu_ctx)
        assert fn() == ERR_INVALID_ARG, what
        sync(gpu_ctx)
        assert (host(buf) == SENTINEL).all(), "%s: something was written" % what
    assert lib.stark_lde_batch_dev(h, 0, 0, None, log_n, lb, None, None) == 0
    assert lib.stark_ntt_batch_dev(h, 0, 0, None, log_n, 0, None) == 0
    sync(gpu_ctx)
    assert (host(buf) == SENTINEL).all()
    want = oracle.lde(0, host(x), lb)                                       # the context is usable afterwards
    gpu_ctx._chk(lib.stark_lde_batch_dev(h, 0, 2, ins, log_n, lb, None, outs)); sync(gpu_ctx)
    same(host(buf)[:N], want, "after the refused calls, column 0"); same(host(buf)[N:2 * N], want, "after the refused calls, column 1")
    assert (host(buf)[2 * N] == SENTINEL).all()


def test_lde_batch_is_not_slower_than_single_calls(gpu_ctx, oracle):
    """(8, 3), B = 64 (sixteen four-column traces at n0 = 2^11): the batch call against 64 single calls in the same process, warmed, median of five
    alternations.  Only "not slower" is asserted: the single path is the reference; the ratio is reported in lde_batch.json under the directory
    STARK_TEST_RECORDS names (default: test_records/ in the repository root, ignored by git)."""
    import torch
    log_n, lb, B = 8, 3, 64; n, N = 1 << log_n, 1 << (log_n + lb)
    shift = oracle.from_u64(GEN[0], 0)
    xs = [dev(oracle.synth_column(0x64B, c, 0, n)) for c in range(B)]
    ob = [torch.empty((N, 4), dtype=torch.int64, device="cuda") for _ in range(B)]
    os_ = [torch.empty((N, 4), dtype=torch.int64, device="cuda") for _ in range(B)]
    ip, bp, sp = [x.data_ptr() for x in xs], [o.data_ptr() for o in ob], [o.data_ptr() for o in os_]
    lib, h, sh = gpu_ctx.lib, gpu_ctx.h, _ptr(shift)

    def batch():
        gpu_ctx.lde_batch_dev(0, ip, log_n, lb, bp, shift); gpu_ctx.sync()

    def singles():
        for i, o in zip(ip, sp):
            gpu_ctx._chk(lib.stark_lde_dev(h, 0, C.c_void_p(i), log_n, lb, sh, C.c_void_p(o)))
        gpu_ctx.sync()
    batch(); singles()                                                     # warms both paths
    assert all((host(a) == host(b)).all() for a, b in zip(ob, os_))
    tb, ts = [], []
    for _ in range(5):
        t0 = time.perf_counter(); batch(); tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); singles(); ts.append(time.perf_counter() - t0)
    rec = {"log_n": log_n, "log_blowup": lb, "batch": B, "batch_ms": 1e3 * statistics.median(tb), "singles_ms": 1e3 * statistics.median(ts)}
    rec["ratio_singles_over_batch"] = rec["singles_ms"] / rec["batch_ms"]
    out = os.environ.get("STARK_TEST_RECORDS") or os.path.join(ROOT, "test_records"); os.makedirs(out, exist_ok=True)
    json.dump(rec, open(os.path.join(out, "lde_batch.json"), "w"), indent=1)
    print(rec)
    assert rec["batch_ms"] <= rec["singles_ms"], rec
