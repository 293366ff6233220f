"""The low-degree extension at every blow-up and first-pass route (tests/lde_shapes.py), bit for bit against the CPU oracle.

What the first pass of the big forward transform of `stark_lde` does depends on log_blowup (never-written padding taken as zero in
four different ways, real padding, no padding); the rest of the suite pins it at log_blowup = 3 only.  Here every route runs for
one-, two- and three-pass plans, with the coset pre-scale in its three table forms and at every tile width, through the host and the
device entry point, above the size a full oracle LDE is affordable at, across changes of the cached coset of a plan, and through the
emulated ranks of the sharded LDE (including the blow-up whose shift tables overflow the per-plan table cache).  tests/test_lde_shapes_host.py
proves on the CPU that the shape list reaches every route and that the oracle's LDE is the definition.  Needs an MI355X: `pytest -m gpu`.

Inputs at 2^21 outputs are thinned to keep the single-core oracle affordable (about 1.5 s per LDE of that size): Pallas runs the
synthetic column under every shift and the corner list by index under the generator shift, BLS12-381 one shape per route.  No route
is dropped."""
import ctypes as C

import numpy as np
import pytest

import corner_values as cv
import lde_shapes as ls
import pyref

pytestmark = pytest.mark.gpu

from stark_mlwe_amd.api import StarkError, _ptr

PRIMES = {0: pyref.P_PALLAS, 1: pyref.P_BLS}
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
# {label: {option: (value, value that restores the default)}}: the three forms of the coset pre-scale, the tile widths, the 256-thread launch
OPTIONS = {"ntt_merged_coset = 0 (direct pre-scale table)": {"ntt_merged_coset": (0, 1)}, "ntt_direct_max_log = 0 (two-level lookup)": {"ntt_direct_max_log": (0, 24)},
           "ntt_log_tile = 8": {"ntt_log_tile": (8, -1)}, "ntt_log_tile = 9": {"ntt_log_tile": (9, -1)}, "ntt_log_tile = 12": {"ntt_log_tile": (12, -1)},
           "ntt_min_waves = 4": {"ntt_min_waves": (4, 2)}}


def with_options(ctx, opts, fn):
    """run fn with context options set to `opts` ({key: (value, value to restore)}), restoring them whatever happens"""
    try:
        for k, (v, _) in opts.items():
            ctx.set_option(k, v)
        return fn()
    finally:
        for k, (_, back) in opts.items():
            ctx.set_option(k, back)


def check(got, want, log_n, lb, pre, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size:
        j = int(bad[0]); P, name = ls.route(log_n, lb, pre)
        pytest.fail("%s: shape (log_n = %d, lb = %d), %d-pass route '%s': %d of %d outputs differ from the oracle, first at j = %d (j mod 2^lb = %d, j >> lb = %d)"
                    % (what, log_n, lb, P, name, bad.size, got.shape[0], j, j & ((1 << lb) - 1), j >> lb))


@pytest.fixture(scope="module")
def shifts(oracle):
    """{field: {name: four limbs or None}}: no shift, the explicit one, the multiplicative generator, a shift with all four canonical limbs populated"""
    out = {}
    for field, gen in ((0, 5), (1, 7)):
        full = pow(3, 1000003, PRIMES[field])
        assert all((full >> (64 * i)) & cv.M64 for i in range(4))
        out[field] = {"none": None, "one": oracle.from_u64(1, field), "generator": oracle.from_u64(gen, field), "full-width": oracle.from_int(full, field)}
    return out


def bls_shapes():
    """the first shape of SHAPES on every (passes, route), with and without pre-scale"""
    seen, out = set(), []
    for s in ls.SHAPES:
        keys = {ls.route(s[0], s[1], pre) for pre in (0, 1)}
        if not keys <= seen:
            seen |= keys; out.append(s)
    return out


class Case:
    """One shape: its inputs, and the oracle's LDE computed once per (field, input, shift)."""

    def __init__(self, oracle, shifts, log_n, lb):
        self.o, self.shifts, self.log_n, self.lb, self.big = oracle, shifts, log_n, lb, log_n + lb
        self._in, self._want = {}, {}

    def inputs(self, field, name):
        if (field, name) not in self._in:
            n = 1 << self.log_n
            self._in[(field, name)] = (self.o.synth_column(0x1DE0000 + 64 * self.log_n + self.lb, field, 0, n) if name == "synthetic column"      # below 2^254: both fields
                                       else cv.patterns(PRIMES[field], n)[name])
        return self._in[(field, name)]

    def want(self, field, name, shift):
        key = (field, name, "none" if shift == "one" else shift)       # the explicit one must give the unshifted extension
        if key not in self._want:
            self._want[key] = self.o.lde(field, self.inputs(field, name), self.lb, self.shifts[field][key[2]])
        return self._want[key]

    def legs(self, field):
        """(input name, shift name) pairs of the matrix"""
        if field == 1:
            return [("synthetic column", s) for s in ("none", "generator")]
        out = [("synthetic column", s) for s in ("none", "one", "generator", "full-width")]
        if self.log_n >= 8 and self.big <= 20:
            out += [(name, s) for name in ("corners by index", "all p-1") for s in ("none", "generator", "full-width")]
        elif self.log_n >= 8:
            out += [("corners by index", "generator")]
        return out

    def pre(self, shift):
        return 0 if shift in ("none", "one") else 1

    def run(self, ctx, field, name, shift):
        return ctx.lde(self.inputs(field, name), self.lb, field=field, coset=self.shifts[field][shift])


@pytest.fixture(scope="module", params=ls.SHAPES, ids=lambda s: "logn%d-lb%d" % s)
def case(request, oracle, shifts):
    c = Case(oracle, shifts, *request.param)
    yield c
    c._in.clear(); c._want.clear()


def test_lde_matrix_equals_oracle(gpu_ctx, case):
    """gpu_ctx.lde == oracle.lde on every output: Pallas under no shift, the explicit one (which must give the unshifted extension), the generator and a
    full-width shift, on a synthetic column and (log_n >= 8) on stored-limb corner vectors; BLS12-381 on one shape per route."""
    fields = [0] + ([1] if (case.log_n, case.lb) in bls_shapes() else [])
    for field in fields:
        for name, shift in case.legs(field):
            got = case.run(gpu_ctx, field, name, shift)
            check(got, case.want(field, name, shift), case.log_n, case.lb, case.pre(shift), "field %d, input '%s', shift '%s'" % (field, name, shift))


def test_lde_prescale_forms_and_tiles_equal_oracle(gpu_ctx, case):
    """The coset legs of the shapes whose padding is never written, with the pre-scale read from the direct table, from the two-level lookup, and at
    tile widths 2^8, 2^9, 2^12 and under the 256-thread launch (the tile width C enters the fast route's index arithmetic).  A setting the library
    refuses with "NTT tile exceeds LDS" is accepted for that leg only if the default tile gives the oracle's values, and only for a quarter of the legs
    (pick_log_c shrinks C until the tile fits: none is expected)."""
    if ls.route(case.log_n, case.lb, 1)[1] not in ls.SKIP_COSET:
        return
    legs = [(name, shift) for name, shift in case.legs(0) if case.pre(shift)]
    assert ("synthetic column", "generator") in legs and ("synthetic column", "full-width") in legs
    total = refused = 0
    for label, opts in OPTIONS.items():
        for name, shift in legs:
            what = "%s, input '%s', shift '%s'" % (label, name, shift)
            total += 1
            try:
                got = with_options(gpu_ctx, opts, lambda: case.run(gpu_ctx, 0, name, shift))
            except StarkError as e:
                assert e.code == ERR_UNSUPPORTED and "NTT tile exceeds LDS" in str(e), what
                refused += 1
                check(case.run(gpu_ctx, 0, name, shift), case.want(0, name, shift), case.log_n, case.lb, 1, "default options after a refused '%s'" % what)
                continue
            check(got, case.want(0, name, shift), case.log_n, case.lb, 1, what)
    assert 4 * refused <= total, "%d of %d option legs refused as unsupported" % (refused, total)


SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.mark.parametrize("log_n,lb", [(8, 2), (12, 4), (17, 4)])
def test_lde_dev_writes_all_of_out_and_nothing_else(gpu_ctx, oracle, shifts, log_n, lb):
    """stark_lde_dev on device buffers, one shape per pass count: the skip routes never touch out[n..N) before the transform, so `out` starts as a
    sentinel pattern; one sentinel row in front and one behind must survive, every row of out equals the oracle, the input is unchanged."""
    import torch
    n, N = 1 << log_n, 1 << (log_n + lb)
    assert ls.passes(log_n, lb) == {8: 1, 12: 2, 17: 3}[log_n]
    ev = oracle.synth_column(0xDE7 + log_n, 3, 0, n)
    x = torch.from_numpy(ev.view(np.int64).copy()).cuda()
    for shift in ("none", "generator"):
        buf = torch.full((N + 2, 4), SENTINEL, dtype=torch.int64, device="cuda")
        out = buf[1:N + 1]
        assert out.data_ptr() == buf.data_ptr() + 32
        torch.cuda.synchronize()
        gpu_ctx._chk(gpu_ctx.lib.stark_lde_dev(gpu_ctx.h, 0, C.c_void_p(x.data_ptr()), log_n, lb, _ptr(shifts[0][shift]), C.c_void_p(out.data_ptr())))
        gpu_ctx.sync(); torch.cuda.synchronize()
        host = buf.cpu().numpy().view(np.uint64)
        assert (host[0] == SENTINEL).all() and (host[N + 1] == SENTINEL).all(), (log_n, lb, shift, "a row outside out[0, N) was written")
        check(host[1:N + 1], oracle.lde(0, ev, lb, shifts[0][shift]), log_n, lb, shift != "none", "stark_lde_dev, shift '%s'" % shift)
        assert (x.cpu().numpy().view(np.uint64) == ev).all()
    del buf, out, x


@pytest.mark.parametrize("log_n,lb", [(20, 4), (18, 6)])
def test_lde_2pow24_zero_group_route_against_horner_and_inverse(gpu_ctx, oracle, shifts, log_n, lb):
    """Three-pass zero-group route above the size of a full oracle LDE.  (i) no shift: the extension restricted to the original domain is the input.
    (ii) generator shift: sampled outputs — 1024 random ones, the ends, the middle, one of every residue class mod 2^lb — equal the Horner evaluation of
    the interpolating polynomial (coefficients from the ORACLE's inverse NTT).  (iii) the inverse coset transform of the whole extension has the oracle's
    coefficients in [0, n) and exact zero limbs in [n, N)."""
    assert ls.route(log_n, lb, 1) == (3, ls.FAST_ZERO)
    n, N, b = 1 << log_n, 1 << (log_n + lb), 1 << lb
    ev = oracle.synth_column(0x24000 + log_n, 1, 0, n)
    out1 = gpu_ctx.lde(ev, lb, field=0)
    bad = np.nonzero((out1[::b] != ev).any(axis=1))[0]
    assert bad.size == 0, "no shift: out[%d * 2^%d] differs from evals[%d]" % (bad[0], lb, bad[0])
    g = shifts[0]["generator"]
    out = gpu_ctx.lde(ev, lb, field=0, coset=g)
    coeffs = oracle.ntt(0, ev, inverse=True)
    rng = np.random.default_rng(log_n)
    idx = np.unique(np.concatenate([[0, 1, N - 1, N // 2], rng.integers(0, N, 1024), np.arange(b) + b * rng.integers(0, n, b)]))
    assert set(int(i) % b for i in idx) == set(range(b))
    wN = oracle.root_of_unity(log_n + lb)
    for o, sh, what in ((out, g, "generator shift"), (out1, None, "no shift")):
        pts = np.stack([oracle.pow(wN, int(i)) if sh is None else oracle.mul(sh, oracle.pow(wN, int(i))) for i in idx])
        bad = np.nonzero((o[idx] != oracle.poly_eval_many(0, coeffs, pts)).any(axis=1))[0]
        assert bad.size == 0, "%s: output j = %d (j mod 2^lb = %d, j >> lb = %d) differs from Horner" % (what, idx[bad[0]], idx[bad[0]] % b, idx[bad[0]] >> lb)
    del out1
    back = gpu_ctx.ifft(out, field=0, coset=g)
    assert (back[:n] == coeffs).all()
    assert not back[n:].any(), "non-zero coefficient at index %d" % (n + int(np.nonzero(back[n:].any(axis=1))[0][0]))
    del back, out; gpu_ctx.trim()


@pytest.mark.parametrize("s,lde_shape", [(10, (6, 4)), (14, (10, 4)), (21, (17, 4))])
def test_coset_cache_across_changes_of_coset(gpu_ctx, oracle, shifts, s, lde_shape):
    """A plan caches the tables of ONE coset and rebuilds them on a change; the LDE shares the forward plan of its output size with plain transforms.
    On one context and one size per pass count: forward coset transforms with g1, g2, g1, none, g1, an LDE of that output size with g2, the forward
    transform with g1 again, the inverse coset transform with g2 then g1 — every result against the oracle; then the same under ntt_merged_coset = 0."""
    assert sum(lde_shape) == s and len(ls.split(s)) == {10: 1, 14: 2, 21: 3}[s]
    g = {"g1": shifts[0]["generator"], "g2": shifts[0]["full-width"], "none": None}
    x = oracle.synth_column(0xC05E7 + s, 2, 0, 1 << s); ev = x[:1 << lde_shape[0]]
    want = {}

    def ref(kind, k):
        if (kind, k) not in want:
            want[(kind, k)] = (oracle.lde(0, ev, lde_shape[1], g[k]) if kind == "lde" else oracle.ntt(0, x, inverse=kind == "ifft", coset=g[k]))
        return want[(kind, k)]

    def sequence(tag):
        steps = [("fft", k) for k in ("g1", "g2", "g1", "none", "g1")] + [("lde", "g2"), ("fft", "g1"), ("ifft", "g2"), ("ifft", "g1")]
        for i, (kind, k) in enumerate(steps):
            got = (gpu_ctx.lde(ev, lde_shape[1], field=0, coset=g[k]) if kind == "lde" else
                   gpu_ctx.fft(x, field=0, coset=g[k]) if kind == "fft" else gpu_ctx.ifft(x, field=0, coset=g[k]))
            bad = np.nonzero((got != ref(kind, k)).any(axis=1))[0]
            assert bad.size == 0, "%s, step %d (%s with %s) at 2^%d: first differing index %d" % (tag, i, kind, k, s, bad[0])

    sequence("default tables")
    with_options(gpu_ctx, {"ntt_merged_coset": (0, 1)}, lambda: sequence("ntt_merged_coset = 0"))


# ---- emulated ranks of the sharded LDE --------------------------------------------------------------------------------------------------
def emulated(ctx, field, W, x_dev, log_n, lb, shift):
    import torch
    a = torch.empty(((1 << log_n) << lb, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx._chk(ctx.lib.stark_diag_lde_sharded_emulated_dev(ctx.h, field, W, C.c_void_p(x_dev.data_ptr()), log_n, lb, _ptr(shift), C.c_void_p(a.data_ptr())))
    ctx.sync(); torch.cuda.synchronize()
    return a.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,lb", [(12, 0), (13, 1), (16, 4), (11, 5), (14, 6), (8, 6)])
def test_sharded_lde_emulated_ranks_equal_oracle(gpu_ctx, oracle, shifts, field, log_n, lb):
    """stark_diag_lde_sharded_emulated_dev (the phase code of stark_lde_sharded_dev for W virtual ranks on one GPU) against the ORACLE's LDE, W = 2, 4, 8,
    both fields, generator and full-width shift, blow-ups the suite never sharded.  At lb = 6 every rank asks for 64 shift tables plus the root table, more
    than the plan's 40-entry table FIFO holds: the eviction branch runs, and the call is repeated on the same context."""
    import torch
    ev = oracle.synth_column(0xE301 + log_n, lb, 0, 1 << log_n)                # stored values below 2^254: elements of both fields
    x = torch.from_numpy(ev.view(np.int64).copy()).cuda()
    for sname in ("generator", "full-width"):
        sh = shifts[field][sname]
        want = oracle.lde(field, ev, lb, sh)
        for W in (2, 4, 8):
            for rep in range(2 if lb == 6 else 1):
                got = emulated(gpu_ctx, field, W, x, log_n, lb, sh)
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert bad.size == 0, "field %d, W = %d, (log_n = %d, lb = %d), shift '%s', run %d: %d outputs differ, first at j = %d (j mod 2^lb = %d, j >> lb = %d)" % (
                    field, W, log_n, lb, sname, rep, bad.size, bad[0], bad[0] & ((1 << lb) - 1), bad[0] >> lb)
    del x; gpu_ctx.trim()


def test_sharded_lde_emulated_invalid_rank_counts_leave_the_context_usable(gpu_ctx, oracle, shifts):
    import torch
    sh = shifts[0]["generator"]
    ev = oracle.synth_column(0xE3FF, 0, 0, 1 << 6)
    x = torch.from_numpy(ev.view(np.int64).copy()).cuda()
    for W, log_n in ((4, 2), (2, 1), (4, 1)):          # 2^2 is viewed as 2 x 2: four ranks do not divide it; log_n = 1 is below the smallest view
        with pytest.raises(StarkError) as e:
            emulated(gpu_ctx, 0, W, x, log_n, 1, sh)
        assert e.value.code == ERR_INVALID_ARG, (W, log_n)
        assert (emulated(gpu_ctx, 0, 2, x, 6, 4, sh) == oracle.lde(0, ev, 4, sh)).all(), (W, log_n)


# ---- the Python wrapper ----------------------------------------------------------------------------------------------------------------------
def test_lde_wrapper_rejects_lengths_that_are_not_powers_of_two(gpu_ctx, oracle):
    ev = oracle.synth_column(0x1DE, 0, 0, 1024)
    with pytest.raises(StarkError):
        gpu_ctx.lde(ev[:1000], 3)
    with pytest.raises(StarkError):
        gpu_ctx.lde(np.zeros((0, 4), np.uint64), 3)
    with pytest.raises(StarkError):
        gpu_ctx.fft(ev[:1000])
    one = gpu_ctx.lde(ev[:1], 3)                        # a constant: eight copies
    assert one.shape == (8, 4) and (one == ev[0]).all()
    assert (gpu_ctx.lde(ev, 3) == oracle.lde(0, ev, 3)).all()
