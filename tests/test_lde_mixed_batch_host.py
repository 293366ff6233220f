"""stark_ntt_mixed_batch_dev / stark_lde_mixed_batch_dev without a device: the two symbols in the header, the ctypes table and the Rust declarations,
and the host-only rules of csrc/ntt_mixed_plan.hpp through libstark_mlwe_hostcheck.so — the tile lookup the kernels run, the launch plan of a pass
against a plain-Python restatement, the pass cutting with a length per column and the overlap check of ranges of different lengths.  CPU only."""
import ctypes as C
import itertools
import os
import re

import numpy as np

import hostcheck_lib
import lde_shapes as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"stark_ntt_mixed_batch_dev": 7, "stark_lde_mixed_batch_dev": 8}
IN, OUT, SCRATCH = 0, 1, 2
INVERSE, PAD, FORWARD = 0, 1, 2
PAD_BLOCK = 256
MAX_LDS = 160 * 1024
SIZES = (0, 1, 3, 10, 11, 12, 20, 21)


def test_mixed_symbols_in_header_ctypes_table_and_rust_declarations():
    from stark_mlwe_amd._abi import SIGNATURES
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stark_mlwe.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "rust", "stark-mlwe-hip", "src", "ffi.rs")).read()
    for name, arity in ARITY.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, "%s is not declared in include/stark_mlwe.h" % name
        assert len(m.group(1).split(",")) == arity, name
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == arity and SIGNATURES[name][0] is C.c_int32, name
        r = re.search(r"pub fn %s\(([^)]*)\) -> i32;" % name, ffi)
        assert r and len(r.group(1).split(",")) == arity, name
    lib_rs = open(os.path.join(ROOT, "rust", "stark-mlwe-hip", "src", "lib.rs")).read()
    assert "stark_lde_mixed_batch_dev(" in lib_rs and "stark_ntt_mixed_batch_dev(" in lib_rs, "no wrapper in lib.rs"
    from stark_mlwe_amd.api import Context
    assert callable(Context.ntt_mixed_batch_dev) and callable(Context.lde_mixed_batch_dev)


# ---- tile lookup ------------------------------------------------------------------------------------------------------------------------------
def test_tile_lookup_equals_a_linear_scan_for_every_tile():
    lib = C.CDLL(hostcheck_lib.PATH)
    lib.hc_ntt_ragged_locate.restype = C.c_uint32
    rng = np.random.default_rng(0x7113)
    lists = [[1], [5000], [1] * 17, [1, 4096, 2048], [4096, 2048, 1], [3000, 1, 3000], [1] * 1000,
             list(rng.integers(1, 40, 1000)), list(rng.integers(1, 9, 33)), [2, 1], [1, 2]]
    lists += [list(rng.integers(1, 200, int(k))) for k in rng.integers(1, 64, 20)]
    for counts in lists:
        first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)
        total = int(np.sum(counts))
        want = np.repeat(np.arange(len(counts)), counts)                       # the linear scan: tile t belongs to the column whose run covers it
        p = first.ctypes.data_as(C.c_void_p)
        for t in range(total):
            c = lib.hc_ntt_ragged_locate(p, C.c_uint32(len(counts)), C.c_uint32(t))
            assert c == want[t] and first[c] <= t < first[c] + counts[c], (counts[:8], t, c)


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------------
def lds_bytes(log_b, log_c):
    E, NT = 1 << (log_b + log_c), (1 << (log_b - 1)) if log_b > 0 else 1
    return (((9 * E + 3) & ~3) + ((9 * NT + 3) & ~3)) * 4


def pick_log_c(log_b, cap, total_log, log_tile=11, forced=False):
    le = log_tile
    if not forced and total_log - le < 9:
        le = max(8, min(le, total_log - 8))
    lc = max(0, min(max(2, le - log_b), cap))
    while lc > 0 and lds_bytes(log_b, lc) > MAX_LDS:
        lc -= 1
    return lc


def ref_transforms(kind, items, pre_first):
    """items: (col, log_n, log_nonzero, src, dst, work offset).  Passes aligned at the end: pass j of a P-pass transform runs in step 3 - P + j; a step is
    one launch per (strided, pre) form; larger tiles first."""
    out = []
    for step in range(3):
        for pre in (False, True):
            mem = []
            for it in items:
                b = ls.split(it[1]); j = step - (3 - len(b))
                if j >= 0 and (pre_first and j == 0) == pre:
                    mem.append((it, b, j))
            if not mem:
                continue
            total_log = sum(1 << it[1] for it, _, _ in mem).bit_length() - 1
            strided = step < 2
            ent = []
            for it, b, j in mem:
                col, log_n, lnz, src, dst, work = it
                P, log_b, log_m = len(b), b[j], log_n - sum(b[:j])
                log_c = pick_log_c(log_b, log_m - log_b, total_log) if strided else (0 if P == 1 else pick_log_c(log_b, b[0], total_log))
                nz = strided and j == 0 and 0 <= lnz < log_n and lnz >= log_m - log_b
                shape = (log_n, P, j, log_b, log_c, log_m, lnz if nz else -1, (1 << log_n) >> (log_b + log_c))
                ent.append((shape, col, src if j == 0 else (SCRATCH, work), dst if j == P - 1 else (SCRATCH, work)))
            ent.sort(key=lambda e: -(e[0][3] + e[0][4]))                       # stable
            shapes, cols, ntiles = [], [], 0
            for shape, col, src, dst in ent:
                if shape not in shapes:
                    shapes.append(shape)
                cols.append((col, shapes.index(shape), ntiles) + src + dst + (0, 0, 0)); ntiles += shape[7]
            out.append(((kind, step, int(strided), int(pre), ntiles, max(lds_bytes(s[3], s[4]) for s in shapes)), shapes, cols))
    return out


def skips(log_n, lb):
    b = ls.split(log_n + lb)
    return lb > 0 and len(b) > 1 and log_n + lb - b[0] <= log_n


def ref_plan(log_ns, lde, inverse, coset, lb):
    if not lde:
        items, scratch = [], 0
        for i, ln in enumerate(log_ns):
            if ln:
                items.append((i, ln, -1, (IN, 0), (OUT, 0), scratch)); scratch += (1 << ln) if ln > 10 else 0
        return scratch, ref_transforms(INVERSE if inverse else FORWARD, items, coset and not inverse)
    inv, fwd, pad, scratch, ptiles = [], [], [], 0, 0
    for i, ln in enumerate(log_ns):
        n, N = 1 << ln, 1 << (ln + lb)
        X, Cs = scratch, scratch + N; scratch += N + n
        skip = skips(ln, lb); coef = (SCRATCH, Cs if skip else X)
        if ln:
            inv.append((i, ln, -1, (IN, 0), coef, X if skip else Cs))
        if ln == 0 or (N > n and not skip):
            first, head = (0, 1) if ln == 0 else (n, 0)
            src, dst = ((IN, 0), (OUT, 0) if ln + lb == 0 else coef) if ln == 0 else (coef, coef)
            pad.append((i, 0, ptiles) + src + dst + (first, head, N)); ptiles += (N - first + PAD_BLOCK - 1) // PAD_BLOCK
        if ln + lb:
            fwd.append((i, ln + lb, ln if skip else -1, coef, (OUT, 0), X))
    launches = ref_transforms(INVERSE, inv, False)
    if pad:
        launches.append(((PAD, 0, 0, 0, ptiles, 0), [], pad))
    return scratch, launches + ref_transforms(FORWARD, fwd, coset)


def lib_plan(lib, log_ns, lde, inverse, coset, lb):
    lg = (C.c_size_t * max(len(log_ns), 1))(*log_ns)
    lib.hc_ntt_mixed_plan.restype = C.c_size_t
    args = (C.c_size_t(len(log_ns)), lg, int(lde), int(inverse), int(coset), C.c_size_t(lb), 11, 0)
    need = lib.hc_ntt_mixed_plan(*args, None, C.c_size_t(0))
    buf = (C.c_int64 * need)()
    assert lib.hc_ntt_mixed_plan(*args, buf, C.c_size_t(need)) == need
    w = list(buf); scratch, nl = w[0], w[1]; pos = 2; launches = []
    for _ in range(nl):
        kind, step, strided, pre, ntiles, lds, ns, nc = w[pos:pos + 8]; pos += 8
        shapes = [tuple(w[pos + 8 * k:pos + 8 * k + 8]) for k in range(ns)]; pos += 8 * ns
        cols = [tuple(w[pos + 10 * k:pos + 10 * k + 10]) for k in range(nc)]; pos += 10 * nc
        launches.append(((kind, step, strided, pre, ntiles, lds), shapes, cols))
    assert pos == need
    return scratch, launches


def ref_one_shape(launch):
    """ntt_mixed_one_shape restated: None, or (src.mem, src.off, src.pitch, dst.mem, dst.off, dst.pitch) — one shape record, and each end wholly the
    caller's memory of one kind or wholly scratch at off + k * pitch for the k-th column in launch order"""
    (kind, *_), shapes, cols = launch
    if kind == PAD or len(shapes) != 1:
        return None
    ends = []
    for m, o in ((3, 4), (5, 6)):
        if len({c[m] for c in cols}) != 1:
            return None
        offs = [c[o] for c in cols]
        if cols[0][m] != SCRATCH:
            ends += [cols[0][m], 0, 0]; continue
        pitch = offs[1] - offs[0] if len(offs) > 1 else 0
        if pitch < 0 or offs != [offs[0] + k * pitch for k in range(len(offs))]:
            return None
        ends += [SCRATCH, offs[0], pitch]
    return tuple(ends)


def lib_one_shape(lib, log_ns, lde, inverse, coset, lb):
    lg = (C.c_size_t * max(len(log_ns), 1))(*log_ns)
    lib.hc_ntt_mixed_one_shape.restype = C.c_size_t
    args = (C.c_size_t(len(log_ns)), lg, int(lde), int(inverse), int(coset), C.c_size_t(lb), 11, 0)
    nl = lib.hc_ntt_mixed_one_shape(*args, None, C.c_size_t(0))
    buf = (C.c_int64 * max(7 * nl, 1))()
    assert lib.hc_ntt_mixed_one_shape(*args, buf, C.c_size_t(7 * nl)) == nl
    return [tuple(buf[7 * k + 1:7 * k + 7]) if buf[7 * k] else None for k in range(nl)]


def check_transform_launches(launches, sizes, pre_first, what):
    """sizes: {col: log_n} of the transforms these launches run"""
    seen = {c: [] for c in sizes}
    for (kind, step, strided, pre, ntiles, lds), shapes, cols in launches:
        assert 1 <= len(shapes) <= 31, what
        t = 0
        for col, sh, first_tile, *_ in cols:
            log_n, P, j, log_b, log_c, log_m, lnz, tiles = shapes[sh]
            assert log_n == sizes[col] and P == len(ls.split(log_n)) and step == 3 - P + j, (what, col)
            assert bool(strided) == (j < P - 1) == (step < 2) and bool(pre) == (pre_first and j == 0), (what, col)       # no launch mixes the forms
            assert first_tile == t and tiles >= 1 and tiles << (log_b + log_c) == 1 << log_n, (what, col)                # tile ranges partition the launch
            assert lds_bytes(log_b, log_c) <= lds <= MAX_LDS, (what, col)
            t += tiles; seen[col].append(j)
        assert t == ntiles, what
        tile = [shapes[sh][3] + shapes[sh][4] for _, sh, *_ in cols]
        assert tile == sorted(tile, reverse=True), (what, "larger tiles go first")
    for c, log_n in sizes.items():
        assert seen[c] == list(range(len(ls.split(log_n)))), (what, c, seen[c])                                          # every pass once, in order


def scratch_spans(launches):
    """{col: set of (offset, elements)} of every scratch range the plan reads or writes"""
    out = {}
    for (kind, *_), shapes, cols in launches:
        for col, sh, _, smem, soff, dmem, doff, first, head, length in cols:
            if kind == PAD:
                spans = [(dmem, doff, length)]
            else:
                log_n, lnz = shapes[sh][0], shapes[sh][6]
                spans = [(smem, soff, 1 << (lnz if lnz >= 0 else log_n)), (dmem, doff, 1 << log_n)]
            for mem, off, n in spans:
                if mem == SCRATCH:
                    out.setdefault(col, set()).add((off, n))
    return out


def check_scratch(scratch, launches, what):
    spans = scratch_spans(launches)
    hull = sorted((min(o for o, _ in s), max(o + n for o, n in s), c) for c, s in spans.items())
    for (lo, hi, c), nxt in zip(hull, hull[1:] + [(scratch, scratch, None)]):
        assert hi <= nxt[0], (what, "the scratch of columns %s and %s overlaps" % (c, nxt[2]))


def route_of_plan(launches, col, ln, lb, pre):
    """the route name of lde_shapes, read off the plan: the pad launch, and the first pass of the column's forward transform"""
    fwd = [(shapes[sh], s) for (kind, *_), shapes, cols in launches if kind == FORWARD for s in cols for sh in [s[1]] if s[0] == col and shapes[sh][2] == 0]
    padded = any(kind == PAD and s[0] == col for (kind, *_), _, cols in launches for s in cols)
    P = fwd[0][0][1] if fwd else 1
    if lb == 0:
        return P, ls.NO_EXTENSION
    if padded:
        return P, ls.PADDED
    (log_n, _, _, log_b, _, log_m, lnz, _), rec = fwd[0]
    assert lnz == ln and rec[3] == SCRATCH
    nz, B = 1 << (lnz - (log_m - log_b)), 1 << log_b
    if not pre:
        return P, ls.UNIT
    if log_b >= 3 and nz <= B >> 3:
        return P, ls.FAST if nz == B >> 3 else ls.FAST_ZERO_ONE if nz == 1 else ls.FAST_ZERO
    return P, ls.GENERAL


def multisets():
    for k in range(1, 5):
        yield from itertools.combinations_with_replacement(SIZES, k)


def test_plan_equals_a_plain_restatement_and_keeps_its_promises():
    lib = C.CDLL(hostcheck_lib.PATH)
    rng = np.random.default_rng(0x91A4)
    routes = set()
    for ms in multisets():
        log_ns = [int(x) for x in rng.permutation(ms)]                         # the caller's order is arbitrary
        for inverse in (0, 1):
            for coset in (0, 1):
                what = "transform %s, inverse %d, coset %d" % (log_ns, inverse, coset)
                scratch, launches = lib_plan(lib, log_ns, 0, inverse, coset, 0)
                assert (scratch, launches) == ref_plan(log_ns, 0, inverse, coset, 0), what
                assert lib_one_shape(lib, log_ns, 0, inverse, coset, 0) == [ref_one_shape(l) for l in launches], what
                assert len(launches) <= 5, what
                assert all(k == (INVERSE if inverse else FORWARD) for (k, *_), _, _ in launches)
                check_transform_launches(launches, {i: ln for i, ln in enumerate(log_ns) if ln}, bool(coset and not inverse), what)
                check_scratch(scratch, launches, what)
        for lb in (0, 1, 3, 7):
            for coset in (0, 1):
                what = "LDE %s, blow-up %d, coset %d" % (log_ns, lb, coset)
                scratch, launches = lib_plan(lib, log_ns, 1, 0, coset, lb)
                assert (scratch, launches) == ref_plan(log_ns, 1, 0, coset, lb), what
                assert lib_one_shape(lib, log_ns, 1, 0, coset, lb) == [ref_one_shape(l) for l in launches], what
                assert scratch == sum((1 << (ln + lb)) + (1 << ln) for ln in log_ns), what
                kinds = [k for (k, *_), _, _ in launches]
                assert kinds == sorted(kinds) and kinds.count(PAD) <= 1 and kinds.count(INVERSE) <= 3 and kinds.count(FORWARD) <= 5 and len(launches) <= 9, what
                check_transform_launches([l for l in launches if l[0][0] == INVERSE], {i: ln for i, ln in enumerate(log_ns) if ln}, False, what)
                check_transform_launches([l for l in launches if l[0][0] == FORWARD], {i: ln + lb for i, ln in enumerate(log_ns) if ln + lb}, bool(coset), what)
                for (kind, _, _, _, ntiles, _), _, cols in launches:
                    if kind == PAD:
                        t = 0
                        for col, _, first_tile, *_, first, head, length in cols:
                            assert first_tile == t and first < length == 1 << (log_ns[col] + lb), what
                            t += (length - first + PAD_BLOCK - 1) // PAD_BLOCK
                        assert t == ntiles, what
                check_scratch(scratch, launches, what)
                for i, ln in enumerate(log_ns):
                    got = route_of_plan(launches, i, ln, lb, coset)
                    assert got == ls.route(ln, lb, coset), (what, i, got)
                    routes.add(got[1])
    assert {ls.NO_EXTENSION, ls.PADDED, ls.UNIT} <= routes and routes & set(ls.SKIP_COSET), routes       # padded, skipping and unextended columns all occurred


def same_size_launches(B, log_n):
    """(strided, log_b, log_c, ntiles) per launch of B transforms of 2^log_n points as a same-size driver cuts them: the split of one transform, tile
    widths picked over all B << log_n elements"""
    b = ls.split(log_n); total, rem, out = B << log_n, log_n, []
    for i in range(len(b) - 1):
        lc = pick_log_c(b[i], rem - b[i], total.bit_length() - 1); out.append((1, b[i], lc, total >> (b[i] + lc))); rem -= b[i]
    lc = 0 if len(b) == 1 else pick_log_c(b[-1], b[0], total.bit_length() - 1)
    return out + [(0, b[-1], lc, total >> (b[-1] + lc))]


def check_equal_lengths(lib, log_ns, lde, inverse, coset, lb):
    """every transform launch of a batch of equal lengths has one shape at one pitch, and the launches are the same-size driver's"""
    B, ln = len(log_ns), log_ns[0]; what = (log_ns, lde, inverse, coset, lb)
    scratch, launches = lib_plan(lib, log_ns, lde, inverse, coset, lb)
    assert (scratch, launches) == ref_plan(log_ns, lde, inverse, coset, lb), what
    one = lib_one_shape(lib, log_ns, lde, inverse, coset, lb)
    assert one == [ref_one_shape(l) for l in launches], what
    pitch = (1 << (ln + lb)) + (1 << ln) if lde else 1 << ln
    got = {INVERSE: [], FORWARD: []}
    for ((kind, step, strided, pre, ntiles, lds), shapes, cols), ends in zip(launches, one):
        if kind == PAD:
            assert ends is None, what
            continue
        assert ends is not None and len(shapes) == 1 and [c[0] for c in cols] == list(range(B)), what
        for mem, off, p in (ends[:3], ends[3:]):
            assert p == pitch if mem == SCRATCH else (off, p) == (0, 0), (what, ends)
        assert ntiles == B * shapes[0][7] and lds == lds_bytes(shapes[0][3], shapes[0][4]), what
        got[kind].append((strided, shapes[0][3], shapes[0][4], ntiles))
    if not lde:
        want = {INVERSE if inverse else FORWARD: same_size_launches(B, ln) if ln else [], FORWARD if inverse else INVERSE: []}
    else:
        want = {INVERSE: same_size_launches(B, ln) if ln else [], FORWARD: same_size_launches(B, ln + lb) if ln + lb else []}
    assert got == want, (what, got, want)
    return launches


def test_equal_lengths_are_one_shape_launches_with_the_same_size_drivers_tiles():
    lib = C.CDLL(hostcheck_lib.PATH)
    for coset in (0, 1):
        for inverse in (0, 1):
            assert len(check_equal_lengths(lib, [11] * 3, 0, inverse, coset, 0)) == 2
        kinds = lambda launches: [l[0][0] for l in launches]
        assert kinds(check_equal_lengths(lib, [8] * 4, 1, 0, coset, 3)) == [INVERSE, FORWARD, FORWARD]             # skip route: no pad launch
        assert kinds(check_equal_lengths(lib, [4] * 3, 1, 0, coset, 1)) == [INVERSE, PAD, FORWARD]                 # padded route
        assert kinds(check_equal_lengths(lib, [0] * 3, 1, 0, coset, 0)) == [PAD]                                   # one point, no extension: a copy
        launches = check_equal_lengths(lib, [0] * 3, 1, 0, coset, 2)
        assert kinds(launches) == [PAD, FORWARD] and ref_one_shape(launches[1]) == (SCRATCH, 0, 5, OUT, 0, 0)      # reads the padded points at N + n


def test_mixed_lengths_one_shape_launches_inside_ragged_calls():
    lib = C.CDLL(hostcheck_lib.PATH)
    for coset in (0, 1):
        for inverse in (0, 1):
            # (b) step 1 holds the first pass of the two 2^12 columns only: one shape over a subset of the caller's table; step 2 has three shapes
            _, launches = lib_plan(lib, [5, 12, 3, 12], 0, inverse, coset, 0)
            one = lib_one_shape(lib, [5, 12, 3, 12], 0, inverse, coset, 0)
            assert [(l[0][1], [c[0] for c in l[2]]) for l in launches][0] == (1, [1, 3]), launches
            assert one[0] == (IN, 0, 0, SCRATCH, 0, 1 << 12) and len(launches[0][1]) == 1
            assert all(l[0][1] == 2 and (o is None) == (len(l[1]) > 1) for l, o in zip(launches[1:], one[1:]))
            if coset and not inverse:                                      # the pre-scaled form is a launch of its own: the one-pass columns
                assert [(l[0][3], len(l[1])) for l in launches[1:]] == [(0, 1), (1, 2)] and one[1] == (SCRATCH, 0, 1 << 12, OUT, 0, 0)
            else:
                assert [len(l[1]) for l in launches[1:]] == [3] and one[1:] == [None]
        # (c) no launch with two shapes is a one-shape launch
        _, launches = lib_plan(lib, [9, 9, 10], 1, 0, coset, 2)
        one = lib_one_shape(lib, [9, 9, 10], 1, 0, coset, 2)
        assert one == [ref_one_shape(l) for l in launches] and any(len(l[1]) == 2 for l in launches)
        for l, o in zip(launches, one):
            assert o is None or len(l[1]) == 1, l


def test_launch_count_does_not_grow_with_the_batch_or_the_sizes():
    lib = C.CDLL(hostcheck_lib.PATH)
    log_ns = [ln for ln in range(0, 22) for _ in range(3)]
    for coset in (0, 1):
        assert len(lib_plan(lib, log_ns, 0, 0, coset, 0)[1]) <= 5
        assert len(lib_plan(lib, log_ns, 1, 0, coset, 3)[1]) <= 9
        for _, shapes, _ in lib_plan(lib, log_ns, 1, 0, coset, 3)[1]:
            assert len(shapes) <= 31


# ---- pass cutting and the overlap check ---------------------------------------------------------------------------------------------------------
def passes_ref(log_out, limit):
    out, cols, total = [], 0, 0
    for lg in log_out:
        if cols and total + (1 << lg) > limit:
            out.append(cols); cols, total = 0, 0
        cols += 1; total += 1 << lg
    return out + ([cols] if cols else [])


def test_pass_cutting_with_a_length_per_column():
    lib = C.CDLL(hostcheck_lib.PATH)
    lib.hc_ntt_mixed_passes.restype = C.c_size_t
    rng = np.random.default_rng(0xC077)

    def cut(log_out, limit):
        lg = (C.c_size_t * max(len(log_out), 1))(*log_out); buf = (C.c_size_t * 64)()
        k = lib.hc_ntt_mixed_passes(C.c_size_t(len(log_out)), lg, C.c_size_t(limit), buf, C.c_size_t(64))
        assert k <= 64
        return [int(buf[i]) for i in range(k)]
    assert cut([], 1 << 24) == []
    assert cut([11, 11, 8, 14, 11], 2 << 11) == [2, 1, 1, 1] and cut([11, 11, 8, 14, 11], 1 << 24) == [5]
    for _ in range(2000):
        log_out = [int(x) for x in rng.integers(0, 27, int(rng.integers(0, 12)))]
        limit = int(rng.choice([1 << 10, (1 << 14) + 1, 3 << 19, 1 << 24, 1 << 28]))
        got = cut(log_out, limit)
        assert got == passes_ref(log_out, limit), (log_out, limit, got)
        assert sum(got) == len(log_out) and all(p >= 1 for p in got)                                   # every column once, in order: consecutive runs
        pos = 0
        for p in got:
            assert p == 1 or sum(1 << lg for lg in log_out[pos:pos + p]) <= limit, (log_out, limit, got)   # over the limit only as a pass of one column
            pos += p


def test_overlap_check_of_ranges_of_different_lengths():
    lib = C.CDLL(hostcheck_lib.PATH)

    def overlap(ranges):
        a = np.array([s for s, _ in ranges], np.uint64); b = (C.c_size_t * max(len(ranges), 1))(*[n for _, n in ranges])
        return lib.hc_ntt_mixed_ranges_overlap(a.ctypes.data_as(C.c_void_p), b, C.c_size_t(len(ranges)))
    assert overlap([]) == 0 and overlap([(4096, 32)]) == 0
    assert overlap([(4096, 1024), (4096 + 1024, 32), (4096 + 1056, 4096)]) == 0                       # adjacent
    assert overlap([(4096 + 1056, 4096), (4096, 1024), (4096 + 1024, 32)]) == 0                       # adjacent, out of order
    assert overlap([(4096, 1025), (4096 + 1024, 32)]) == 1 and overlap([(4096 + 1024, 32), (4096, 1025)]) == 1    # one byte
    assert overlap([(4096, 1 << 20), (4096 + 4096, 32)]) == 1 and overlap([(8192, 32), (16384, 64), (4096, 1 << 20)]) == 1   # a short range inside a long one
    assert overlap([(4096, 32), (4096, 1 << 20)]) == 1                                                # the same start
    assert overlap([(4096 + 32, 32), (4096, 64), (1 << 40, 32)]) == 1                                  # the end of a long range reaches into the next
    assert overlap([((1 << 63) + 4096, 1024), (4096, 1 << 30), ((1 << 63) + 4096 + 1024, 32)]) == 0
