"""The two routes of lagrange_eval_batch behind the options "lagrange_shared_inverse" and "lagrange_share_cosets" (csrc/lagrange_dev.hpp) without a device:
the driver with k_lagrange_totals, k_lagrange_invert and the shared / coset forms of k_lagrange_partials in lockstep on the host, through
hc_lagrange_eval_batch_opt and hc_lagrange_eval_shard_opt (csrc/hostcheck.cpp).  Every result must equal the definition (R2 of lagrange_cases.py) and the
result under options (0, 0), byte for byte; the census of a call (Fermat inversions, weight sets of the partials kernel, products of the totals kernel,
member walks) shows that the routes are the ones taken.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import lagrange_cases as lc
import lagrange_shard_cases as sc

vp = C.c_void_p
SETTINGS = ((0, 1), (1, 0), (1, 1))                            # (lagrange_shared_inverse, lagrange_share_cosets)
N_MATRIX = (1, 2, 8, 64, 256, 1 << 11, 1 << 12, 1 << 14)
NCOLS = (1, 4, 9)
NPOINTS = (1, 2, 5)
INV, WEIGHTS, TOTALS, WALKS = range(4)                         # LagHostExec::census


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=-1))
    assert not bad[0].size, "%s: first difference at (point, column) = %s" % (what, tuple(int(b[0]) for b in bad))


def _call(f, cols, zs, head, omega, max_partials, col_groups, opt):
    keep = {id(v): np.ascontiguousarray(v, dtype=np.uint64) for v in cols}
    ptrs = (vp * max(len(cols), 1))(*[keep[id(v)].ctypes.data for v in cols])
    z = np.ascontiguousarray(zs, dtype=np.uint64).reshape(-1, 4); npts = z.shape[0]
    w = None if omega is None else np.ascontiguousarray(omega, dtype=np.uint64)
    out = np.full((npts, len(cols), 4), 0x5A5A5A5A5A5A5A5A, np.uint64); passes = C.c_size_t(99); census = (C.c_uint64 * 4)(9, 9, 9, 9)
    rc = f(len(cols), ptrs, *head, None if w is None else w.ctypes.data_as(vp), npts, z.ctypes.data_as(vp), max_partials, col_groups, opt[0], opt[1], out.ctypes.data_as(vp),
           C.byref(passes), census)
    assert rc == 0, rc
    return out, passes.value, [int(x) for x in census]


def hc_opt(hostcheck, cols, n, zs, opt, omega=None, max_partials=0, col_groups=-1):
    """hc_lagrange_eval_batch_opt -> ((P, C, 4), passes, census)"""
    f = hostcheck.l.hc_lagrange_eval_batch_opt
    f.argtypes = [C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_size_t), vp]; f.restype = C.c_int
    return _call(f, cols, zs, (n,), omega, max_partials, col_groups, opt)


def hc_shard_opt(hostcheck, rows, n_local, j0, n_global, zs, opt, omega=None, max_partials=0, col_groups=-1):
    """hc_lagrange_eval_shard_opt on a block's rows -> ((P, C, 4) shares, passes, census)"""
    f = hostcheck.l.hc_lagrange_eval_shard_opt
    f.argtypes = [C.c_size_t, vp, C.c_size_t, C.c_uint64, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_size_t), vp]; f.restype = C.c_int
    return _call(f, rows, zs, (n_local, j0, n_global), omega, max_partials, col_groups, opt)


def coset_points(oracle, n):
    """-> (zs (7, 4), classes): z, z w, z w^(n-1), z w^s with s in the second workgroup's tile, z again, an unrelated z2 and z2 w^(n/2), in an order that
    interleaves the two classes; classes = the positions of each class in zs, the representative first"""
    w = lc.omega_of(oracle, n); z, z2 = lc.points(oracle, n, 2); s = 300 + lc.workgroups(n) * lc.THREADS
    assert lc.workgroups(n) >= 2 and s < n
    sh = lambda a, e: oracle.mul(a, oracle.pow(w, e))
    zs = np.ascontiguousarray(np.stack([z, z2, sh(z, 1), sh(z, n - 1), sh(z2, n // 2), sh(z, s), z]))
    return zs, [[0, 2, 3, 5, 6], [1, 4]]


def check_all_settings(hostcheck, oracle, cols, n, zs, want, what, **kw):
    base, passes, census0 = hc_opt(hostcheck, cols, n, zs, (0, 0), **kw)
    same(base, want, what + " under (0, 0) against R2")
    for opt in SETTINGS:
        got, took, _ = hc_opt(hostcheck, cols, n, zs, opt, **kw)
        assert took == passes, (what, opt, took, passes)
        same(got, want, "%s under %s against R2" % (what, opt)); same(got, base, "%s under %s against (0, 0)" % (what, opt))
    return base, passes, census0


@pytest.mark.parametrize("n", N_MATRIX)
def test_shape_matrix(hostcheck, oracle, n):
    ref = lc.matrix_reference(oracle, n)
    for ncols in NCOLS:
        for npoints in NPOINTS:
            check_all_settings(hostcheck, oracle, lc.columns(oracle, n, ncols), n, lc.points(oracle, n, npoints), ref[:npoints, :ncols], "n = %d, %d columns, %d points" % (n, ncols, npoints))


@pytest.mark.parametrize("n", [2, 8, 1 << 11, 1 << 12])
def test_points_inside_and_outside_h_in_one_call(hostcheck, oracle, n):
    """the points inside H of lagrange_cases (the first twice: a shift by 0 of another inside point; -1 and omega^(n-1): shifts of 1) between two points
    outside H and a shift of the first of those"""
    cols = lc.columns(oracle, n, 3); ins = lc.inside_points(oracle, n); outs = lc.points(oracle, n, 2); w = lc.omega_of(oracle, n)
    zs = np.stack([outs[0]] + [z for z, _ in ins] + [outs[1], oracle.mul(outs[0], w)])
    got, passes, _ = check_all_settings(hostcheck, oracle, cols, n, zs, lc.r2(oracle, cols, zs), "n = %d, mixed points" % n)
    assert passes == 1
    for q, (_, j) in enumerate(ins):
        same(got[1 + q], np.stack([v[j] for v in cols]), "n = %d, z = omega^%d" % (n, j))
    _, _, census = hc_opt(hostcheck, cols, n, zs, (1, 1))
    assert census[INV] == 2, "the points inside H are gathered; the three outside are two classes"


@pytest.mark.parametrize("n", [1 << 12, 1 << 14])
def test_coset_classes(hostcheck, oracle, n):
    cols = lc.columns(oracle, n, 4); zs, classes = coset_points(oracle, n); tiles = lc.workgroups(n)
    want = lc.r2(oracle, cols, zs)
    check_all_settings(hostcheck, oracle, cols, n, zs, want, "n = %d, the coset points" % n)
    for members in classes:
        for m in members[1:]:
            assert m == 6 or (want[m] != want[members[0]]).any(), "a shifted point has its own value"
    same(want[6], want[0], "the duplicate")
    # the census: one pass, one point group per class or point (7 and 2 are below the 1024 / tiles point groups a launch may have), one column group
    assert sc.hc_col_groups(hostcheck, -1, 4, n, 7)[0] == 1 and sc.hc_col_groups(hostcheck, -1, 4, n, 2)[0] == 1
    c00 = hc_opt(hostcheck, cols, n, zs, (0, 0))[2]; c10 = hc_opt(hostcheck, cols, n, zs, (1, 0))[2]
    c01 = hc_opt(hostcheck, cols, n, zs, (0, 1))[2]; c11 = hc_opt(hostcheck, cols, n, zs, (1, 1))[2]
    assert c00 == [7 * tiles, 7 * tiles, 0, 7 * tiles], c00                       # points x tiles x column groups inversions and weight sets
    assert c10 == [7, 7 * tiles, 7 * tiles, 7 * tiles], c10                       # one inversion per outside point of the pass
    assert c01 == [2 * tiles, 2 * tiles, 0, 7 * tiles], c01                       # a workgroup computes one weight set per class it walks and serves every member
    assert c11 == [2, 2 * tiles, 2 * tiles, 7 * tiles], c11                       # totals and inverses per representative only


def test_census_with_column_groups(hostcheck, oracle):
    """3 column groups: option 0 inverts once per (point, tile, column group); the shared tables are computed once per (point, tile) and read by every group"""
    n = 1 << 12; cols = lc.columns(oracle, n, 9); zs = lc.points(oracle, n, 5); tiles = lc.workgroups(n); want = lc.matrix_reference(oracle, n)
    check_all_settings(hostcheck, oracle, cols, n, zs, want, "9 columns in 3 groups", col_groups=3)
    assert hc_opt(hostcheck, cols, n, zs, (0, 0), col_groups=3)[2] == [5 * tiles * 3, 5 * tiles * 3, 0, 5 * tiles * 3]
    assert hc_opt(hostcheck, cols, n, zs, (1, 0), col_groups=3)[2] == [5, 5 * tiles * 3, 5 * tiles, 5 * tiles * 3]


@pytest.mark.parametrize("n", [1 << 12, 1 << 14])
def test_forced_passes_cut_a_class(hostcheck, oracle, n):
    """passes of three points over the seven coset points: (z, z2, z w | z w^(n-1), z2 w^(n/2), z w^s | z), so both classes are cut and the second and third
    pass recompute a representative that lies in an earlier pass; 9 columns in 3 forced groups"""
    cols = lc.columns(oracle, n, 9); zs, _ = coset_points(oracle, n); tiles = lc.workgroups(n)
    max_partials = 3 * 9 * tiles
    base, passes, _ = check_all_settings(hostcheck, oracle, cols, n, zs, lc.r2(oracle, cols, zs), "n = %d, passes of three points" % n, max_partials=max_partials, col_groups=3)
    assert passes == 3 == lc.expected_passes(n, 9, 7, max_partials)
    same(base, hc_opt(hostcheck, cols, n, zs, (1, 1))[0], "against one pass")
    census = hc_opt(hostcheck, cols, n, zs, (1, 1), max_partials=max_partials, col_groups=3)[2]
    assert census == [2 + 2 + 1, (2 + 2 + 1) * tiles * 3, (2 + 2 + 1) * tiles, 7 * tiles * 3], census      # the classes of each pass: 2, 2 and 1
    census = hc_opt(hostcheck, cols, n, zs, (1, 0), max_partials=max_partials, col_groups=3)[2]
    assert census[INV] == 7 and census[TOTALS] == 7 * tiles, census                                         # the outside points of each pass: 3, 3 and 1
    for opt in ((0, 0),) + SETTINGS:                                                                        # passes of one point
        got, took, _ = hc_opt(hostcheck, cols[:2], n, zs, opt, max_partials=1)
        assert took == 7
        same(got, base[:, :2], "passes of one point under %s" % (opt,))


def test_block_form_ignores_the_cosets(hostcheck, oracle):
    """the blocks [0, n/4) and [n/4, n) of n = 2^12 under (1, 1), combined: the whole call; a rotation leaves the block, so every point has its own weights"""
    n = 1 << 12; cols = lc.columns(oracle, n, 4); zs, _ = coset_points(oracle, n)
    whole, _, _ = hc_opt(hostcheck, cols, n, zs, (1, 1))
    same(whole, lc.r2(oracle, cols, zs), "the whole call under (1, 1) against R2")
    shares = []
    for j0, nl in ((0, n // 4), (n // 4, n - n // 4)):
        tiles = lc.workgroups(nl); rows = sc.block_rows(cols, j0, nl)
        got, passes, census = hc_shard_opt(hostcheck, rows, nl, j0, n, zs, (1, 1))
        assert passes == 1
        assert census == [7, 7 * tiles, 7 * tiles, 7 * tiles], census              # shared inverse: one inversion per point; no sharing of weights: 7 sets per workgroup
        plain, _ = sc.hc_shard(hostcheck, rows, nl, j0, n, zs)
        same(got, plain, "the share of block (%d, %d) against hc_lagrange_eval_shard" % (j0, nl))
        assert hc_shard_opt(hostcheck, rows, nl, j0, n, zs, (0, 1))[2] == [7 * tiles, 7 * tiles, 0, 7 * tiles]
        shares.append(got)
    rc, out = sc.hc_from_partials_rc(hostcheck, np.stack(shares), 4, n, zs)
    assert rc == 0
    same(out, whole, "two blocks combined against the whole call")


def test_many_totals_per_lane(hostcheck, oracle):
    """n = 2^20, one column, two points: 512 tiles for the 256 lanes of k_lagrange_invert, two totals per lane"""
    n = 1 << 20; cols = [oracle.synth_column(lc.SEED + n, 0, 0, n)]; zs = oracle.synth_column(lc.SEED + 0x100 + n, 0, 0, 2)
    assert lc.workgroups(n) == 512
    base, passes, c0 = hc_opt(hostcheck, cols, n, zs, (0, 0)); got, took, c1 = hc_opt(hostcheck, cols, n, zs, (1, 0))
    assert passes == took == 1
    same(got, base, "n = 2^20 under (1, 0) against (0, 0)")
    assert c0[INV] == 2 * 512 and c1[INV] == 2 and c1[TOTALS] == 2 * 512


def test_stored_limb_corners(hostcheck, oracle):
    """corner columns at n = 2^11 under (1, 1); among the points z = omega^j + 1 and z = omega^j - 1, whose difference z - omega^j is 1 and r - 1, a shift
    of the first, and corner points"""
    n = 1 << 11; cols = lc.corner_columns(n, 3); w = lc.omega_of(oracle, n); one = oracle.from_u64(1)
    z_plus = oracle.add(oracle.pow(w, 777), one); z_minus = oracle.sub(oracle.pow(w, 1300), one)
    zs = np.ascontiguousarray(np.concatenate([[z_plus, z_minus, oracle.mul(z_plus, oracle.pow(w, n - 5))], lc.corners()[:11]]))
    got, _, _ = hc_opt(hostcheck, cols, n, zs, (1, 1))
    same(got, lc.r2(oracle, cols, zs), "corner values under (1, 1) against R2")
    same(got, hc_opt(hostcheck, cols, n, zs, (0, 0))[0], "corner values under (1, 1) against (0, 0)")


def test_results_do_not_depend_on_stale_blocks(hostcheck, oracle):
    """the executor's blocks pre-filled with 0x5A and with 0x00: the totals, the inverses and the class tables are written before they are read"""
    n = 1 << 12; cols = lc.columns(oracle, n, 4); zs, _ = coset_points(oracle, n); want = lc.r2(oracle, cols, zs)
    old = hostcheck.set_alloc_fill(0x5A)
    try:
        for fill in (0x5A, 0x00):
            hostcheck.set_alloc_fill(fill)
            for opt in SETTINGS:
                same(hc_opt(hostcheck, cols, n, zs, opt)[0], want, "fill %#x under %s" % (fill, opt))
                got, passes, _ = hc_opt(hostcheck, cols, n, zs, opt, max_partials=3 * 4 * lc.workgroups(n), col_groups=3)
                assert passes == 3
                same(got, want, "fill %#x under %s, passes of three" % (fill, opt))
    finally:
        hostcheck.set_alloc_fill(old)
