"""stark_lagrange_eval_on_h_dev / _batch_dev without a device: the driver (host classification of the points, 2-adic discrete logarithm, passes, gather,
finish) and the lane pieces of k_lagrange_partials (csrc/lagrange_dev.hpp) through their host instantiation hc_lagrange_eval_batch, against the
oracle's own lagrange_eval_on_h (R1), the definition (R2) and the columns' own bytes (R3) of lagrange_cases.py.  CPU only."""
import numpy as np
import pytest

import lagrange_cases as lc


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=-1))
    assert not bad[0].size, "%s: first difference at (point, column) = %s" % (what, tuple(int(b[0]) for b in bad))


def run_matrix(hostcheck, oracle):
    for n in lc.N_MATRIX:
        ref = lc.matrix_reference(oracle, n)
        for ncols in lc.NCOLS:
            for npoints in lc.NPOINTS:
                got, passes = lc.hc_eval(hostcheck, lc.columns(oracle, n, ncols), n, lc.points(oracle, n, npoints))
                assert passes == lc.expected_passes(n, ncols, npoints) == 1
                same(got, ref[:npoints, :ncols], "n = %d, %d columns, %d points against R2" % (n, ncols, npoints))


def test_the_two_references_agree(oracle):
    """R1 = R2 on the oracle alone at the matrix's sizes: the reference's function and the definition give the same bytes"""
    for n in lc.N_MATRIX:
        if n >= 2:
            cols = lc.columns(oracle, n, 2); zs = lc.points(oracle, n, 3)
            same(lc.r1(oracle, cols, zs), lc.matrix_reference(oracle, n)[:3, :2], "R1 against R2 at n = %d" % n)
    v = lc.columns(oracle, 8, 1)[0]
    same(lc.r2(oracle, [v], [oracle.pow(lc.omega_of(oracle, 8), 5)])[0], v[5:6], "R2 at omega^5")


def test_shape_matrix(hostcheck, oracle):
    run_matrix(hostcheck, oracle)
    for n in (2, 256, 1 << 12):
        cols = lc.columns(oracle, n, 3); zs = lc.points(oracle, n, 2)
        same(lc.hc_eval(hostcheck, cols, n, zs)[0], lc.r1(oracle, cols, zs), "n = %d against R1" % n)
    v = lc.columns(oracle, 1, 1)[0]
    same(lc.hc_eval(hostcheck, [v], 1, lc.points(oracle, 1, 5))[0], np.tile(v[0], (5, 1, 1)), "n = 1 gives v[0] for every z")


@pytest.mark.parametrize("fill", [0x5A, 0x00])
def test_shape_matrix_does_not_depend_on_stale_blocks(hostcheck, oracle, fill):
    """the whole matrix again with every block of the host executor pre-filled: partials, tables and uploads read nothing they did not write"""
    old = hostcheck.set_alloc_fill(fill)
    try:
        run_matrix(hostcheck, oracle)
        n = 1 << 12; cols = lc.columns(oracle, n, 3)
        zs = np.stack([lc.points(oracle, n, 2)[0], lc.inside_points(oracle, n)[3][0], lc.points(oracle, n, 2)[1]])
        got, passes = lc.hc_eval(hostcheck, cols, n, zs, max_partials=1)
        assert passes == 2
        same(got, lc.r2(oracle, cols, zs), "mixed points in passes of one under fill %#x" % fill)
    finally:
        hostcheck.set_alloc_fill(old)


@pytest.mark.parametrize("n", [1, 2, 8, 1 << 11, 1 << 12, 1 << 14])
def test_points_inside_and_outside_h_in_one_call(hostcheck, oracle, n):
    """z = 1, -1, omega^(n-1), omega^j in the second workgroup's tile, the first point twice, between points outside H: the columns' own bytes"""
    cols = lc.columns(oracle, n, 3); ins = lc.inside_points(oracle, n); outs = lc.points(oracle, n, 2)
    zs = np.stack([outs[0]] + [z for z, _ in ins] + [outs[1]])
    got, passes = lc.hc_eval(hostcheck, cols, n, zs)
    assert passes == 1
    for q, (_, j) in enumerate(ins):
        same(got[1 + q], np.stack([v[j] for v in cols]), "n = %d, z = omega^%d" % (n, j))
    same(got, lc.r2(oracle, cols, zs), "n = %d, mixed points against R2" % n)
    only_inside, passes = lc.hc_eval(hostcheck, cols, n, np.stack([z for z, _ in ins]))
    assert passes == 0
    same(only_inside, got[1:-1], "n = %d, only points inside H" % n)


def test_z_zero_is_the_mean(hostcheck, oracle):
    for n in (2, 64, 1 << 12):
        cols = lc.columns(oracle, n, 3)
        got, _ = lc.hc_eval(hostcheck, cols, n, np.zeros((1, 4), np.uint64))
        same(got[0], np.stack([lc.coefficients(oracle, v)[0] for v in cols]), "z = 0 at n = %d: coefficient 0" % n)


@pytest.mark.parametrize("n,npoints", [(256, None), (1 << 12, 11)])
def test_stored_limb_corners(hostcheck, oracle, n, npoints):
    """columns and points whose stored limbs are corners; the Montgomery one and its negative among the points are z = 1 and z = -1, inside H"""
    cols = lc.corner_columns(n, 3); zs = lc.corners()[:npoints]
    got, _ = lc.hc_eval(hostcheck, cols, n, zs)
    same(got, lc.r2(oracle, cols, zs), "corner values at n = %d" % n)


def test_repeated_column_and_another_primitive_root(hostcheck, oracle):
    n = 1 << 11; a, b = lc.columns(oracle, n, 2); zs = lc.points(oracle, n, 2)
    got, _ = lc.hc_eval(hostcheck, [a, b, a, a], n, zs)
    same(got, lc.matrix_reference(oracle, n)[:2, [0, 1, 0, 0]], "a repeated column pointer")
    for n in (8, 1 << 12):
        v = lc.columns(oracle, n, 1)[0]; w3, u = lc.third_power_domain(oracle, v)
        zs = np.concatenate([lc.points(oracle, n, 2), [oracle.pow(w3, 5)]])
        got, _ = lc.hc_eval(hostcheck, [v], n, zs, omega=w3)
        same(got, lc.r2(oracle, [u], zs), "omega^3 as the generator at n = %d" % n)
        same(got[2], v[5:6], "z = (omega^3)^5 at n = %d" % n)
        same(got[:2], lc.r1(oracle, [v], zs[:2], omega=w3), "omega^3 as the generator at n = %d against R1" % n)


def test_passes(hostcheck, oracle):
    """5 points at n = 2^12 (two workgroups per column) and 3 columns: passes of one point, of two, and one pass; equal bytes"""
    n, ncols = 1 << 12, 3
    cols = lc.columns(oracle, n, ncols); zs = lc.points(oracle, n, 5); want = lc.matrix_reference(oracle, n)[:, :ncols]
    per_point = ncols * lc.workgroups(n)
    for max_partials, passes in ((1, 5), (per_point, 5), (2 * per_point, 3), (2 * per_point + 1, 3), (5 * per_point, 1), (0, 1)):
        got, took = lc.hc_eval(hostcheck, cols, n, zs, max_partials=max_partials)
        assert took == passes == lc.expected_passes(n, ncols, 5, max_partials or lc.DEFAULT_MAX_PARTIALS), (max_partials, took)
        same(got, want, "max_partials = %d" % max_partials)


def test_refused_domains(hostcheck, oracle):
    one = oracle.from_u64(1)
    assert lc.hc_refused(hostcheck, 0, None) and lc.hc_refused(hostcheck, 3, None) and lc.hc_refused(hostcheck, 1 << 31, None)
    assert lc.hc_refused(hostcheck, 4, one), "omega = 1 at n = 4"
    assert lc.hc_refused(hostcheck, 4, oracle.domain_omega(8)), "omega of order 2 n"
    assert lc.hc_refused(hostcheck, 4, oracle.domain_omega(2)), "omega of order n / 2"
    assert not lc.hc_refused(hostcheck, 4, oracle.domain_omega(4)) and not lc.hc_refused(hostcheck, 4, None) and not lc.hc_refused(hostcheck, 1, one)
