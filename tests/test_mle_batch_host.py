"""stark_mle_evaluate_dev / stark_mle_evaluate_batch_dev without a device: the pass structure of the driver and the tile body of k_mle_fold_pass
(csrc/mle_dev.hpp) through their host instantiation hc_mle_evaluate_batch, against the oracle's Mle::evaluate and against the definition.  CPU only."""
import numpy as np
import pytest

import mle_cases as mc


def same(got, want, what):
    assert got.shape == want.shape and (got == want).all(), "%s: first difference at instance %d" % (what, int(np.nonzero((got != want).any(axis=-1))[0][0]))


@pytest.mark.parametrize("B", [1, 3])
def test_tile_3_reaches_zero_to_four_passes(hostcheck, oracle, B):
    for k, passes in zip(mc.K_MATRIX, mc.PASSES_AT_TILE_3):
        tabs, pts = mc.tables_and_points(oracle, k, B)
        for contig in (0, 1):
            got, n = mc.hc_evaluate(hostcheck, tabs, k, pts, 3, contig)
            assert n == passes, (k, n)
            same(got, mc.reference(oracle, tabs, k, pts), "tile 3, k = %d, B = %d, contig = %d" % (k, B, contig))


@pytest.mark.parametrize("B", [1, 3])
def test_default_tile_around_its_own_size(hostcheck, oracle, B):
    T = mc.default_log_tile(hostcheck)
    assert T in mc.LOG_TILES
    for k in (T - 1, T, T + 1):
        tabs, pts = mc.tables_and_points(oracle, k, B)
        got, n = mc.hc_evaluate(hostcheck, tabs, k, pts)
        assert n == -(-k // T), (k, n)
        same(got, mc.reference(oracle, tabs, k, pts), "default tile, k = %d, B = %d" % (k, B))


def test_every_tile_and_both_lane_ownerships(hostcheck, oracle):
    """k = 13: every tile of the option's range (no, one .. four lane-local rounds; two tiles, one tile per workgroup), a full pass and a rest"""
    k = 13; tabs, pts = mc.tables_and_points(oracle, k, 2); want = mc.reference(oracle, tabs, k, pts)
    for T in mc.LOG_TILES:
        for contig in (0, 1):
            got, n = mc.hc_evaluate(hostcheck, tabs, k, pts, T, contig)
            assert n == -(-k // T)
            same(got, want, "tile %d, contig = %d" % (T, contig))
    for bad in (2, 13):
        assert hostcheck.l.hc_mle_evaluate_batch(0, None, 0, None, bad, 0, None, None) == -1


def test_one_table_at_many_points(hostcheck, oracle):
    k = 7; tabs, pts = mc.tables_and_points(oracle, k, 5)
    rep = [tabs[0], tabs[1], tabs[0], tabs[0], tabs[1]]
    got, _ = mc.hc_evaluate(hostcheck, rep, k, pts, 3)
    same(got, mc.reference(oracle, rep, k, pts), "repeated tables")
    assert len({got[i].tobytes() for i in (0, 2, 3)}) == 3


@pytest.mark.parametrize("log_tile", [3, -1])
def test_definition_at_boolean_points(hostcheck, oracle, log_tile):
    """no oracle: r = x in {0, 1}^k gives table[x] (r_0 binds the least significant bit), all zero table[0], all one table[2^k - 1]"""
    k = 4; tab = mc.tables_and_points(oracle, k, 1)[0][0]; pts = mc.boolean_points(oracle, k)
    got, _ = mc.hc_evaluate(hostcheck, [tab] * (1 << k), k, pts, log_tile)
    same(got, tab, "every Boolean point at k = 4")
    for k in (1, 7, 10, 13):
        tab = mc.tables_and_points(oracle, k, 1)[0][0]; one = oracle.from_u64(1)
        pts = np.stack([np.zeros((k, 4), np.uint64), np.tile(one, (k, 1))])
        got, _ = mc.hc_evaluate(hostcheck, [tab, tab], k, pts, log_tile)
        same(got, np.stack([tab[0], tab[-1]]), "all zero / all one at k = %d" % k)


@pytest.mark.parametrize("log_tile", [3, -1])
def test_stored_limb_corners(hostcheck, oracle, log_tile):
    for k in (1, 6, 10):
        tabs, pts = mc.corner_case(k, 3)
        got, _ = mc.hc_evaluate(hostcheck, tabs, k, pts, log_tile)
        same(got, mc.reference(oracle, tabs, k, pts), "corner values, k = %d" % k)
