"""The block form of lagrange_eval_on_h without a device: stark_lagrange_eval_shard_dev per block and stark_lagrange_eval_from_partials_dev through
their host instantiations (hc_lagrange_eval_shard, hc_lagrange_eval_from_partials: the same driver, every workgroup of k_lagrange_partials in
lockstep, the column groups included), against the definition (R2 of lagrange_cases.py) and, inside H, the columns' own bytes; the header of the
collective call.  CPU only."""
import numpy as np
import pytest

import lagrange_cases as lc
import lagrange_shard_cases as sc


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=-1))
    assert not bad[0].size, "%s: first difference at %s" % (what, tuple(int(b[0]) for b in bad))


@pytest.mark.parametrize("n,blocks", sc.PARTITIONS, ids=sc.PARTITION_IDS)
def test_partitions(hostcheck, oracle, n, blocks):
    """3 columns at two points outside H mixed with points inside H: the combined shares are R2; inside H the owner's share is the column's bytes and
    every other block's share is zero bytes; the passes of a block follow its own geometry"""
    cols = lc.columns(oracle, n, 3); zs, ins = sc.mixed_points(oracle, n, blocks)
    got, shares, passes = sc.hc_partitioned(hostcheck, cols, n, blocks, zs)
    same(got, sc.reference(oracle, n, blocks), "n = %d, blocks %s against R2" % (n, blocks))
    for q, j in ins:
        same(got[q], np.stack([v[j] for v in cols]), "z = omega^%d" % j)
        for b, (j0, nl) in enumerate(blocks):
            want = np.stack([v[j] for v in cols]) if j0 <= j < j0 + nl else np.zeros((3, 4), np.uint64)
            same(shares[b, q], want, "the share of block %d at z = omega^%d" % (b, j))
    assert passes == [lc.expected_passes(nl, 3, 2) for _, nl in blocks] == [1] * len(blocks)
    whole, took = lc.hc_eval(hostcheck, cols, n, zs)
    same(got, whole, "the partition against the single call")
    assert took == lc.expected_passes(n, 3, 2)


@pytest.mark.parametrize("max_partials", [0, 1])
def test_column_groups(hostcheck, oracle, max_partials):
    """9 and 17 columns at n = 2^12 in 1, 2, 3, 9 and 64 groups (an uneven last group, more groups than columns) and under the automatic rule: equal
    bytes and equal passes, over uneven blocks of one and of two workgroups; max_partials = 1: passes of one point"""
    n = 1 << 12; blocks = [(0, 1000), (1000, 3096)]; zs = lc.points(oracle, n, 2)
    for ncols in sc.GROUP_NCOLS:
        cols = sc.columns17(oracle, n)[:ncols]; want = sc.reference17(oracle, n, zs)[:, :ncols]
        first = None
        for g in sc.GROUPS + (-1,):
            got, shares, passes = sc.hc_partitioned(hostcheck, cols, n, blocks, zs, max_partials=max_partials, col_groups=g)
            same(got, want, "%d columns in %d groups against R2" % (ncols, g))
            assert passes == [lc.expected_passes(nl, ncols, 2, max_partials or lc.DEFAULT_MAX_PARTIALS) for _, nl in blocks] == ([2, 2] if max_partials else [1, 1]), (g, passes)
            if first is None:
                first = shares
            same(shares, first, "the shares of %d columns in %d groups against one group" % (ncols, g))


def test_the_rule_of_the_column_groups(hostcheck):
    """lag_col_groups: min(g, ncols) groups, none empty; automatic: one group below 16 columns, never fewer than 8 columns per group, and no group
    added once the launch has 512 workgroups (kLagGroupTargetWorkgroups)"""
    n = 1 << 12                                                 # two tiles; two points: two point groups
    for ncols in (1, 9, 15):
        assert sc.hc_col_groups(hostcheck, -1, ncols, n, 2) == (1, ncols)
    assert sc.hc_col_groups(hostcheck, -1, 16, n, 2) == (2, 8)
    assert sc.hc_col_groups(hostcheck, -1, 17, n, 2) == (2, 9)
    assert sc.hc_col_groups(hostcheck, -1, 64, n, 2) == (8, 8)
    assert sc.hc_col_groups(hostcheck, -1, 64, 1 << 16, 2) == (8, 8)          # 32 tiles x 2 point groups x 8 = 512
    assert sc.hc_col_groups(hostcheck, -1, 64, 1 << 17, 2) == (4, 16)         # a shard of 2^20 rows over 8 ranks: 64 tiles x 2 point groups x 4 = 512
    assert sc.hc_col_groups(hostcheck, -1, 64, 1 << 20, 1) == (1, 64)         # 512 tiles already
    assert sc.hc_col_groups(hostcheck, -1, 1 << 16, n, 2)[0] == 128           # 2 x 2 x 128 = 512
    for ncols in sc.GROUP_NCOLS:
        for g in sc.GROUPS:
            groups, per = sc.hc_col_groups(hostcheck, g, ncols, n, 2)
            assert groups <= min(g, ncols) and (groups - 1) * per < ncols <= groups * per, (ncols, g, groups, per)
            assert per == -(-ncols // min(g, ncols))
    assert sc.hc_col_groups(hostcheck, 9, 17, n, 2) == (9, 2) and sc.hc_col_groups(hostcheck, 64, 9, n, 2) == (9, 1) and sc.hc_col_groups(hostcheck, 2, 17, n, 2) == (2, 9)


def test_corners_and_another_primitive_root(hostcheck, oracle):
    n = 1 << 12
    cols = lc.corner_columns(n, 3); zs = lc.corners()[:11]
    got, _, _ = sc.hc_partitioned(hostcheck, cols, n, sc.even(n, 4), zs)
    same(got, lc.r2(oracle, cols, zs), "corner columns and points at n = 2^12, W = 4")
    v = lc.columns(oracle, n, 1)[0]; w3, u = lc.third_power_domain(oracle, v)
    zs = np.concatenate([lc.points(oracle, n, 2), [oracle.pow(w3, 5)], [oracle.pow(w3, n // 2 + 5)]])
    got, shares, _ = sc.hc_partitioned(hostcheck, [v], n, sc.even(n, 2), zs, omega=w3)
    same(got, lc.r2(oracle, [u], zs), "omega^3 as the generator at n = 2^12, W = 2")
    same(got[2], v[5:6], "z = (omega^3)^5"); same(got[3], v[n // 2 + 5:n // 2 + 6], "z = (omega^3)^(n/2 + 5)")
    same(shares[:, 2, 0], np.stack([v[5], np.zeros(4, np.uint64)]), "the first block owns row 5")
    same(shares[:, 3, 0], np.stack([np.zeros(4, np.uint64), v[n // 2 + 5]]), "the second block owns row n/2 + 5")


@pytest.mark.parametrize("fill", [0x5A, 0x00])
def test_does_not_depend_on_stale_blocks(hostcheck, oracle, fill):
    """the uneven partition of 2^12 with every block of the host executor pre-filled, in one pass and in passes of one point"""
    n, blocks = sc.PARTITIONS[5]; cols = lc.columns(oracle, n, 3); zs, _ = sc.mixed_points(oracle, n, blocks)
    old = hostcheck.set_alloc_fill(fill)
    try:
        for max_partials in (0, 1):
            got, _, passes = sc.hc_partitioned(hostcheck, cols, n, blocks, zs, max_partials=max_partials)
            same(got, sc.reference(oracle, n, blocks), "fill %#x, max_partials %d" % (fill, max_partials))
            assert passes == ([2, 2, 2] if max_partials else [1, 1, 1])
    finally:
        hostcheck.set_alloc_fill(old)


def test_refusals(hostcheck, oracle):
    n = 8; cols = lc.columns(oracle, n, 2); zs = lc.points(oracle, n, 2); one = oracle.from_u64(1)
    rows = sc.block_rows(cols, 0, 4)
    assert sc.hc_shard_rc(hostcheck, rows, 4, 0, n, zs)[0] == 0 and sc.hc_shard_rc(hostcheck, rows, 4, 4, n, zs)[0] == 0
    assert sc.hc_shard_rc(hostcheck, rows, 0, 0, n, zs)[0] == -1, "n_local = 0"
    assert sc.hc_shard_rc(hostcheck, rows, 4, 5, n, zs)[0] == -1, "j0 + n_local > n_global"
    assert sc.hc_shard_rc(hostcheck, rows, 4, 9, n, zs)[0] == -1, "j0 > n_global"
    assert sc.hc_shard_rc(hostcheck, rows, 4, (1 << 64) - 2, n, zs)[0] == -1, "j0 + n_local wraps"
    assert sc.hc_shard_rc(hostcheck, rows, 4, 0, 12, zs)[0] == -1 and sc.hc_shard_rc(hostcheck, rows, 4, 0, 0, zs)[0] == -1, "n_global not a power of two"
    assert sc.hc_shard_rc(hostcheck, rows, 4, 0, n, zs, omega=one)[0] == -1, "omega = 1"
    assert sc.hc_shard_rc(hostcheck, rows, 4, 0, n, zs, omega=oracle.domain_omega(16))[0] == -1, "omega of order 2 n"
    assert sc.hc_shard_rc(hostcheck, rows, 4, 0, n, zs, omega=oracle.domain_omega(4))[0] == -1, "omega of order n / 2"
    shares = np.zeros((2, 2, 2, 4), np.uint64)
    assert sc.hc_from_partials_rc(hostcheck, shares, 2, n, zs)[0] == 0
    assert sc.hc_from_partials_rc(hostcheck, shares[:0], 2, n, zs)[0] == -1, "nparts = 0"
    assert sc.hc_from_partials_rc(hostcheck, shares, 2, 12, zs)[0] == -1 and sc.hc_from_partials_rc(hostcheck, shares, 2, n, zs, omega=one)[0] == -1


def test_header_of_the_collective_call(hostcheck, oracle):
    """the header every rank all-gathers first: equal arguments give equal headers; one limb of one point, ncols, npoints, n or omega change it, and
    the comparison flags a single rank that differs"""
    n = 1 << 12; w = lc.omega_of(oracle, n); zs = np.array(lc.points(oracle, n, 5))
    h = sc.hc_header(hostcheck, n, 3, zs, w)
    assert (h == sc.hc_header(hostcheck, n, 3, zs.copy(), w.copy())).all() and h[1] == n and h[2] == 3 and h[3] == 5
    others = {}
    for p in range(5):
        for limb in range(4):
            z2 = zs.copy(); z2[p, limb] ^= np.uint64(1)
            others["limb %d of point %d" % (limb, p)] = sc.hc_header(hostcheck, n, 3, z2, w)
    others["ncols"] = sc.hc_header(hostcheck, n, 4, zs, w)
    others["npoints"] = sc.hc_header(hostcheck, n, 3, zs[:4], w)
    others["n_global"] = sc.hc_header(hostcheck, 2 * n, 3, zs, w)
    others["omega"] = sc.hc_header(hostcheck, n, 3, zs, oracle.pow(w, 3))
    others["two points swapped"] = sc.hc_header(hostcheck, n, 3, zs[[1, 0, 2, 3, 4]], w)
    assert sc.hc_headers_agree(hostcheck, [h] * 8, h)
    for what, o in others.items():
        assert (o != h).any(), what
        for at in (0, 3, 7):
            assert not sc.hc_headers_agree(hostcheck, [h] * at + [o] + [h] * (7 - at), h), "%s at rank %d" % (what, at)
    assert len({o.tobytes() for o in others.values()}) == len(others)
