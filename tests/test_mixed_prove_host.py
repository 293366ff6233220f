"""The host side of the mixed-size batch prove: hc_tr_hash_many — tr_hash_body over the Ragged layout of TrStream, built by the same
tr_ragged_items that builds the device items, in the same launch order and with the same out slots — against the oracle; the launch order
itself; and the grouping of traces by shape (mixed_prove_groups).  No GPU needed; the device side is tests/test_gpu_mixed_prove.py."""
import numpy as np
import pytest

import mixed_prove_cases as mp


@pytest.fixture(scope="module")
def tp(hostcheck):
    return hostcheck.params(1)


@pytest.fixture(scope="module")
def pl(oracle):
    return mp.pool(oracle)


def test_the_cases_reach_every_duplex_boundary(hostcheck):
    """the lengths come from the frames: with 70 items every tag absorbs 15, 16, 17, 31, 32 and 33 elements (where its frame is short enough)
    and has k = 0, 1 and 100"""
    items = mp.items_for(hostcheck, 70)
    for tag in mp.TAGS:
        np_, ns = mp.frame_dims(hostcheck, tag)
        assert np_ > 0 and np_ + ns <= 15, (tag, np_, ns)          # every boundary is reachable under every tag
        mine = [it for it in items if it[0] == tag]
        assert {mp.total_of(hostcheck, it) for it in mine} >= set(mp.BOUNDARIES), tag
        assert {it[2] for it in mine} >= {0, 1, 100}, tag
    assert len({(it[1]) for it in items[:5]}) < 5                  # a pointer used twice from count 5 on


@pytest.mark.parametrize("count", mp.COUNTS)
def test_hc_tr_hash_many_against_the_oracle(hostcheck, oracle, tp, pl, count):
    items = mp.items_for(hostcheck, count)
    before = pl.copy()
    got, order = mp.hc_hash_many(hostcheck, tp, pl, items)
    want = mp.oracle_digests(oracle, pl, items)
    for i, it in enumerate(items):
        assert (got[i] == want[i]).all(), (count, i, it)
        assert (got[i] == hostcheck.tr_hash(tp, it[0], pl[it[1]:it[1] + it[2]])).all(), (count, i, it)     # the Equal layout on the item alone
    assert (pl == before).all()
    # the launch order is a permutation, longest first, ties in the caller's order; the digests above sit in the CALLER's slots all the same
    assert sorted(order) == list(range(count))
    tot = [mp.total_of(hostcheck, items[i]) for i in order]
    assert all(tot[j] > tot[j + 1] or (tot[j] == tot[j + 1] and order[j] < order[j + 1]) for j in range(count - 1)), (order, tot)
    if count == 70:
        assert order != list(range(count))


def test_launch_order_ties_and_nulls(hostcheck, oracle, tp, pl):
    """equal lengths keep the caller's order; items of k = 0 carry no pointer at all (the whole table may be null then)"""
    import ctypes as C
    same = [(b"FRI/index", 0, 3)] * 6
    got, order = mp.hc_hash_many(hostcheck, tp, pl, same)
    assert order == list(range(6)) and (got == got[0]).all()
    mixed = [(b"FRI/index", 0, 3), (b"FRI/index", 1, 7), (b"FRI/index", 2, 3), (b"FRI/index", 3, 7), (b"FRI/index", 0, 0)]
    _, order = mp.hc_hash_many(hostcheck, tp, pl, mixed)
    assert order == [1, 3, 0, 2, 4]
    n = 3
    tags = (C.c_char_p * n)(*mp.TAGS[:n]); ks = (C.c_size_t * n)(0, 0, 0); out = np.zeros((n, 4), np.uint64)
    assert hostcheck.l.hc_tr_hash_many(tp, C.c_size_t(n), tags, None, ks, out.ctypes.data_as(mp.vp), None) == 0
    for i in range(n):
        assert (out[i] == oracle.tr_hash_fields_tagged(mp.TAGS[i], np.zeros((0, 4), np.uint64))).all(), i
    ks = (C.c_size_t * n)(0, 1, 0)                                  # a null pointer under k > 0 is refused
    assert hostcheck.l.hc_tr_hash_many(tp, C.c_size_t(n), tags, None, ks, out.ctypes.data_as(mp.vp), None) != 0


def test_groups_by_shape(hostcheck):
    S = mp.PROVE_SHAPES
    shapes = [(1 << k,) + S[k] for k in mp.PROVE_ORDER]
    grp, order, ng = mp.groups_of(hostcheck, shapes)
    assert ng == 4
    assert grp == [0, 1, 0, 2, 3, 0, 1]                             # groups in order of first appearance
    assert order == [0, 2, 5, 1, 6, 3, 4]                           # traces in the caller's order inside a group
    # equal n0 under another schedule, another schedule length or another r is another group; the empty schedule is a shape like any other
    shapes = [(64, [4, 2], 4), (64, [2, 4], 4), (64, [4, 2], 8), (64, [4], 4), (64, [], 4), (64, [4, 2], 4), (64, [], 4), (128, [4, 2], 4)]
    grp, order, ng = mp.groups_of(hostcheck, shapes)
    assert ng == 6 and grp == [0, 1, 2, 3, 4, 0, 4, 5]
    assert order == [0, 5, 1, 2, 3, 4, 6, 7]
    assert mp.groups_of(hostcheck, [(64, [4, 2], 4)]) == ([0], [0], 1)
