"""k_leaf_pair2 (the wave-pair leaf kernel, whose full rounds run on the matrix cores through the residue tables) at the smallest sizes that reach
it: under the context option "sponge_one_wave" a leaf layer of any size takes the wave pair.  Against the oracle's hash_leaf_pair on every leaf."""
import numpy as np
import pytest

import corner_values as cv
import pyref

pytestmark = pytest.mark.gpu
P = pyref.P_PALLAS


def leaves(seed, n):
    """stored corners at the even positions (rotating through the whole family), seeded random stored values at the odd ones"""
    rng = np.random.default_rng(seed)
    corners = cv.stored_corners(P)
    vals = [corners[(i // 2) % len(corners)] if i % 2 == 0 else int.from_bytes(rng.bytes(32), "little") % P for i in range(n)]
    return cv.raw_array(vals)


@pytest.mark.parametrize("n", [65, 193])          # 65: two workgroups, 63 tail lanes recomputing the last leaf; 193: four, one live lane in the last
def test_wave_pair_leaf_kernel_equals_oracle_at_its_smallest_sizes(gpu_ctx, oracle, n):
    m = 16
    f = leaves(1000 + n, n); fn = leaves(2000 + n, (n + m - 1) // m)[::-1].copy()
    want_next = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    try:
        gpu_ctx.set_option("sponge_one_wave", 1)
        got_next = gpu_ctx.leaf_pair_hash(f, fn, m); got_plain = gpu_ctx.leaf_pair_hash(f, None, m)
    finally:
        gpu_ctx.set_option("sponge_one_wave", 0)          # the option has no getter; 0 is the context's default and what every other test leaves behind
    assert got_next.shape == want_next.shape and (got_next == want_next).all(), np.nonzero((got_next != want_next).any(axis=1))[0][:5]
    assert (got_plain == want_plain).all(), np.nonzero((got_plain != want_plain).any(axis=1))[0][:5]
    assert (want_next != want_plain).any()
