"""The byte-domain finish of the lanes between two 8-round blocks (poseidon_pair.hpp mfma_post_bytes in blk8_lane_rows: each lane folds the word columns it
holds, four 64-bit columns per tile cross the lane pair, one pass over eight words), on the device, at the smallest shapes that reach the two kernels
that run it: k_leaf_pair2<true> against the oracle on every leaf, k_node16_pair<true> against the oracle and against the blocks of 4 (option
"poseidon_block8" = 0), and steered levels — one per position of an 8-round block and one per uniform corner — every node against the reference's dense
rounds under the steered constants.  k_hash_ds2<17> keeps canonical lanes and is not touched.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref
from test_gpu_partial_block8 import both_forms, leaves

pytestmark = pytest.mark.gpu
P = pyref.P_PALLAS
LEVEL, LABEL = 3, 42


def test_leaf_kernel_65_leaves_equals_oracle(gpu_ctx, oracle):
    """stark_leaf_pair_hash_dev behind leaf_pair_hash, 65 leaves with m = 16: two workgroups, 63 tail lanes recomputing the last leaf (option
    sponge_one_wave sends a leaf layer of any size to the wave pair)"""
    n, m = 65, 16
    f = leaves(15000 + n, n); fn = leaves(16000 + n, (n + m - 1) // m)[::-1].copy()
    want = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    try:
        gpu_ctx.set_option("sponge_one_wave", 1)
        got = gpu_ctx.leaf_pair_hash(f, fn, m); got_plain = gpu_ctx.leaf_pair_hash(f, None, m)
    finally:
        gpu_ctx.set_option("sponge_one_wave", 0)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (got_plain == want_plain).all(), np.nonzero((got_plain != want_plain).any(axis=1))[0][:5]


def test_level_of_4097_nodes_equals_oracle_and_blocks_of_4(gpu_ctx, oracle):
    """the smallest level that reaches k_node16_pair: every node against the blocks of 4, and the oracle on the first, last and boundary nodes of the workgroups"""
    nodes = 4097
    p17 = gpu_ctx.poseidon_params_for_width(17)
    ch = oracle.synth_column(2900 + nodes, 3, 0, nodes * 16)
    new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(p17, 16, 2, 1000, 9, ch))
    assert new.shape == (nodes, 4) and (new == old).all(), np.nonzero((new != old).any(axis=1))[0][:5]
    fe = oracle.from_u64
    for k in sorted({0, 1, 31, 32, 63, 64, 65, nodes // 2, 4031, 4032, 4095, 4096}):          # the oracle takes 5 ms per node; the blocks of 4 cover every node
        kids = ch[16 * k: 16 * k + 16]
        assert (new[k] == oracle.hash_with_ds_dynamic(0, 17, np.array([fe(16), fe(2), fe(1000 + k), fe(9)]), kids, 16)).all(), k


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


def steered_level(gpu_ctx, hostcheck, oracle, base17, nd, kstar):
    nodes = 4097
    arrays = cv.params_arrays(nd["params"])
    dev = gpu_ctx.params_upload(*arrays); h = hostcheck.params_upload(*arrays)
    try:
        assert b8.table(hostcheck, h, 0).shape[0] == base17["rp"] // 8          # a set the block form really serves
        ch, pos0 = cv.steered_level(base17, nd, nodes, kstar)
        got = gpu_ctx.hash_ds_level(dev, 16, LEVEL, pos0, LABEL, ch)
        want = b8.dense_level16(hostcheck, h, oracle.from_u64, LEVEL, pos0, LABEL, ch)
    finally:
        dev.free(); hostcheck.params_free(h)
    assert got.shape == (nodes, 4)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (got[kstar] == nd["digest"]).all(), (cv.hex_limbs(got[kstar]), cv.hex_limbs(nd["digest"]))


@pytest.mark.parametrize("r", range(8))
def test_steered_level_per_block_position(gpu_ctx, hostcheck, oracle, base17, r):
    """chosen corners behind the S-box at every position of an 8-round block (partial_block8_lib.block8_schedule): the lane rows between the blocks take
    them as their eight y operands"""
    nd = cv.steered_set(base17, b8.block8_schedule(base17, r), 1, 13000 + 977 * r, LEVEL, LABEL)
    _, op, _ = cv.sbox_outputs(nd["params"], nd["state"])
    assert op == nd["tp"] and nd["params"]["rp"] % 8 == 0
    steered_level(gpu_ctx, hostcheck, oracle, base17, nd, [0, 31, 32, 63, 64, 4095, 4096, 2049][r])


@pytest.mark.parametrize("i", range(len(cv.uniform_corners(P))))
def test_steered_level_per_uniform_corner(gpu_ctx, hostcheck, oracle, base17, i):
    """uniform corner i behind all eight S-boxes of every block at once: every lane row's eight y operands carry the same extreme digits together"""
    c = cv.uniform_corners(P)[i]
    nd = cv.steered_set(base17, cv.target_schedules(base17)[i], 1, 14000 + 977 * i, LEVEL, LABEL)
    _, op, _ = cv.sbox_outputs(nd["params"], nd["state"])
    assert op == [c] * base17["rp"] and base17["rp"] % 8 == 0
    steered_level(gpu_ctx, hostcheck, oracle, base17, nd, [0, 31, 32, 63, 64, 4095, 4096, 2049, 1][i])
