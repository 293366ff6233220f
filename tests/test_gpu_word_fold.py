"""The word-column finish to nine limbs on the device (poseidon_pair.hpp mfma_post_limbs: each lane folds the word columns it holds by a multiply-add chain,
four 64-bit columns per tile cross the lane pair, one pass over eight words, the nine limbs for the S-box) in the rows that run it — the fused full-round
rows, the H_q rows of the 8-round blocks and the last block's lane rows — at the smallest shapes that reach the three wave-pair kernels: k_leaf_pair2<true>
against the oracle on every leaf, k_node16_pair<true> against the oracle and the blocks of 4 (option "poseidon_block8" = 0), k_hash_ds2<17> on a level with a
ragged last node, an uploaded rf = 2 set against the host's dense rounds, and steered levels — one per position of an 8-round block and one per uniform
corner — every node against the dense rounds under the steered constants.  Needs an MI355X: `pytest -m gpu`."""
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
    """65 leaves with m = 16 through option sponge_one_wave (it sends a leaf layer of any size to the wave pair): two workgroups, 63 tail lanes"""
    n, m = 65, 16
    f = leaves(17000 + n, n); fn = leaves(18000 + n, (n + m - 1) // m)[::-1].copy()
    want = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    try:
        gpu_ctx.set_option("sponge_one_wave", 1)
        got = gpu_ctx.leaf_pair_hash(f, fn, m); got_plain = gpu_ctx.leaf_pair_hash(f, None, m)
    finally:
        gpu_ctx.set_option("sponge_one_wave", 0)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (got_plain == want_plain).all(), np.nonzero((got_plain != want_plain).any(axis=1))[0][:5]


def test_leaf_kernel_4162_leaves_equals_oracle(gpu_ctx, oracle):
    """67 workgroups, the last with two live lanes, as the launcher sends them without any option"""
    n, m = 4162, 16
    f = leaves(17000 + n, n); fn = leaves(18000 + n, (n + m - 1) // m)[::-1].copy()
    want = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    got = gpu_ctx.leaf_pair_hash(f, fn, m); got_plain = gpu_ctx.leaf_pair_hash(f, None, m)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (got_plain == want_plain).all(), np.nonzero((got_plain != want_plain).any(axis=1))[0][:5]


@pytest.mark.parametrize("nodes,last", [(4097, None), (4100, 5)])        # k_node16_pair<true>; a ragged last node of 5 children: k_hash_ds2<17>
def test_merkle_level_equals_blocks_of_4_and_oracle(gpu_ctx, oracle, nodes, last):
    """every node against the blocks of 4, and the oracle on the first, last and workgroup-boundary nodes"""
    p17 = gpu_ctx.poseidon_params_for_width(17)
    n_in = nodes * 16 if last is None else (nodes - 1) * 16 + last
    ch = oracle.synth_column(3100 + nodes, 4, 0, n_in)
    new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(p17, 16, 2, 3000, 5, ch))
    assert new.shape == (nodes, 4) and (new == old).all(), np.nonzero((new != old).any(axis=1))[0][:5]
    fe = oracle.from_u64
    for k in sorted({0, 1, 31, 32, 63, 64, 65, nodes // 2, 4031, 4032, 4095, 4096, nodes - 1}):          # the oracle takes 5 ms per node
        kids = ch[16 * k: 16 * k + 16]
        assert (new[k] == oracle.hash_with_ds_dynamic(0, 17, np.array([fe(16), fe(2), fe(3000 + k), fe(5)]), kids, kids.shape[0])).all(), k


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


def test_two_full_rounds_level_equals_host(gpu_ctx, hostcheck, oracle, base17):
    """an uploaded rf = 2 set: no fused product — the last block's lane rows and the chain's final value feed the squeeze round's own S-box; every node of a
    4097-node level against the dense rounds on the host"""
    arrays = cv.params_arrays(dict(base17, rf=2, rc_full=base17["rc_full"][:2]))
    dev = gpu_ctx.params_upload(*arrays); h = hostcheck.params_upload(*arrays)
    try:
        assert b8.table(hostcheck, h, 0).shape[0] == 8
        ch = oracle.synth_column(3200, 6, 0, 4097 * 16)
        got = gpu_ctx.hash_ds_level(dev, 16, 2, 500, 7, ch)
        want = b8.dense_level16(hostcheck, h, oracle.from_u64, 2, 500, 7, ch)
    finally:
        dev.free(); hostcheck.params_free(h)
    assert got.shape == (4097, 4) and (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]


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
    """chosen corners behind the S-box at every position of an 8-round block (partial_block8_lib.block8_schedule): the H_q rows take them as their Gamma
    operands, the last block's lane rows as their eight y operands"""
    nd = cv.steered_set(base17, b8.block8_schedule(base17, r), 1, 15000 + 977 * r, LEVEL, LABEL)
    _, op, _ = cv.sbox_outputs(nd["params"], nd["state"])
    assert op == nd["tp"] and nd["params"]["rp"] % 8 == 0
    steered_level(gpu_ctx, hostcheck, oracle, base17, nd, [0, 31, 32, 63, 64, 4095, 4096, 2049][r])


@pytest.mark.parametrize("i", range(len(cv.uniform_corners(P))))
def test_steered_level_per_uniform_corner(gpu_ctx, hostcheck, oracle, base17, i):
    """uniform corner i behind all eight S-boxes of every block at once: every row's y operands carry the same extreme digits together"""
    c = cv.uniform_corners(P)[i]
    nd = cv.steered_set(base17, cv.target_schedules(base17)[i], 1, 16000 + 977 * i, LEVEL, LABEL)
    _, op, _ = cv.sbox_outputs(nd["params"], nd["state"])
    assert op == [c] * base17["rp"] and base17["rp"] % 8 == 0
    steered_level(gpu_ctx, hostcheck, oracle, base17, nd, [0, 31, 32, 63, 64, 4095, 4096, 2049, 1][i])
