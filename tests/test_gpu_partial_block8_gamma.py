"""The Gamma terms of the 8-round partial blocks as K-steps of the E rows' tiles (poseidon_pair.hpp pair_block8: row q of a block is one tile of
16 + q K-steps, no Gamma term on the vector ALU), on the device: the leaf kernel against the oracle on every leaf, the arity-16 level kernels against
the blocks of 4 (option "poseidon_block8" = 0) on every item and against the oracle on sampled nodes, and one steered level per uniform corner —
its constants put that corner behind all eight S-boxes of every block at once, so row 7's seven Gamma steps carry the same extreme digits together
(the windows of tests/test_gpu_partial_block8.py put a different corner at each position) — every node against the reference's dense rounds.
Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref
from test_gpu_partial_block8 import both_forms, leaves

pytestmark = pytest.mark.gpu
P = pyref.P_PALLAS
LEVEL, LABEL = 3, 42


@pytest.mark.parametrize("n", [65, 193])          # 65: two workgroups, 63 tail lanes; 193: four, one live lane in the last
def test_leaf_kernel_equals_oracle(gpu_ctx, oracle, n):
    """k_leaf_pair2 (option sponge_one_wave sends a leaf layer of any size to the wave pair): every leaf against the oracle"""
    m = 16
    f = leaves(5000 + n, n); fn = leaves(6000 + n, (n + m - 1) // m)[::-1].copy()
    want = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    try:
        gpu_ctx.set_option("sponge_one_wave", 1)
        got = gpu_ctx.leaf_pair_hash(f, fn, m); got_plain = gpu_ctx.leaf_pair_hash(f, None, m)
    finally:
        gpu_ctx.set_option("sponge_one_wave", 0)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (got_plain == want_plain).all(), np.nonzero((got_plain != want_plain).any(axis=1))[0][:5]


@pytest.mark.parametrize("nodes,last", [(4097, None), (4100, 5)])        # k_node16_pair; a ragged last node: k_hash_ds2<17>
def test_merkle_level_equals_blocks_of_4_and_oracle(gpu_ctx, oracle, nodes, last):
    p17 = gpu_ctx.poseidon_params_for_width(17)
    n_in = nodes * 16 if last is None else (nodes - 1) * 16 + last
    ch = oracle.synth_column(1900 + nodes, 3, 0, n_in)
    new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(p17, 16, 2, 1000, 9, ch))
    assert new.shape == (nodes, 4) and (new == old).all(), np.nonzero((new != old).any(axis=1))[0][:5]
    fe = oracle.from_u64
    for k in sorted({0, 1, 31, 32, 63, 64, 65, nodes // 2, 4095, 4096, nodes - 2, nodes - 1}):
        kids = ch[16 * k: 16 * k + 16]
        assert (new[k] == oracle.hash_with_ds_dynamic(0, 17, np.array([fe(16), fe(2), fe(1000 + k), fe(9)]), kids, kids.shape[0])).all(), k


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


@pytest.mark.parametrize("i", range(len(cv.uniform_corners(P))))
def test_steered_level_per_uniform_corner(gpu_ctx, hostcheck, oracle, base17, i):
    """A level of 4097 nodes (k_node16_pair) under the steered set of uniform corner i: the steered node's first permutation has that corner behind
    every S-box, so in every block y_0..y_7 are that one value and row 7 takes seven Gamma steps of it.  Every node against the reference's dense
    rounds under the same constants (partial_block8_lib.dense_level16), the steered node also against the digest pyref's construction predicts."""
    nodes, kstar = 4097, [0, 31, 32, 63, 64, 4095, 4096, 2049, 1][i]
    c = cv.uniform_corners(P)[i]
    nd = cv.steered_set(base17, cv.target_schedules(base17)[i], 1, 11000 + 977 * i, LEVEL, LABEL)
    _, op, _ = cv.sbox_outputs(nd["params"], nd["state"])
    assert op == [c] * base17["rp"] and base17["rp"] % 8 == 0
    arrays = cv.params_arrays(nd["params"])
    dev = gpu_ctx.params_upload(*arrays); h = hostcheck.params_upload(*arrays)
    try:
        assert b8.table(hostcheck, h, 0).shape[0] == base17["rp"] // 8
        ch, pos0 = cv.steered_level(base17, nd, nodes, kstar)
        got = gpu_ctx.hash_ds_level(dev, 16, LEVEL, pos0, LABEL, ch)
        want = b8.dense_level16(hostcheck, h, oracle.from_u64, LEVEL, pos0, LABEL, ch)
    finally:
        dev.free(); hostcheck.params_free(h)
    assert got.shape == (nodes, 4)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (got[kstar] == nd["digest"]).all(), (cv.hex_limbs(got[kstar]), cv.hex_limbs(nd["digest"]))
