"""The scaled S-box chain of the 8-round partial blocks on the device (poseidon_pair.hpp pair_block8: wave X carries lambda_q X_q, no a_q y_q
product in a round, one product by 1 / lambda_rp per permutation): k_leaf_pair2, k_node16_pair and k_hash_ds2<17> in the 8-round form at their
smallest shapes, against the oracle and against the context option "poseidon_block8" = 0 (blocks of 4 on the vector ALU, untouched); one steered
level per block position with the stored corners at the S-box of the scaled chain, every node against the reference's dense rounds.  The option
"merkle_wave_pair" sends Merkle levels of every size to the wave pair (as the FRI commit's side stream does), "sponge_one_wave" the small leaf
layers.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import corner_values as cv
import merkle_batch_cases as mc
import partial_block8_lib as b8
import pyref
import scaled_chain_lib as sc
from test_gpu_partial_block8 import both_forms, leaves

pytestmark = pytest.mark.gpu
P = pyref.P_PALLAS
LEVEL, LABEL = 3, 42
PAIR = {"merkle_wave_pair": (1, 0)}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])         # one live lane; one tail lane; a full workgroup; two and three workgroups
def test_leaf_kernel_equals_oracle_and_blocks_of_4(gpu_ctx, oracle, n):
    """k_leaf_pair2 (pair_permute_fused: the unscale in front of element 0's fused S-box), m = 16, with f_next and without"""
    m = 16
    f = leaves(5000 + n, n); fn = leaves(6000 + n, (n + m - 1) // m)[::-1].copy()
    want = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    new, old = both_forms(gpu_ctx, lambda: (gpu_ctx.leaf_pair_hash(f, fn, m), gpu_ctx.leaf_pair_hash(f, None, m)), {"sponge_one_wave": (1, 0)})
    for got in (new, old):
        assert (got[0] == want).all(), np.nonzero((got[0] != want).any(axis=1))[0][:5]
        assert (got[1] == want_plain).all(), np.nonzero((got[1] != want_plain).any(axis=1))[0][:5]


def oracle_level(oracle, ch, nodes, level, pos0, label):
    fe = oracle.from_u64
    return np.stack([oracle.hash_with_ds_dynamic(0, 17, np.array([fe(16), fe(level), fe(pos0 + k), fe(label)]), ch[16 * k:16 * k + 16], ch[16 * k:16 * k + 16].shape[0])
                     for k in range(nodes)])


@pytest.mark.parametrize("nodes", [1, 64, 65])
def test_node16_kernel_equals_oracle_and_blocks_of_4(gpu_ctx, oracle, nodes):
    """k_node16_pair: two permutations per node, each unscaled inside its last block"""
    p17 = gpu_ctx.poseidon_params_for_width(17)
    ch = oracle.synth_column(7100 + nodes, 3, 0, nodes * 16)
    new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(p17, 16, 2, 1000, 9, ch), PAIR)
    want = oracle_level(oracle, ch, nodes, 2, 1000, 9)
    assert new.shape == (nodes, 4)
    assert (new == want).all(), np.nonzero((new != want).any(axis=1))[0][:5]
    assert (old == want).all(), np.nonzero((old != want).any(axis=1))[0][:5]


@pytest.mark.parametrize("n_in", [17, 1041])                # 2 and 66 nodes, the last one of a single child: its lane sits out the first permutation
def test_ragged_level_equals_oracle_and_blocks_of_4(gpu_ctx, oracle, n_in):
    """k_hash_ds2<17, DsStream, true> (pair_permute_blk8: the unscale in front of the store of element 0) over a stream of two permutations, the dead
    permutation of the short node included: every permutation must be unscaled"""
    p17 = gpu_ctx.poseidon_params_for_width(17)
    nodes = (n_in + 15) // 16
    ch = oracle.synth_column(7200 + n_in, 3, 0, n_in)
    new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(p17, 16, 4, 77, 11, ch), PAIR)
    want = oracle_level(oracle, ch, nodes, 4, 77, 11)
    assert new.shape == (nodes, 4)
    assert (new == want).all(), np.nonzero((new != want).any(axis=1))[0][:5]
    assert (old == want).all(), np.nonzero((old != want).any(axis=1))[0][:5]


def test_batched_trees_equal_oracle_and_blocks_of_4(gpu_ctx, oracle):
    """two trees of 17 leaves through stark_merkle_build_batch_dev: k_hash_ds2<17> over the batch streams, ragged level and root"""
    from test_gpu_merkle_batch import dev
    arity, n, B, seed = 16, 17, 2, 0x5CA1
    fs = [mc.leaves_of(oracle, seed, b, n) for b in range(B)]; labels = mc.labels_of(B)
    fd = [dev(f) for f in fs]

    def build():
        trees = gpu_ctx.merkle_build_batch_dev([t.data_ptr() for t in fd], n, arity, labels, gpu_ctx.poseidon_params_for_arity(arity))
        try:
            return [[t.level(v).copy() for v in range(t.num_levels)] for t in trees]
        finally:
            for t in trees:
                t.free()
    new, old = both_forms(gpu_ctx, build, PAIR)
    for b in range(B):
        o = mc.oracle_tree(oracle, seed, b, arity, n, False, labels[b], False)
        assert len(new[b]) == len(old[b]) == o.num_levels()
        for v in range(o.num_levels()):
            assert (new[b][v] == o.level(v)).all() and (old[b][v] == o.level(v)).all(), (b, v)


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


@pytest.mark.parametrize("side", ["out", "in"])
@pytest.mark.parametrize("r", range(8))
def test_steered_level_per_block_position(gpu_ctx, hostcheck, oracle, base17, r, side):
    """A level of 65 nodes (k_node16_pair) under the steered sets of test_scaled_chain_host: window r of the stored corners delivered (out) or read
    (in) by the S-box of the scaled chain at every position of a block.  Every node against the reference's dense rounds under the same constants,
    with the option at 1 and at 0; the steered node also against the digest pyref's construction predicts."""
    nodes, kstar = 65, [0, 31, 32, 63, 64, 1, 33, 62][r]
    sched, corners = sc.scaled_schedule(base17, r, side)
    nd = cv.steered_set(base17, sched, 1, 9100 + 977 * r + (0 if side == "out" else 5), LEVEL, LABEL)
    ins, outs = sc.scaled_chain_values(nd["params"], nd["state"])
    assert (outs if side == "out" else ins) == corners
    arrays = cv.params_arrays(nd["params"])
    dev = gpu_ctx.params_upload(*arrays); h = hostcheck.params_upload(*arrays)
    try:
        assert sc.raw_table(hostcheck, h, 4).size == 8 * 8 * 16 * 1024
        ch, pos0 = cv.steered_level(base17, nd, nodes, kstar)
        new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(dev, 16, LEVEL, pos0, LABEL, ch), PAIR)
        want = b8.dense_level16(hostcheck, h, oracle.from_u64, LEVEL, pos0, LABEL, ch)
    finally:
        dev.free(); hostcheck.params_free(h)
    assert new.shape == (nodes, 4)
    assert (new == want).all(), np.nonzero((new != want).any(axis=1))[0][:5]
    assert (old == want).all(), np.nonzero((old != want).any(axis=1))[0][:5]
    assert (new[kstar] == nd["digest"]).all(), (cv.hex_limbs(new[kstar]), cv.hex_limbs(nd["digest"]))


def test_set_with_zero_m00_is_refused(gpu_ctx, base17):
    """M[0][0] = 0: no lambda.  stark_poseidon_params_upload refuses the set, as before (the in-place LU of M has no pivoting): no launcher ever sees
    a t = 17 set without its 8-round tables."""
    from stark_mlwe_amd.api import StarkError
    with pytest.raises(StarkError) as e:
        gpu_ctx.params_upload(*cv.params_arrays(sc.zero_m00_params(base17))).free()
    assert "singular leading minor" in str(e.value), str(e.value)
