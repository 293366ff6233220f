"""The 8-round partial blocks of the t = 17 wave-pair kernels (poseidon_pair.hpp pair_block8: E-product and lane product on the matrix cores).
Context option "poseidon_block8" = 1 (the default) against 0 (blocks of 4 on the vector ALU): equal values on every item, the oracle on every
leaf and on sampled nodes, at the smallest shapes that reach k_leaf_pair2, k_node16_pair and k_hash_ds2<17>; then one steered level per position
of an 8-round block, every node against the reference's dense rounds under the steered constants.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref

pytestmark = pytest.mark.gpu
P = pyref.P_PALLAS
LEVEL, LABEL = 3, 42


def both_forms(ctx, fn, extra=None):
    """fn() with poseidon_block8 = 1 and = 0 (under the further options `extra`), the context's defaults restored whatever happens"""
    extra = extra or {}
    try:
        for k, (v, _) in extra.items():
            ctx.set_option(k, v)
        ctx.set_option("poseidon_block8", 1); new = fn()
        ctx.set_option("poseidon_block8", 0); old = fn()
    finally:
        ctx.set_option("poseidon_block8", 1)
        for k, (_, back) in extra.items():
            ctx.set_option(k, back)
    return new, old


def leaves(seed, n):
    """stored corners at the even positions, seeded random stored values at the odd ones"""
    rng = np.random.default_rng(seed)
    corners = cv.stored_corners(P)
    return cv.raw_array([corners[(i // 2) % len(corners)] if i % 2 == 0 else int.from_bytes(rng.bytes(32), "little") % P for i in range(n)])


@pytest.mark.parametrize("n", [65, 193])          # 65: two workgroups, 63 tail lanes; 193: four, one live lane in the last
def test_leaf_kernel_both_block_forms_equal_oracle(gpu_ctx, oracle, n):
    """k_leaf_pair2 at its smallest sizes (option sponge_one_wave sends a leaf layer of any size to the wave pair): every leaf against the oracle."""
    m = 16
    f = leaves(3000 + n, n); fn = leaves(4000 + n, (n + m - 1) // m)[::-1].copy()
    want = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    new, old = both_forms(gpu_ctx, lambda: (gpu_ctx.leaf_pair_hash(f, fn, m), gpu_ctx.leaf_pair_hash(f, None, m)), {"sponge_one_wave": (1, 0)})
    for got in (new, old):
        assert (got[0] == want).all(), np.nonzero((got[0] != want).any(axis=1))[0][:5]
        assert (got[1] == want_plain).all(), np.nonzero((got[1] != want_plain).any(axis=1))[0][:5]


@pytest.mark.parametrize("nodes,last", [(4097, None), (4100, 5)])        # k_node16_pair; a ragged last node: k_hash_ds2<17>
def test_merkle_level_both_block_forms_equal_oracle(gpu_ctx, oracle, nodes, last):
    p17 = gpu_ctx.poseidon_params_for_width(17)
    n_in = nodes * 16 if last is None else (nodes - 1) * 16 + last
    ch = oracle.synth_column(900 + nodes, 3, 0, n_in)
    new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(p17, 16, 2, 1000, 9, ch))
    assert new.shape == (nodes, 4) and (new == old).all(), np.nonzero((new != old).any(axis=1))[0][:5]
    fe = oracle.from_u64
    for k in sorted({0, 1, 31, 32, 63, 64, 65, nodes // 2, 4095, 4096, nodes - 2, nodes - 1}):
        kids = ch[16 * k: 16 * k + 16]
        assert (new[k] == oracle.hash_with_ds_dynamic(0, 17, np.array([fe(16), fe(2), fe(1000 + k), fe(9)]), kids, kids.shape[0])).all(), k


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


@pytest.mark.parametrize("r", range(8))
def test_steered_level_per_block_position(gpu_ctx, hostcheck, oracle, base17, r):
    """A level of 4097 nodes (k_node16_pair) under a steered set whose partial-round S-box outputs are chosen corners at every position of an
    8-round block (partial_block8_lib.block8_schedule): the WHOLE level against the reference's dense rounds under the same constants
    (dense_level16: hc_permute_dense, which reads M and the round constants and none of the kernel-form tables), with the option at 1 and at 0;
    the steered node also against the digest pyref's construction predicts, and eight other nodes against pyref itself (24 ms per node: the whole
    level through pyref would take minutes, so it pins the dense host reference on a sample and that reference checks every node).
    The uploaded set must be one the block form really serves: rp a multiple of 8 and non-empty block-8 tables (a set with rp % 8 == 0 whose
    tables are missing on the device is an error of the launcher, not a return to blocks of 4)."""
    nodes, kstar = 4097, [0, 31, 32, 63, 64, 4095, 4096, 2049][r]
    nd = cv.steered_set(base17, b8.block8_schedule(base17, r), 1, 9000 + 977 * r, LEVEL, LABEL)
    of, op, _ = cv.sbox_outputs(nd["params"], nd["state"])
    assert op == nd["tp"]                                   # the partial-round S-boxes deliver the scheduled corners
    assert nd["params"]["t"] == 17 and nd["params"]["rp"] % 8 == 0
    arrays = cv.params_arrays(nd["params"])
    dev = gpu_ctx.params_upload(*arrays); h = hostcheck.params_upload(*arrays)
    try:
        assert b8.table(hostcheck, h, 0).shape[0] == nd["params"]["rp"] // 8
        ch, pos0 = cv.steered_level(base17, nd, nodes, kstar)
        new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(dev, 16, LEVEL, pos0, LABEL, ch))
        want = b8.dense_level16(hostcheck, h, oracle.from_u64, LEVEL, pos0, LABEL, ch)
    finally:
        dev.free(); hostcheck.params_free(h)
    assert new.shape == (nodes, 4)
    assert (new == want).all(), np.nonzero((new != want).any(axis=1))[0][:5]
    assert (old == want).all(), np.nonzero((old != want).any(axis=1))[0][:5]
    assert (new[kstar] == nd["digest"]).all(), (cv.hex_limbs(new[kstar]), cv.hex_limbs(nd["digest"]))
    for k in sorted({0, 63, 64, 4032, 4095, 4096} | set(np.random.default_rng(r).integers(0, nodes, 3).tolist()) - {kstar})[:8]:
        assert (want[k] == cv.node_digest(nd["params"], LEVEL, pos0 + k, LABEL, ch[k * 16:(k + 1) * 16])).all(), k
