"""The lazy chain of the 8-round partial blocks on the device (poseidon_pair.hpp blk8_round_x / blk8_round_y, mfma_digits.hpp: wave Y hands H_q over as
its nine finish limbs with the next round's scaled constant in them, wave X adds them to the S-box output's limbs and never forms a field element inside
a block, y_q is posted recoded from the unreduced x5) at the smallest shapes the launchers send to the three wave-pair kernels WITHOUT any option:
k_leaf_pair2 from 4097 leaves, k_node16_pair for a level of 4097 full nodes, k_hash_ds2<17> (pair_permute_blk8, the same block internals) for 4100 nodes whose last
has 5 children.  Against the oracle and against the context option "poseidon_block8" = 0 (blocks of 4 on the vector ALU, untouched); an uploaded rf = 2
set (no fused product, a standalone squeeze S-box) and one steered level per uniform corner and per block position, every node against the reference's
dense rounds under the steered constants.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref
import scaled_chain_lib as sc
from test_gpu_partial_block8 import both_forms, leaves

pytestmark = pytest.mark.gpu
P = pyref.P_PALLAS
R = pyref.R
LEVEL, LABEL = 3, 42
LEAF0 = 4097                      # kCoopMaxLeaves + 1: the smallest leaf layer poseidon_form sends to the wave pair


@pytest.mark.parametrize("n", [LEAF0, LEAF0 + 1, LEAF0 + 65])      # 65 workgroups with one live lane in the last; two live lanes; 67 workgroups, the last with two
def test_leaf_kernel_equals_oracle_and_blocks_of_4(gpu_ctx, oracle, n):
    """k_leaf_pair2, m = 16, with f_next and without: every leaf against the oracle, both forms"""
    m = 16
    f = leaves(5200 + n, n); fn = leaves(6200 + n, (n + m - 1) // m)[::-1].copy()
    want = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    new, old = both_forms(gpu_ctx, lambda: (gpu_ctx.leaf_pair_hash(f, fn, m), gpu_ctx.leaf_pair_hash(f, None, m)))
    for got in (new, old):
        assert (got[0] == want).all(), np.nonzero((got[0] != want).any(axis=1))[0][:5]
        assert (got[1] == want_plain).all(), np.nonzero((got[1] != want_plain).any(axis=1))[0][:5]


@pytest.mark.parametrize("nodes,last", [(4097, None), (4100, 5)])        # k_node16_pair; a ragged last node of 5 children: k_hash_ds2<17>
def test_merkle_level_equals_oracle_and_blocks_of_4(gpu_ctx, oracle, nodes, last):
    p17 = gpu_ctx.poseidon_params_for_width(17)
    n_in = nodes * 16 if last is None else (nodes - 1) * 16 + last
    ch = oracle.synth_column(2300 + nodes, 5, 0, n_in)
    new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(p17, 16, 4, 77000, 11, ch))
    assert new.shape == (nodes, 4) and (new == old).all(), np.nonzero((new != old).any(axis=1))[0][:5]
    fe = oracle.from_u64
    for k in sorted({0, 1, 31, 32, 63, 64, 65, nodes // 2, 4095, 4096, nodes - 2, nodes - 1}):
        kids = ch[16 * k: 16 * k + 16]
        assert (new[k] == oracle.hash_with_ds_dynamic(0, 17, np.array([fe(16), fe(4), fe(77000 + k), fe(11)]), kids, kids.shape[0])).all(), k


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


@pytest.fixture(scope="module")
def rf2_set(base17):
    """the width-17 constants cut to TWO full rounds: half = rf - 1, so the chain's final value goes through the squeeze round's own S-box, not recoded"""
    return cv.params_arrays(dict(base17, rf=2, rc_full=base17["rc_full"][:2]))


@pytest.mark.parametrize("nodes,last", [(4097, None), (4100, 5)])
def test_two_full_rounds_merkle_level(gpu_ctx, hostcheck, oracle, rf2_set, nodes, last):
    """both level kernels under rf = 2: options 1 and 0 equal on every node; the level of full nodes also against the dense rounds on the host"""
    dev = gpu_ctx.params_upload(*rf2_set); h = hostcheck.params_upload(*rf2_set)
    try:
        assert b8.table(hostcheck, h, 0).shape[0] == 8
        n_in = nodes * 16 if last is None else (nodes - 1) * 16 + last
        ch = oracle.synth_column(2400 + nodes, 6, 0, n_in)
        new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(dev, 16, 2, 500, 7, ch))
        want = b8.dense_level16(hostcheck, h, oracle.from_u64, 2, 500, 7, ch) if last is None else None
    finally:
        dev.free(); hostcheck.params_free(h)
    assert new.shape == (nodes, 4) and (new == old).all(), np.nonzero((new != old).any(axis=1))[0][:5]
    if want is not None:
        assert (new == want).all(), np.nonzero((new != want).any(axis=1))[0][:5]


def steered_level_check(gpu_ctx, hostcheck, oracle, base17, nd, nodes, kstar):
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


@pytest.mark.parametrize("side", ["out", "in"])
@pytest.mark.parametrize("i", range(len(cv.uniform_corners(P))))
def test_steered_level_per_uniform_corner(gpu_ctx, hostcheck, oracle, base17, i, side):
    """A level of 4097 nodes (k_node16_pair) whose steered node has uniform corner i as the stored value the scaled chain's S-box delivers (out: the x5 that is
    recoded unreduced and whose limbs meet the slot's) or reads mod r (in) in all 64 rounds at once"""
    c = cv.uniform_corners(P)[i]
    lam = sc.lambdas(base17["mds"], base17["rp"]); Ri = pow(R, -1, P)
    if side == "out":
        tp = [c * pow(pow(lam[q], 5, P), -1, P) % P for q in range(base17["rp"])]
    else:
        tp = [cv.restored(pow(c * Ri % P * pow(lam[q], -1, P) % P, 5, P)) for q in range(base17["rp"])]
    nd = cv.steered_set(base17, ("scaled uniform", cv.target_schedules(base17)[i][1], tp), 1, 12300 + 31 * i + (0 if side == "out" else 7), LEVEL, LABEL)
    ins, outs = sc.scaled_chain_values(nd["params"], nd["state"])
    assert (outs if side == "out" else ins) == [c] * base17["rp"]
    steered_level_check(gpu_ctx, hostcheck, oracle, base17, nd, 4097, [0, 31, 32, 63, 64, 4095, 4096, 2049, 1][i])


@pytest.mark.parametrize("side", ["out", "in"])
@pytest.mark.parametrize("r", range(8))
def test_steered_level_per_block_position(gpu_ctx, hostcheck, oracle, base17, r, side):
    """A level of 4097 nodes under the steered sets of scaled_chain_lib.scaled_schedule: over r = 0..7 every non-uniform stored corner at every position of
    an 8-round block, delivered (out) or read (in) by the chain's S-box"""
    sched, corners = sc.scaled_schedule(base17, r, side)
    nd = cv.steered_set(base17, sched, 1, 9100 + 977 * r + (0 if side == "out" else 5), LEVEL, LABEL)
    ins, outs = sc.scaled_chain_values(nd["params"], nd["state"])
    assert (outs if side == "out" else ins) == corners
    steered_level_check(gpu_ctx, hostcheck, oracle, base17, nd, 4097, [0, 31, 32, 63, 64, 4095, 4096, 2049][r])
