"""The once-per-permutation edges of the t = 17 wave-pair kernels on the device (poseidon_pair.hpp): the leaf's round 0 as a two-K-step product handed to
round 1's S-box in limb form (pair_leaf_round0_mfma, k_leaf_pair2<true>) and the squeeze row as one matrix-core row in wave X (pair_squeeze_row_mfma, every
t = 17 wave-pair kernel), at the smallest shapes that reach each path: k_leaf_pair2<true> against the oracle on every leaf and against the blocks of 4 (option
"poseidon_block8" = 0, which keeps the closed form on the vector ALU), leaves whose x4 / x5 are the uniform corners, k_node16_pair<true> and k_hash_ds2<17>
levels, an uploaded rf = 2 set whose last block's lane rows feed the squeeze row directly, and steered levels that put the uniform corners behind the S-boxes
in front of the squeeze row and in front of the partial rounds.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref
from test_gpu_partial_block8 import both_forms, leaves

pytestmark = pytest.mark.gpu
P = pyref.P_PALLAS
R = pyref.R
LEVEL, LABEL = 3, 42


def first_diff(a, b):
    return np.nonzero((a != b).any(axis=1))[0][:5]


def check_leaves(gpu_ctx, oracle, f, fn, m, extra=None):
    """both forms of the leaf kernel, with and without f_next: the 8-round form equals the oracle on every leaf and equals the blocks of 4"""
    want = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    new, old = both_forms(gpu_ctx, lambda: (gpu_ctx.leaf_pair_hash(f, fn, m), gpu_ctx.leaf_pair_hash(f, None, m)), extra)
    assert (new[0] == want).all(), first_diff(new[0], want)
    assert (new[1] == want_plain).all(), first_diff(new[1], want_plain)
    assert (new[0] == old[0]).all() and (new[1] == old[1]).all()
    assert (want != want_plain).any()


def test_leaf_kernel_65_leaves(gpu_ctx, oracle):
    """65 leaves with m = 16 through option sponge_one_wave (it sends a leaf layer of any size to the wave pair): two workgroups, 63 tail lanes"""
    n, m = 65, 16
    f = leaves(27000 + n, n); fn = leaves(28000 + n, (n + m - 1) // m)[::-1].copy()
    check_leaves(gpu_ctx, oracle, f, fn, m, {"sponge_one_wave": (1, 0)})


@pytest.mark.parametrize("m", [16, 8])
def test_leaf_kernel_4162_leaves(gpu_ctx, oracle, m):
    """67 workgroups, the last with two live lanes, as the launcher sends them without any option"""
    n = 4162
    f = leaves(27000 + n + m, n); fn = leaves(28000 + n + m, (n + m - 1) // m)[::-1].copy()
    check_leaves(gpu_ctx, oracle, f, fn, m)


def test_leaf_kernel_uniform_corner_pairs_in_every_lane(gpu_ctx, oracle):
    """Leaves whose x4 and x5 — the two operands of round 0's rows — are uniform corners, placed by the fifth root.  One workgroup is 64 leaves; with m = 1 every
    leaf has its own f_next, and lane l of workgroup w takes corner pair (w + l) mod 81: over the 81 workgroups every pair of corners meets every lane, lanes
    0, 31, 32 and 63 (the ends of the two halves of the exchange) among them."""
    tp = hc_transcript_rc0()
    corners = cv.uniform_corners(P); nc = len(corners)
    pre4 = [cv.sbox_preimage(c, tp[4]) for c in corners]; pre5 = [cv.sbox_preimage(c, tp[5]) for c in corners]
    n = 64 * nc * nc
    pair = [((i // 64) + (i % 64)) % (nc * nc) for i in range(n)]
    for lane in (0, 31, 32, 63):
        assert {pair[64 * w + lane] for w in range(nc * nc)} == set(range(nc * nc))
    f = cv.raw_array([pre4[p // nc] for p in pair]); fn = cv.raw_array([pre5[p % nc] for p in pair])
    check_leaves(gpu_ctx, oracle, f, fn, 1)


def hc_transcript_rc0():
    """round 0's constants of the transcript set as stored integers"""
    import hostcheck_lib
    from test_limb_handover_host import SETS17
    hc = hostcheck_lib.HostCheck(); kind, seed = SETS17["transcript"]
    h = hc.params(kind, 17, seed)
    try:
        _, rcf, _ = hc.params_export(h, 17, 8, 64)
    finally:
        hc.params_free(h)
    return [cv.raw_to_int(x) for x in rcf[:17]]


@pytest.mark.parametrize("nodes,last", [(4097, None), (4100, 5)])        # k_node16_pair<true>; a ragged last node of 5 children: k_hash_ds2<17>, the squeeze of pair_permute_blk8
def test_merkle_level_equals_blocks_of_4_and_oracle(gpu_ctx, oracle, nodes, last):
    """every node against the blocks of 4, and the oracle on the first, last and workgroup-boundary nodes"""
    p17 = gpu_ctx.poseidon_params_for_width(17)
    n_in = nodes * 16 if last is None else (nodes - 1) * 16 + last
    ch = oracle.synth_column(4100 + nodes, 4, 0, n_in)
    new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(p17, 16, 2, 3000, 5, ch))
    assert new.shape == (nodes, 4) and (new == old).all(), first_diff(new, old)
    fe = oracle.from_u64
    for k in sorted({0, 31, 32, 63, 64, 4095, 4096, nodes - 1}):          # the oracle takes 5 ms per node
        kids = ch[16 * k: 16 * k + 16]
        assert (new[k] == oracle.hash_with_ds_dynamic(0, 17, np.array([fe(16), fe(2), fe(3000 + k), fe(5)]), kids, kids.shape[0])).all(), k


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


def test_two_full_rounds_level_equals_host(gpu_ctx, hostcheck, oracle, base17):
    """an uploaded rf = 2 set: the last block's lane rows and the chain's final value go through the squeeze round's S-box and feed the squeeze row directly;
    every node of a 4097-node level against the dense rounds on the host"""
    arrays = cv.params_arrays(dict(base17, rf=2, rc_full=base17["rc_full"][:2]))
    dev = gpu_ctx.params_upload(*arrays); h = hostcheck.params_upload(*arrays)
    try:
        assert b8.table(hostcheck, h, 0).shape[0] == 8
        ch = oracle.synth_column(4200, 6, 0, 4097 * 16)
        got = gpu_ctx.hash_ds_level(dev, 16, 2, 500, 7, ch)
        want = b8.dense_level16(hostcheck, h, oracle.from_u64, 2, 500, 7, ch)
    finally:
        dev.free(); hostcheck.params_free(h)
    assert got.shape == (4097, 4) and (got == want).all(), first_diff(got, want)


@pytest.mark.parametrize("i", range(len(cv.uniform_corners(P))))
def test_steered_level_corners_at_the_squeeze_and_the_entry(gpu_ctx, hostcheck, oracle, base17, i):
    """Steered constants (corner_values.steered_set, both permutations of a full node) that put uniform corner i behind every S-box of the LAST full round —
    the squeeze row's 17 operands carry the same extreme digits together (element 16 is the one target the construction fixes) — and behind every S-box of
    round rf / 2 - 1, the operands of the rows that enter the partial rounds; the other rounds follow the first rotation of the other corners.  Every node of a
    4097-node level against the dense rounds under the steered constants, the steered node against its digest."""
    c = cv.uniform_corners(P)[i]; rf, t = base17["rf"], base17["t"]
    _, tf, tp = next(s for s in cv.target_schedules(base17) if s[0].startswith("rotation"))
    tf = [list(r) for r in tf]; tf[rf - 1] = [c] * t; tf[rf // 2 - 1] = [c] * t
    nd = cv.steered_set(base17, ("corner %d at the squeeze and the entry" % i, tf, tp), 2, 26000 + 977 * i, LEVEL, LABEL)
    of, _, _ = cv.sbox_outputs(nd["params"], nd["state"])
    assert of[rf - 1][:t - 1] == [c] * (t - 1) and of[rf // 2 - 1] == [c] * t and of == nd["tf"]
    nodes = 4097; kstar = [0, 31, 32, 63, 64, 4095, 4096, 2049, 1][i]
    arrays = cv.params_arrays(nd["params"])
    dev = gpu_ctx.params_upload(*arrays); h = hostcheck.params_upload(*arrays)
    try:
        assert b8.table(hostcheck, h, 0).shape[0] == base17["rp"] // 8          # a set the block form really serves
        ch, pos0 = cv.steered_level(base17, nd, nodes, kstar)
        got = gpu_ctx.hash_ds_level(dev, 16, LEVEL, pos0, LABEL, ch)
        want = b8.dense_level16(hostcheck, h, oracle.from_u64, LEVEL, pos0, LABEL, ch)
    finally:
        dev.free(); hostcheck.params_free(h)
    assert got.shape == (nodes, 4) and (got == want).all(), first_diff(got, want)
    assert (got[kstar] == nd["digest"]).all(), (cv.hex_limbs(got[kstar]), cv.hex_limbs(nd["digest"]))
