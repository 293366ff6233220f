"""The limb-form hand-over of the t = 17 wave-pair kernels' full rounds (poseidon_pair.hpp pair_mds_sbox_mfma: a product row goes from its nine
finish limbs through the next round's S-box in the wave that formed it) at the smallest shapes that reach k_leaf_pair2, k_node16_pair and
k_hash_ds2<17> (which keeps canonical rows: it must still agree).  Context option "poseidon_block8" = 1 (the default; the two fixed-shape kernels take the
new hand-over) against 0 (the untouched form: canonical rows, standalone S-boxes, blocks of 4): equal on every item, every leaf and sampled nodes
against the oracle.  Then an uploaded set with rf = 2, where the one standalone S-box of the second half is the squeeze round's own and must not
be recoded: both forms against the host's dense rounds.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref

pytestmark = pytest.mark.gpu
P = pyref.P_PALLAS


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
def test_leaf_kernel_limb_handover_equals_oracle(gpu_ctx, oracle, n):
    """k_leaf_pair2 (option sponge_one_wave sends a leaf layer of any size to the wave pair), with and without f_next: every leaf against the oracle,
    the two forms equal on every leaf."""
    m = 16
    f = leaves(5100 + n, n); fn = leaves(6100 + n, (n + m - 1) // m)[::-1].copy()
    want = oracle.leaf_pair_hash(f, fn, m); want_plain = oracle.leaf_pair_hash(f, None, m)
    new, old = both_forms(gpu_ctx, lambda: (gpu_ctx.leaf_pair_hash(f, fn, m), gpu_ctx.leaf_pair_hash(f, None, m)), {"sponge_one_wave": (1, 0)})
    for a, b in zip(new, old):
        assert (a == b).all(), np.nonzero((a != b).any(axis=1))[0][:5]
    assert (new[0] == want).all(), np.nonzero((new[0] != want).any(axis=1))[0][:5]
    assert (new[1] == want_plain).all(), np.nonzero((new[1] != want_plain).any(axis=1))[0][:5]


@pytest.mark.parametrize("nodes,last", [(4097, None), (4100, 5)])        # k_node16_pair; a ragged last node of 5 children: k_hash_ds2<17>
def test_merkle_level_limb_handover_equals_oracle(gpu_ctx, oracle, nodes, last):
    p17 = gpu_ctx.poseidon_params_for_width(17)
    n_in = nodes * 16 if last is None else (nodes - 1) * 16 + last
    ch = oracle.synth_column(1700 + nodes, 5, 0, n_in)
    new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(p17, 16, 4, 77000, 11, ch))
    assert new.shape == (nodes, 4) and (new == old).all(), np.nonzero((new != old).any(axis=1))[0][:5]
    fe = oracle.from_u64
    for k in sorted({0, 1, 31, 32, 63, 64, 65, nodes // 2, 4095, 4096, nodes - 2, nodes - 1}):
        kids = ch[16 * k: 16 * k + 16]
        assert (new[k] == oracle.hash_with_ds_dynamic(0, 17, np.array([fe(16), fe(4), fe(77000 + k), fe(11)]), kids, kids.shape[0])).all(), k


@pytest.fixture(scope="module")
def rf2_set():
    """the width-17 constants cut to TWO full rounds (rp = 64 stays a multiple of 8, so the set gets its block-8 tables): half = rf - 1, the round after the
    partial rounds is the last one"""
    base = pyref.params_for_width(17)
    return cv.params_arrays(dict(base, rf=2, rc_full=base["rc_full"][:2]))


@pytest.mark.parametrize("nodes,last", [(4097, None), (4100, 5)])
def test_two_full_rounds_merkle_level(gpu_ctx, hostcheck, oracle, rf2_set, nodes, last):
    """k_node16_pair (its second permutation squeezes) and k_hash_ds2<17> under rf = 2 (the leaf kernel is defined over the transcript's own constants and
    refuses any other set, so it cannot meet this case): options 1 and 0 equal on every node; the level of full nodes also
    against the reference's dense rounds on the host (partial_block8_lib.dense_level16), every node."""
    dev = gpu_ctx.params_upload(*rf2_set); h = hostcheck.params_upload(*rf2_set)
    try:
        assert b8.table(hostcheck, h, 0).shape[0] == 8
        n_in = nodes * 16 if last is None else (nodes - 1) * 16 + last
        ch = oracle.synth_column(2200 + nodes, 6, 0, n_in)
        new, old = both_forms(gpu_ctx, lambda: gpu_ctx.hash_ds_level(dev, 16, 2, 500, 7, ch))
        want = b8.dense_level16(hostcheck, h, oracle.from_u64, 2, 500, 7, ch) if last is None else None
    finally:
        dev.free(); hostcheck.params_free(h)
    assert new.shape == (nodes, 4) and (new == old).all(), np.nonzero((new != old).any(axis=1))[0][:5]
    if want is not None:
        assert (new == want).all(), np.nonzero((new != want).any(axis=1))[0][:5]

