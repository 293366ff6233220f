"""The Merkle climb written once (csrc/merkle_batch.hpp merkle_climb / merkle_climb_ragged) under every driver that runs it, at the smallest shapes
where a climb can go wrong, and the two pair-leaf batch streams (DsBatchPairPtrStream behind pointer tables, DsBatchPairStream at a pitch) against
each other where their shapes coincide.  Needs an MI355X (`pytest -m gpu`)."""
import functools

import numpy as np
import pytest

import merkle_batch_cases as mc
import pyref
from test_gpu_merkle_batch import build_batch, dev

pytestmark = pytest.mark.gpu

KS = (0, 1, 4, 5, 9)                     # 2^k leaves under arity 16: one leaf, one ragged node, one full node, a ragged root over two nodes, three levels
SEED_Z = 0xDEEFBAAD


@functools.lru_cache(maxsize=None)
def witnesses(oracle):
    """three witnesses per size under distinct labels, and the root of MerkleCommitment::commit of each by pyref (computed once, left unchanged)"""
    X5 = pyref.derive_params(b"POSEIDON-T17-X5-SEED", 17, 8, 64)                                     # commitment/src/lib.rs:48-51
    ws, ks, labels, roots = [], [], [], []
    for k in KS:
        for i, w in enumerate(oracle.rand_fr_columns(0xC11B + k, 1 << k, 3)):
            cur = [pyref.from_limbs(r) for r in w]; label = 3000 + 10 * k + i; level = 0
            while len(cur) > 1:                                                                      # merkle/src/lib.rs:163-179, arity 16
                cur = [pyref.hash_with_ds_dynamic([16, level, j, label], cur[16 * j:16 * j + 16], X5) for j in range((len(cur) + 15) // 16)]; level += 1
            ws.append(w); ks.append(k); labels.append(label); roots.append(cur[0])
    assert len(set(labels)) == len(labels)
    return ws, ks, labels, roots


def test_every_driver_climbs_to_the_same_root(gpu_ctx, oracle):
    """the root inside each proof of stark_sumcheck_prove_plain_batch_dev = the root of stark_commitment_commit_batch_dev on that witness and label =
    pyref; then all fifteen witnesses in ONE stark_sumcheck_prove_plain_mixed_batch_dev call against stark_commitment_commit_mixed_batch_dev and pyref"""
    ws, ks, labels, want = witnesses(oracle)
    td = [dev(w) for w in ws]; ptrs = [t.data_ptr() for t in td]
    for k in KS:
        sel = [i for i in range(len(ks)) if ks[i] == k]
        proofs = gpu_ctx.prove_plain_batch_dev(k, [labels[i] for i in sel], [ptrs[i] for i in sel])
        trees = gpu_ctx.commitment_commit_batch_dev([labels[i] for i in sel], [ptrs[i] for i in sel], 1 << k)
        roots = gpu_ctx.merkle_roots_batch(trees)
        for j, i in enumerate(sel):
            assert pyref.parse_proof_plain(proofs[j])["root"] == want[i], "prove_plain_batch, k = %d, witness %d" % (k, j)
            assert pyref.from_limbs(roots[j]) == want[i], "commitment_commit_batch, k = %d, witness %d" % (k, j)
            assert trees[j].num_levels == len(mc_level_lens(1 << k)), (k, j)
    proofs = gpu_ctx.prove_plain_mixed_batch_dev(list(ks), labels, ptrs)
    trees = gpu_ctx.commitment_commit_mixed_batch_dev(labels, ptrs, [1 << k for k in ks])
    roots = gpu_ctx.merkle_roots_batch(trees)
    for i in range(len(ks)):
        assert pyref.parse_proof_plain(proofs[i])["root"] == want[i], "prove_plain_mixed_batch, witness %d (k = %d)" % (i, ks[i])
        assert pyref.from_limbs(roots[i]) == want[i], "commitment_commit_mixed_batch, witness %d (k = %d)" % (i, ks[i])


def mc_level_lens(n, arity=16):
    lens = [n]
    while lens[-1] > 1:
        lens.append(-(-lens[-1] // arity))
    return lens


@pytest.mark.parametrize("arity", [4, 2])
def test_pair_leaves_behind_pointers_equal_the_oracle(gpu_ctx, oracle, arity):
    """stark_merkle_build_batch_dev with pairs = 1 — the pair leaves behind pointer tables — of three trees of n = 1, 2, 5 and 8 leaves, the last tree's
    second column null: every level of every tree equals the oracle's MerkleTree::new_pairs"""
    B = 3; labels = mc.labels_of(B)
    for n in (1, 2, 5, 8):
        fs = [mc.leaves_of(oracle, 0x9A1, b, n) for b in range(B)]
        cps = [mc.leaves_of(oracle, 0x9A1, b + 100, n) for b in range(B - 1)] + [None]
        fd = [dev(f) for f in fs]; cd = [None if c is None else dev(c) for c in cps]
        trees = build_batch(gpu_ctx, arity, labels, fd, n, cd)
        for b in range(B):
            o = oracle.merkle_build(arity, labels[b], fs[b], np.zeros((n, 4), np.uint64) if cps[b] is None else cps[b])
            assert trees[b].num_levels == o.num_levels() == len(mc_level_lens(n, arity)), (arity, n, b)
            for v in range(o.num_levels()):
                assert (trees[b].level(v) == o.level(v)).all(), "arity %d, n = %d, tree %d, level %d" % (arity, n, b, v)
            o.free()


@pytest.mark.parametrize("n0, m", [(8, 4), (8, 2), (16, 2), (4, 2)])
def test_pair_leaves_at_a_pitch_equal_those_behind_pointers(gpu_ctx, oracle, n0, m):
    """where the shapes coincide: the two unhashed layers of stark_fri_commit_batch_dev over three traces of n0 rows under schedule [m] — layer 0, pair
    leaves (f_0[i], f_1[i / m]) at a pitch with cp_div = m under arity 4 (m = 4) or 2; layer 1, the last: arity 2, zero partners — against
    stark_merkle_build_batch_dev with pairs = 1 over the same columns under the labels 0 and 1 (layer 0's second column written out, layer 1's null).
    The commit hands out the top level of each tree, its root: that level is compared, and the build's every level with the oracle's"""
    B = 3; n1 = n0 // m
    f0 = [mc.leaves_of(oracle, 0x9A2 + n0 + m, b, n0) for b in range(B)]
    z0 = gpu_ctx.fri_sample_z_ell(SEED_Z, 0, n0)
    f1 = [gpu_ctx.fri_fold_layer(f, z0, m) for f in f0]
    fd = [dev(f) for f in f0]
    roots = gpu_ctx.fri_commit_batch_dev([t.data_ptr() for t in fd], n0, [m], SEED_Z)                # (B, 2, 4)
    layers = [(0, 4 if m == 4 else 2, n0, f0, [np.repeat(f, m, axis=0) for f in f1], False), (1, 2, n1, f1, [np.zeros((n1, 4), np.uint64)] * B, True)]
    for l, arity, n, fs, cps, null_cp in layers:
        cols = [dev(f) for f in fs]; cd = [None if null_cp else dev(c) for c in cps]
        trees = build_batch(gpu_ctx, arity, [l] * B, cols, n, cd)
        got = gpu_ctx.merkle_roots_batch(trees)
        for b in range(B):
            o = oracle.merkle_build(arity, l, fs[b], cps[b])
            for v in range(o.num_levels()):
                assert (trees[b].level(v) == o.level(v)).all(), "layer %d (arity %d, n = %d), trace %d, level %d" % (l, arity, n, b, v)
            assert (got[b] == roots[b, l]).all() and (got[b] == o.root()).all(), "layer %d (arity %d, n = %d), trace %d: the roots" % (l, arity, n, b)
            o.free()
