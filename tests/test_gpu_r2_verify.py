"""N3 on the GPU: the library's verifier entry points (capi_verify.hip: the walks of fri_verify.hpp planned as a batch of one and run by the
batch runner on the prover's kernels) against the oracle's restatement of deep_fri_verify / verify_many_ds / verify_pairs_ds, on proofs the GPU prover made.
Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import merkle_batch_cases as mc
from stark_mlwe_amd.api import DeepFriParams, StarkError


@pytest.mark.parametrize("n0,sched,r", [(1 << 10, [16, 8], 8), (1 << 11, [16, 16, 8], 32), (1 << 9, [8, 4, 2], 5), (1 << 10, [32, 32], 40), (1 << 12, [64, 64], 6), (2, [2], 1)])
def test_gpu_verifier_accepts_gpu_proofs_and_agrees_with_oracle_under_tampering(gpu_ctx, oracle, n0, sched, r):
    cols = oracle.rand_fr_columns(2025 + n0, n0, 4)
    prm = DeepFriParams(sched, r, 0xDEEFBAAD)
    proof, _, _ = gpu_ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, prm)
    assert gpu_ctx.deep_fri_verify(prm, proof) is True
    assert oracle.deep_fri_verify(proof, sched, r, 0xDEEFBAAD) == 1
    assert gpu_ctx.deep_fri_verify(DeepFriParams(sched, r + 1, 0xDEEFBAAD), proof) is False
    assert gpu_ctx.deep_fri_verify(DeepFriParams(sched[:-1], r, 0xDEEFBAAD), proof) is False
    for bad in (b"", proof[:-1], proof + b"\0"):
        assert gpu_ctx.deep_fri_verify(prm, bad) is False
    rng = random.Random(n0 * 31 + r)
    positions = sorted(set([8, 8 + 31, 41, len(proof) - 1, len(proof) - 41] + [rng.randrange(len(proof)) for _ in range(40)]))
    rejected = 0
    for pos in positions:
        bad = bytearray(proof); bad[pos] ^= 1 << rng.randrange(8)
        want = oracle.deep_fri_verify(bytes(bad), sched, r, 0xDEEFBAAD) == 1
        got = gpu_ctx.deep_fri_verify(prm, bytes(bad))
        assert got == want, f"byte {pos}: library {got}, oracle {want}"
        rejected += not got
    assert rejected >= len(positions) // 2


def test_gpu_verifier_at_bench_size(gpu_ctx, oracle):
    """A 2^20-row proof (r = 32, [16,16,8]) made on the GPU from a synthetic f0: accepted by the library's verifier and by the
    oracle's; one flipped bit in the middle is rejected by both."""
    import torch
    n0, sched, r = 1 << 20, [16, 16, 8], 32
    f0 = torch.empty((n0, 4), dtype=torch.int64, device="cuda")
    gpu_ctx._chk(gpu_ctx.lib.stark_synth_column_dev(gpu_ctx.h, 0x5EED0014, 5, 0, n0, C.c_void_p(f0.data_ptr())))
    sch = np.ascontiguousarray(sched, dtype=np.uint64); h = C.c_void_p()
    gpu_ctx._chk(gpu_ctx.lib.stark_deep_fri_prove_dev(gpu_ctx.h, None, None, None, None, C.c_void_p(f0.data_ptr()), n0, sch.ctypes.data_as(C.c_void_p), 3, r, 0xDEEFBAAD, C.byref(h)))
    proof, _ = gpu_ctx._proof_out(h)
    prm = DeepFriParams(sched, r, 0xDEEFBAAD)
    assert gpu_ctx.deep_fri_verify(prm, proof) is True and oracle.deep_fri_verify(proof, sched, r, 0xDEEFBAAD) == 1
    bad = bytearray(proof); bad[len(bad) // 2] ^= 0x10
    assert gpu_ctx.deep_fri_verify(prm, bytes(bad)) is False and oracle.deep_fri_verify(bytes(bad), sched, r, 0xDEEFBAAD) == 0


@pytest.mark.parametrize("arity,n,label", [(16, 4096, 0), (16, 55, 9), (8, 19, 3), (2, 8, 1), (4, 64, 7), (32, 1024, 4), (128, 300, 2)])
def test_merkle_commit_open_verify_roundtrip_on_gpu(gpu_ctx, oracle, arity, n, label):
    """merkle/src/lib.rs:1053-1136: commit -> open_many -> verify_single is true; tampering a leaf / the root / the label / the
    proof bytes / the index set makes it false (MerkleProver facade through the C-ABI)."""
    leaves = oracle.synth_column(61, arity, 0, n)
    cfg = gpu_ctx.merkle_cfg(arity, label)
    t = gpu_ctx.merkle_new(leaves, cfg)
    rng = random.Random(n + arity); idx = sorted(set(rng.randrange(n) for _ in range(9)))
    pr = t.open_many(idx); root = t.root(); t.free()
    vals = leaves[idx]
    assert gpu_ctx.merkle_verify_single(cfg, root, idx, vals, pr) is True
    bad = vals.copy(); bad[-1, 3] ^= np.uint64(1)
    assert gpu_ctx.merkle_verify_single(cfg, root, idx, bad, pr) is False
    assert gpu_ctx.merkle_verify_single(cfg.with_tree_label(label + 1), root, idx, vals, pr) is False
    r2 = root.copy(); r2[0] ^= np.uint64(1)
    assert gpu_ctx.merkle_verify_single(cfg, r2, idx, vals, pr) is False
    assert gpu_ctx.merkle_verify_single(cfg, root, idx[1:], vals[1:], pr) is False
    b = bytearray(pr); b[len(pr) - 9] ^= 1                          # last group-size byte / arity word region
    assert gpu_ctx.merkle_verify_single(cfg, root, idx, vals, bytes(b)) is False
    with pytest.raises(StarkError):
        gpu_ctx.merkle_verify_single(gpu_ctx.merkle_cfg(arity, label).__class__(129, None, 0), root, idx, vals, pr)     # MerkleChannelCfg::new(129) panics


@pytest.mark.parametrize("arity,n", [(2, 8), (2, 2), (16, 64), (8, 32)])
def test_merkle_pairs_commit_open_verify_roundtrip_on_gpu(gpu_ctx, oracle, arity, n):
    """merkle/src/lib.rs:1138-1168 (commit_pairs / open_pairs / verify_pairs)."""
    f = oracle.synth_column(62, 0, 0, n); cp = oracle.synth_column(62, 1, 0, n)
    cfg = gpu_ctx.merkle_cfg(arity, 5)
    t = gpu_ctx.merkle_new_pairs(f, cp, cfg)
    idx = sorted({0, n - 1, n // 2})
    pr = t.open_many(idx); root = t.root(); t.free()
    assert gpu_ctx.merkle_verify_pairs(cfg, root, idx, f[idx], cp[idx], pr) is True
    bad = f[idx].copy(); bad[0, 0] ^= np.uint64(4)
    assert gpu_ctx.merkle_verify_pairs(cfg, root, idx, bad, cp[idx], pr) is False
    assert gpu_ctx.merkle_verify_pairs(cfg.with_tree_label(6), root, idx, f[idx], cp[idx], pr) is False
    assert gpu_ctx.merkle_verify_single(cfg, root, idx, f[idx], pr) is False


# ---- the six single entry points: each plans a batch of one and takes the batch runner ---------------------------------------------------
_vp = C.c_void_p


def _u8(b):
    return (C.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0")


def _w(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _flip(b, pos, bit=0x10):
    x = bytearray(b); x[pos] ^= bit; return bytes(x)


def _deep_fri_subject(ctx, oracle):
    """-> (call(h, proof, acc), [(proof, the oracle's decision)]): honest and one flipped bit (in roots[0]) of the smallest shape and of a shape
    with two Poseidon widths at one depth (arities 8 and 2 under [8, 4, 2]: the fork / join of verify_batch_groups_on)"""
    seed_z, rows, keep = 0xDEEFBAAD, [], []
    for n0, sched, r in ((2, [2], 1), (1 << 9, [8, 4, 2], 5)):
        cols = oracle.rand_fr_columns(4242 + n0, n0, 4)
        proof, _, _ = ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, seed_z))
        sch = _w(sched); keep.append(sch)
        for p in (proof, _flip(proof, 11)):
            rows.append(((sch, r), p, oracle.deep_fri_verify(p, sched, r, seed_z) == 1))
    def call(h, row, proof, acc):
        sch, r = row if row else (keep[0], 1)
        return ctx.lib.stark_deep_fri_verify(h, _u8(proof), len(proof), sch.ctypes.data_as(_vp), len(sch), r, seed_z, acc)
    return call, rows


def _merkle_subject(pairs):
    def make(ctx, oracle):
        arity, n, label = (2, 2, 5) if pairs else (2, 8, 1)
        f = oracle.synth_column(71, 0, 0, n); cp = oracle.synth_column(71, 1, 0, n)
        cfg = ctx.merkle_cfg(arity, label)
        t = ctx.merkle_new_pairs(f, cp, cfg) if pairs else ctx.merkle_new(f, cfg)
        idx = [0, n - 1] if pairs else [1, n - 2]
        pr = t.open_many(idx); root = _w(t.root()); t.free()
        ix = _w(idx); v = _w(f[idx]); c = _w(cp[idx]); cbad = mc.flip_bit(c, 5, 9)
        if pairs:
            rows = [((v, c), pr, mc.oracle_verify_pairs(arity, label, root, idx, v, c, pr) == 1), ((v, cbad), pr, mc.oracle_verify_pairs(arity, label, root, idx, v, cbad, pr) == 1)]
        else:
            bad = _flip(pr, mc.sibling_offset(idx) + 3)
            rows = [((v, c), p, mc.oracle_verify(arity, label, root, idx, v, p) == 1) for p in (pr, bad)]
        def call(h, row, proof, acc):
            vv, cc = row if row else (v, c)
            a = (h, arity, label, root.ctypes.data_as(_vp), ix.ctypes.data_as(_vp), len(ix), vv.ctypes.data_as(_vp))
            if pairs:
                return ctx.lib.stark_merkle_verify_pairs_ds(*a, cc.ctypes.data_as(_vp), _u8(proof), len(proof), acc)
            return ctx.lib.stark_merkle_verify_many_ds(*a, _u8(proof), len(proof), acc)
        return call, rows
    return make


def _commitment_subject(ctx, oracle):
    n, ds = 17, 77                                                           # arity 16: a two-level tree with a ragged top
    leaves = oracle.synth_column(72, 0, 0, n); idx = [0, 16]
    root, t = ctx.commitment_commit(ds, leaves); pr = t.open_many(idx); t.free()
    o = oracle.merkle_build(16, ds, leaves, params_kind=2)                   # MerkleCommitment's parameters
    assert pr == o.open_bytes(idx) and (root == o.root()).all()              # so the oracle decides on these very bytes
    ix = _w(idx); root = _w(root); v = _w(leaves[idx]); bad = mc.flip_bit(v, 6, 33)
    rows = [(x, pr, o.open_verify(idx, x)[0] == 1) for x in (v, bad)]; o.free()
    def call(h, row, proof, acc):
        vv = v if row is None else row
        return ctx.lib.stark_commitment_verify(h, ds, root.ctypes.data_as(_vp), ix.ctypes.data_as(_vp), len(ix), vv.ctypes.data_as(_vp), _u8(proof), len(proof), acc)
    return call, rows


def _sumcheck_subject(mf):
    def make(ctx, oracle):
        rows = []
        for k in (1, 5):
            w = oracle.rand_fr_columns(600 + k + mf, 1 << k, 1)[0]; label = 31 + k
            p = ctx.prove_mf(k, label, 2, w) if mf else ctx.prove_plain(k, label, w)
            for q in (p, _flip(p, 11)):                                      # byte 11: inside the first root
                rows.append(((k, label), q, oracle.sumcheck_verify(mf, k, label, q, q=2) == 1))
        def call(h, row, proof, acc):
            k, label = row if row else (1, 32)
            if mf:
                return ctx.lib.stark_sumcheck_verify_mf(h, k, label, 2, _u8(proof), len(proof), acc)
            return ctx.lib.stark_sumcheck_verify_plain(h, k, label, _u8(proof), len(proof), acc)
        return call, rows
    return make


_SINGLE = {"deep_fri_verify": _deep_fri_subject, "merkle_verify_many_ds": _merkle_subject(False), "merkle_verify_pairs_ds": _merkle_subject(True),
           "commitment_verify": _commitment_subject, "sumcheck_verify_plain": _sumcheck_subject(0), "sumcheck_verify_mf": _sumcheck_subject(1)}


@pytest.mark.parametrize("entry", sorted(_SINGLE))
def test_single_entry_point_decides_as_the_oracle_and_zeroes_its_flag(gpu_ctx, oracle, entry):
    """Each single verifier is its batch driver with one item.  With the accepted flag preset to 7: bytes that do not decode return 0 and flag 0;
    a null `accepted` or a null context returns -1; an honest proof or opening sets 1 and one with a flipped bit 0, each the oracle's decision."""
    call, rows = _SINGLE[entry](gpu_ctx, oracle)
    acc = C.c_int32(7)
    assert call(gpu_ctx.h, None, b"\x01\x02\x03", C.byref(acc)) == 0 and acc.value == 0
    assert call(gpu_ctx.h, None, b"\x01\x02\x03", None) == -1
    assert call(None, None, b"\x01\x02\x03", C.byref(acc)) == -1
    wants = []
    for row, proof, want in rows:
        acc = C.c_int32(7)
        assert call(gpu_ctx.h, row, proof, C.byref(acc)) == 0
        assert acc.value == int(want), (entry, len(proof), acc.value, want)
        wants.append(want)
    assert wants == [True, False] * (len(rows) // 2)                          # the honest one, then its flipped copy
