"""Parity tests proper: the HIP path through the C-ABI against the oracle on identical seeded inputs
(bit-exact: everything here is exact integer arithmetic), plus size-independent properties at the
BASELINE sizes.  Needs an MI355X: `pytest -m gpu`."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from stark_mlwe_amd.api import BLS12_381_FR, PALLAS_FR, DeepFriParams, StarkError


def F(oracle, x):
    return oracle.from_u64(x)


# ---- Poseidon -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [9, 17, 33])
def test_permute_batch(gpu_ctx, oracle, t):
    n = 130 if t <= 17 else 70                      # not a multiple of the 64-lane workgroup
    states = np.concatenate([oracle.synth_column(3, t, 0, (n - 1) * t), np.zeros((t, 4), np.uint64)]).reshape(n, t, 4)
    got = gpu_ctx.permute(states, gpu_ctx.poseidon_params_for_width(t))
    assert (got == oracle.permute(0, t, states)).all()


def test_permute_t17_bench_params_zero_state(gpu_ctx, oracle):
    # poseidon/benches/poseidon.rs:6-15: generate_params_t17_x5(b"POSEIDON-T17-X5"), state [0;17]
    p = gpu_ctx.generate_params_t17_x5(b"POSEIDON-T17-X5")
    z = np.zeros((1, 17, 4), np.uint64)
    assert (gpu_ctx.permute(z, p) == oracle.permute(3, 17, z)).all()
    mds, rcf, rcp = p.export()
    _, _, m2, f2, p2 = oracle.poseidon_params(3, 17)
    assert (mds == m2).all() and (rcf == f2).all() and (rcp == p2).all()
    p.free()


def test_params_upload_roundtrip(gpu_ctx, oracle):
    rf, rp, mds, rcf, rcp = oracle.poseidon_params(0, 9)
    p = gpu_ctx.params_upload(9, rf, rp, mds, rcf, rcp)
    st = oracle.synth_column(1, 1, 0, 18).reshape(2, 9, 4)
    assert (gpu_ctx.permute(st, p) == oracle.permute(0, 9, st)).all()
    p.free()
    with pytest.raises(StarkError):
        gpu_ctx.poseidon_params_for_width(10)          # unsupported width (poseidon/src/lib.rs:127 panics)


def test_hash_with_ds_dynamic_reference_shapes(gpu_ctx, oracle):
    # merkle/src/lib.rs:966-1050 (t=17: 16 / 5 / 5+zero children; t=9: 8 / 3 / 3+zero)
    p17, p9 = gpu_ctx.poseidon_params_for_width(17), gpu_ctx.poseidon_params_for_width(9)
    ds = np.array([F(oracle, x) for x in (16, 0, 3, 42)])
    digs = []
    for ch in (list(range(1, 17)), list(range(1, 6)), list(range(1, 6)) + [0]):
        c = np.array([F(oracle, x) for x in ch])
        got = gpu_ctx.hash_with_ds_dynamic(ds, c, p17)
        assert (got == oracle.hash_with_ds_dynamic(0, 17, ds, c, len(ch))).all()
        digs.append(got.tobytes())
    assert len(set(digs)) == 3
    ds9 = np.array([F(oracle, x) for x in (8, 2, 5, 7)])
    for ch in (list(range(11, 19)), [21, 22, 23], [21, 22, 23, 0]):
        c = np.array([F(oracle, x) for x in ch])
        assert (gpu_ctx.hash_with_ds_dynamic(ds9, c, p9) == oracle.hash_with_ds_dynamic(0, 9, ds9, c, len(ch))).all()
    # legacy sponge (poseidon/src/lib.rs:85-100) with the commitment seed
    ps = gpu_ctx.generate_params_t17_x5(b"POSEIDON-T17-X5-SEED")
    for cnt in (0, 2, 16, 37):
        c = oracle.synth_column(9, 9, 0, cnt) if cnt else np.zeros((0, 4), np.uint64)
        assert (gpu_ctx.hash_with_ds(c, F(oracle, 77), ps) == oracle.hash_with_ds(2, c, F(oracle, 77))).all()
    ps.free()


def test_leaf_pair_hash_layer(gpu_ctx, oracle):
    n, m = 1 << 12, 16
    f, fn = oracle.synth_column(5, 0, 0, n), oracle.synth_column(5, 1, 0, n // m)
    assert (gpu_ctx.leaf_pair_hash(f, fn, m) == oracle.leaf_pair_hash(f, fn, m)).all()
    assert (gpu_ctx.leaf_pair_hash(f[:100], None, 1) == oracle.leaf_pair_hash(f[:100], None, 1)).all()      # last layer: s = 0
    assert (gpu_ctx.hash_leaf_pair(F(oracle, 1), F(oracle, 2)) == oracle.leaf_pair_hash(F(oracle, 1).reshape(1, 4), F(oracle, 2).reshape(1, 4), 1)[0]).all()
    assert gpu_ctx.leaf_pair_hash(np.zeros((0, 4), np.uint64), None, 1).shape == (0, 4)                     # empty input


def test_tr_hash_fields_tagged(gpu_ctx, oracle):
    for n in (0, 1, 5, 12, 13, 29, 200):
        xs = oracle.synth_column(6, 0, 0, n) if n else np.zeros((0, 4), np.uint64)
        assert (gpu_ctx.tr_hash_fields_tagged(b"ALI/A", xs) == oracle.tr_hash_fields_tagged(b"ALI/A", xs)).all()
    batch = oracle.synth_column(6, 1, 0, 300)
    got = gpu_ctx.tr_hash_fields_tagged(b"FRI/index", batch, n=100)
    for i in (0, 1, 63, 64, 99):
        assert (got[i] == oracle.tr_hash_fields_tagged(b"FRI/index", batch[3 * i:3 * i + 3])).all()


def test_throughput_kernels_on_extreme_field_values(gpu_ctx, oracle):
    """The wave-pair kernels' full rounds multiply on the int8 matrix cores over SIGNED radix-256 digits (poseidon_pair.hpp): inputs whose
    LOGICAL values are extreme — 0, 1, r - 1, r - 2, all-0x7f / all-0x80 / all-0xff byte patterns (reduced below r), single high
    bits — through the leaf hash (k_leaf_pair2) and through an arity-16 Merkle tree of 2^18 leaves, whose first level (16 384 nodes, above
    the one-wave threshold) runs the wave-pair node kernels, against the oracle.  These byte patterns do not reach the recoding: from_int
    multiplies by R and the recoding reads the stored bytes of the S-box OUTPUTS.  test_gpu_corner_values.py crafts inputs whose round-0 S-box
    outputs are the chosen stored bytes."""
    import pyref
    p = pyref.P_PALLAS
    pats = [0, 1, 2, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2]
    pats += [int.from_bytes(bytes([b]) * 32, "little") % p for b in (0x7f, 0x80, 0x81, 0xff, 0x01, 0xfe)]
    pats += [(1 << k) % p for k in (7, 8, 15, 31, 63, 127, 128, 253)] + [((1 << k) - 1) % p for k in (8, 64, 128, 254)]
    vals = np.stack([oracle.from_int(v) for v in pats])
    n = 1 << 13
    rng = np.random.default_rng(7)
    f = vals[rng.integers(0, len(vals), n)]; fn = vals[rng.integers(0, len(vals), n // 16)]
    f[:len(vals)] = vals
    assert (gpu_ctx.leaf_pair_hash(f, fn, 16) == oracle.leaf_pair_hash(f, fn, 16)).all()
    assert (gpu_ctx.leaf_pair_hash(f, None, 1) == oracle.leaf_pair_hash(f, None, 1)).all()
    big = np.concatenate([f] * 32)                      # 2^18 leaves
    t = gpu_ctx.merkle_new(big, gpu_ctx.merkle_cfg(16, 3)); o = oracle.merkle_build(16, 3, big)
    for lvl in range(o.num_levels()):
        assert (t.level(lvl) == o.level(lvl)).all(), lvl
    t.free(); o.free()


def test_wave_pair_level_with_other_t17_constants(gpu_ctx, oracle):
    """The int8 fragments of the dense matrices are derived per parameter set: a Merkle level large enough for the wave-pair kernel
    (2^14 + 3 nodes, ragged last node) hashed with the `POSEIDON-T17-X5` parameters of the reference's bench (poseidon/benches/poseidon.rs:6-15)
    instead of the Merkle defaults, against the oracle's hash_with_ds_dynamic with the same constants on sampled nodes."""
    p = gpu_ctx.generate_params_t17_x5(b"POSEIDON-T17-X5")
    nodes = (1 << 14) + 3
    ch = oracle.synth_column(77, 2, 0, (nodes - 1) * 16 + 5)
    got = gpu_ctx.hash_ds_level(p, 16, 4, 100, 42, ch)
    assert got.shape[0] == nodes
    for k in (0, 1, 63, 64, 8191, 8192, nodes - 2, nodes - 1):
        kids = ch[16 * k: 16 * k + 16]
        ds = np.array([F(oracle, 16), F(oracle, 4), F(oracle, 100 + k), F(oracle, 42)])
        assert (got[k] == oracle.hash_with_ds_dynamic(3, 17, ds, kids, kids.shape[0])).all(), k
    p.free()


# ---- Merkle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arity,n,label", [(16, 4096, 0), (16, 55, 9), (16, 64, 42), (8, 512, 2), (8, 19, 3), (2, 8, 1), (4, 64, 7), (16, 1, 5), (32, 1024, 4)])
def test_merkle_tree_levels(gpu_ctx, oracle, arity, n, label):
    leaves = oracle.synth_column(4, 3, 0, n)
    t = gpu_ctx.merkle_new(leaves, gpu_ctx.merkle_cfg(arity, label))
    o = oracle.merkle_build(arity, label, leaves)
    assert t.num_levels == o.num_levels()
    for lvl in range(t.num_levels):
        assert (t.level(lvl) == o.level(lvl)).all(), lvl
    assert (t.root() == o.root()).all()
    t.free(); o.free()


@pytest.mark.parametrize("arity,n", [(2, 8), (2, 2), (16, 64), (8, 32), (2, 1)])
def test_merkle_pairs(gpu_ctx, oracle, arity, n):
    f, cp = oracle.synth_column(4, 0, 0, n), oracle.synth_column(4, 1, 0, n)
    t = gpu_ctx.merkle_new_pairs(f, cp, gpu_ctx.merkle_cfg(arity, 777))
    o = oracle.merkle_build(arity, 777, f, cp)
    for lvl in range(o.num_levels()):
        assert (t.level(lvl) == o.level(lvl)).all()
    t.free(); o.free()


def test_merkle_errors_and_open(gpu_ctx, oracle):
    with pytest.raises(StarkError):
        gpu_ctx.merkle_new(np.zeros((0, 4), np.uint64), gpu_ctx.merkle_cfg(16))                     # "no leaves"
    from stark_mlwe_amd.api import MerkleChannelCfg
    with pytest.raises(StarkError):
        gpu_ctx.merkle_new(oracle.synth_column(1, 1, 0, 16), MerkleChannelCfg(16, gpu_ctx.poseidon_params_for_width(9)))   # arity/width mismatch
    # open_union_of_paths: reference test indices (merkle/src/lib.rs:948); decode the canonical proof and
    # check every sibling against the tree levels, and the sibling count against the oracle's own opening
    leaves = oracle.rand_fr_columns(999, 64)[0]
    t = gpu_ctx.merkle_new(leaves, gpu_ctx.merkle_cfg(16, 42))
    o = oracle.merkle_build(16, 42, leaves)
    idx = [63, 0, 15, 16, 31, 47, 15]
    b = t.open_many(idx)
    u = lambda off: struct.unpack_from("<Q", b, off)[0]
    off = 0; k = u(off); off += 8
    indices = [u(off + 8 * i) for i in range(k)]; off += 8 * k
    assert indices == sorted(set(idx))
    nlev = u(off); off += 8
    sib_total = 0; sibs = []
    for _ in range(nlev):
        c = u(off); off += 8; sibs.append([b[off + 32 * i: off + 32 * i + 32] for i in range(c)]); off += 32 * c; sib_total += c
    ok, nsib = o.open_verify(idx, leaves[idx])
    assert ok == 1 and nsib == sib_total
    cur = indices
    for lvl in range(nlev):
        level = t.level(lvl); want = []
        for p in sorted(set(i // 16 for i in cur)):
            want += [oracle.to_bytes_le(level[c]) for c in range(16 * p, min(16 * p + 16, len(level))) if c not in cur]
        assert sibs[lvl] == want
        cur = sorted(set(i // 16 for i in cur))
    ng = u(off); off += 8
    for _ in range(ng):
        c = u(off); off += 8 + c
    assert u(off) == 16 and off + 8 == len(b)
    t.free(); o.free()


# ---- FRI -------------------------------------------------------------------------------------------------------
# every arity at a lane count that is a multiple of the 256-thread block (ids as before), then output counts that leave the last block partial
FOLD_SHAPES = ([pytest.param(m, m * 37 if m in (3, 6) else max(m * 5, 1 << 11), id=str(m)) for m in (2, 4, 8, 16, 32, 64, 128, 3, 6)] +
               [(m, m * c) for m in (2, 16, 128) for c in (37, 300)] + [(3, 3 * 257), (6, 6 * 257)])


@pytest.mark.parametrize("m,n", FOLD_SHAPES)
def test_fri_fold_layer(gpu_ctx, oracle, m, n):
    f = oracle.synth_column(2, 0, 0, n); z = oracle.fri_sample_z_ell(0xDEEFBAAD, 0, 1 << 11)
    got = gpu_ctx.fri_fold_layer(f, z, m)
    assert (got == oracle.fri_fold_layer(f, z, m)).all()
    assert (gpu_ctx.compute_s_layer(f, z, m) == oracle.compute_s_layer(f, z, m)).all()


def test_fri_fold_reference_vector_and_errors(gpu_ctx, oracle):
    f = np.array([F(oracle, x) for x in range(1, 65)]); z = F(oracle, 3)
    assert (gpu_ctx.fri_fold_layer(f, z, 16) == oracle.fri_fold_layer(f, z, 16)).all()
    with pytest.raises(StarkError): gpu_ctx.fri_fold_layer(f, z, 1)           # assert!(m >= 2), fri.rs:86
    with pytest.raises(StarkError): gpu_ctx.fri_fold_layer(f, z, 5)           # fri.rs:87
    assert gpu_ctx.fri_fold_layer(np.zeros((0, 4), np.uint64), z, 4).shape == (0, 4)


def test_fri_sample_z(gpu_ctx, oracle):
    for level, size in ((0, 1 << 12), (1, 1 << 8), (2, 16), (0, 1 << 20)):
        assert (gpu_ctx.fri_sample_z_ell(0xDEEFBAAD, level, size) == oracle.fri_sample_z_ell(0xDEEFBAAD, level, size)).all()


@pytest.mark.parametrize("n0,sched", [(1 << 12, [16, 16, 8]), (1 << 11, [16, 16, 8]), (1 << 10, [32, 32]), (1 << 9, [8, 4, 2]), (1 << 7, [128])])
def test_fri_build_transcript(gpu_ctx, oracle, n0, sched):
    f0 = oracle.synth_column(3, 0, 0, n0)
    st = gpu_ctx.fri_build_transcript(f0, sched, 0xDEEFBAAD)
    ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, 1, 0xDEEFBAAD, f0=f0)
    assert st.num_layers == len(sched) + 1
    for l in range(st.num_layers):
        assert (st.f_layer(l) == ref.layer_f(l)).all()
        assert (st.root(l) == ref.root(l)).all(), l
        if l < len(sched):
            assert (st.z(l) == ref.z(l)).all()
    st.free(); ref.free()


# ---- DEEP-ALI / end-to-end -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 64, 1000, 1 << 12])
def test_ali_merge(gpu_ctx, oracle, n):
    cols = [oracle.synth_column(8, c, 0, n) for c in range(5)]
    lg = max(1, (n - 1).bit_length())
    omega, z, beta = oracle.root_of_unity(lg), F(oracle, 0xC0FFEE), F(oracle, 12345)
    f0, _, cs = gpu_ctx.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z)
    w0, wc = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z)
    assert (f0 == w0).all()
    if n == (1 << lg):
        assert (cs == wc).all()            # c* is a statement about the full domain
    f1, _, _ = gpu_ctx.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z, r_eval=cols[4], beta=beta, want_c_star=False)
    w1, _ = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z, r=cols[4], beta=beta, want_c_star=False)
    assert (f1 == w1).all()
    with pytest.raises(StarkError):
        gpu_ctx.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, F(oracle, 1))       # z in H


def test_build_f0(gpu_ctx, oracle):
    n0 = 1 << 9
    cols = oracle.rand_fr_columns(1337, n0, 4)
    f0, aux = gpu_ctx.build_f0(cols[0], cols[1], cols[2], cols[3], n0)
    w0, waux = oracle.build_f0(cols[0], cols[1], cols[2], cols[3], n0)
    assert (aux == waux).all()             # column digests, seed_f, z, beta
    assert (f0 == w0).all()


@pytest.mark.parametrize("n0,sched,r", [(1 << 11, [16, 16, 8], 32), (1 << 10, [16, 8], 8), (1 << 9, [8, 4, 2], 5), (1 << 10, [32, 32], 40)])
def test_deep_fri_prove_bytes(gpu_ctx, oracle, n0, sched, r):
    cols = oracle.rand_fr_columns(4242 + n0, n0, 4)
    got, est, _ = gpu_ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, 0xDEEFBAAD))
    ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, sched, r, 0xDEEFBAAD)
    assert got == ref.bytes()              # bit-exact proof bytes
    assert est == ref.size_estimate()
    assert oracle.deep_fri_verify(got, sched, r, 0xDEEFBAAD) == 1
    ref.free()


def test_published_fingerprint_k11_on_gpu(gpu_ctx, oracle):
    """The reference's own bench input for k = 11 (end_to_end.rs:248-253) through the GPU prover:
    deep_fri_proof_size_bytes must be the published 39592 (crates/channel/benchmarkdata.csv:2)."""
    seed = (1337 * 1103515245 + 12345) % 2**64
    cols = oracle.rand_fr_columns(seed, 1 << 11, 4)
    got, est, _ = gpu_ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], 1 << 11, DeepFriParams([16, 16, 8], 32, 0xDEEFBAAD))
    assert est == 39592
    assert oracle.deep_fri_verify(got, [16, 16, 8], 32, 0xDEEFBAAD) == 1


# ---- NTT -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [PALLAS_FR, BLS12_381_FR])
@pytest.mark.parametrize("lg", [0, 1, 2, 3, 5, 8, 10, 11, 12, 13, 16])
def test_ntt_vs_oracle(gpu_ctx, oracle, field, lg):
    x = oracle.synth_column(77, 7, 0, 1 << lg)
    y = gpu_ctx.fft(x, field=field)
    assert (y == oracle.ntt(field, x)).all()
    assert (gpu_ctx.ifft(y, field=field) == x).all()
    assert (gpu_ctx.ifft(x, field=field) == oracle.ntt(field, x, inverse=True)).all()


@pytest.mark.parametrize("field,gen", [(PALLAS_FR, 5), (BLS12_381_FR, 7)])
def test_ntt_coset_lde_and_reference_roundtrip(gpu_ctx, oracle, field, gen):
    g = oracle.from_u64(gen, field)
    for lg in (3, 10, 12):
        x = oracle.synth_column(78, 7, 0, 1 << lg)
        y = gpu_ctx.fft(x, field=field, coset=g)
        assert (y == oracle.ntt(field, x, coset=g)).all()
        assert (gpu_ctx.ifft(y, field=field, coset=g) == x).all()
    ev = oracle.synth_column(79, 0, 0, 1 << 9)
    assert (gpu_ctx.lde(ev, 3, field=field, coset=g) == oracle.lde(field, ev, 3, g)).all()
    assert (gpu_ctx.lde(ev, 3, field=field)[::8] == ev).all()
    ones = np.tile(oracle.from_u64(1, field), (8, 1))                      # fft/src/lib.rs:39-54
    assert (gpu_ctx.ifft(gpu_ctx.fft(ones, field=field), field=field) == ones).all()
    with pytest.raises(StarkError):
        gpu_ctx.fft(ones[:6], field=field)


@pytest.mark.parametrize("lg", [20, 21])
def test_ntt_large_vs_oracle_and_properties(gpu_ctx, oracle, lg):
    """BASELINE size 2^20 (and a 3-pass size) against the oracle's radix-2 NTT, plus linearity."""
    x = oracle.synth_column(80, 7, 0, 1 << lg)
    y = gpu_ctx.fft(x, field=PALLAS_FR)
    assert (y == oracle.ntt(0, x)).all()
    assert (gpu_ctx.ifft(y, field=PALLAS_FR) == x).all()
    # the DC term is the sum of the inputs; a shifted delta transforms to the powers of w
    d = np.zeros((1 << lg, 4), np.uint64); d[1] = oracle.from_u64(1)
    yd = gpu_ctx.fft(d, field=PALLAS_FR)
    w = oracle.root_of_unity(lg)
    assert (yd[0] == oracle.from_u64(1)).all() and (yd[1] == w).all() and (yd[2] == oracle.mul(w, w)).all()


@pytest.mark.parametrize("lg", [17, 20, 21])
def test_ntt_large_bls12_381(gpu_ctx, oracle, lg):
    """The second field (the `fft` crate's BLS12-381 Fr) at two- and three-pass sizes, incl. the 2^10-point sub-NTTs of 2^20 (ten lazy stages: the
    value head-room of nine limbs is 70 r for this field, against 128 r for Pallas): forward, inverse and coset transforms against the oracle
    (the synthetic values are below 2^254 < r_BLS: valid residues of this field too)."""
    x = oracle.synth_column(81, 7, 0, 1 << lg)
    y = gpu_ctx.fft(x, field=BLS12_381_FR)
    assert (y == oracle.ntt(1, x)).all()
    assert (gpu_ctx.ifft(y, field=BLS12_381_FR) == oracle.ntt(1, y, inverse=True)).all()
    g = oracle.from_u64(7, 1)
    assert (gpu_ctx.fft(x, field=BLS12_381_FR, coset=g) == oracle.ntt(1, x, coset=g)).all()


def test_synthetic_generator(gpu_ctx, oracle):
    import ctypes as C
    import torch
    n = 1000
    buf = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    gpu_ctx._chk(gpu_ctx.lib.stark_synth_column_dev(gpu_ctx.h, 0x5EED0014, 2, 12345, n, C.c_void_p(buf.data_ptr())))
    gpu_ctx.sync()
    got = buf.cpu().numpy().view(np.uint64)
    assert (got == oracle.synth_column(0x5EED0014, 2, 12345, n)).all()


# ---- multi-GPU building blocks on one GPU (world size 1: the exchange is the identity) -------------------------
@pytest.mark.parametrize("log_n,log_rows,inverse", [(12, 6, False), (16, 8, False), (20, 10, False), (14, 7, True), (21, 10, False)])
def test_six_step_building_blocks(gpu_ctx, oracle, log_n, log_rows, inverse):
    import torch
    from stark_mlwe_amd import dist as sd
    n = 1 << log_n
    x = oracle.synth_column(91, 7, 0, n)
    plan = sd.DistNtt(sd.HipProvider(gpu_ctx), log_n, log_rows, inverse=inverse)
    slab = torch.from_numpy(x[plan.local_input_indices().reshape(-1).numpy()].view(np.int64).copy()).cuda()
    scale = oracle.inv(oracle.from_u64(n)) if inverse else None
    rows = plan.forward(slab, scale)
    gpu_ctx.sync()
    want = oracle.ntt(0, x, inverse=inverse)
    got = rows.cpu().numpy().view(np.uint64)
    assert (got == want[plan.local_output_indices().reshape(-1).numpy()]).all()
    nat = plan.to_natural_blocks(rows).cpu().numpy().view(np.uint64)
    assert (nat == want).all()


def test_sharded_merkle_single_rank(gpu_ctx, oracle):
    import torch
    from stark_mlwe_amd import dist as sd
    leaves = oracle.synth_column(5, 1, 0, 4096)
    prov = sd.HipProvider(gpu_ctx)
    root = sd.merkle_sharded_root(prov, gpu_ctx.poseidon_params_for_width(17), 16, 9, torch.from_numpy(leaves.view(np.int64).copy()).cuda(), 4096)
    assert (root.cpu().numpy().view(np.uint64) == oracle.merkle_build(16, 9, leaves).root()).all()
    # a shard of a larger tree: levels built from leaves [2048, 4096) with global positions equal the right half of the full tree
    h = prov.merkle_build(gpu_ctx.poseidon_params_for_width(17), 16, 9, torch.from_numpy(leaves[2048:].view(np.int64).copy()).cuda(), 2048, 2048, 0, 8)
    top, nlev = prov.merkle_last_level(h)
    full = oracle.merkle_build(16, 9, leaves)
    assert nlev == 3 and (top.cpu().numpy().view(np.uint64) == full.level(2)[8:]).all()
    prov.merkle_free(h)


# ---- BASELINE sizes: the oracle where it finishes in seconds, size-independent properties beyond ---------------
def test_leaf_hash_2pow20_sampled_against_oracle(gpu_ctx, oracle):
    """2^20 leaves through the wave-pair kernel; 2048 positions (incl. both ends) checked against the oracle."""
    n, m = 1 << 20, 16
    f, fn = oracle.synth_column(20, 0, 0, n), oracle.synth_column(20, 1, 0, n // m)
    h = gpu_ctx.leaf_pair_hash(f, fn, m)
    rng = np.random.default_rng(7)
    idx = np.unique(np.concatenate([[0, 1, 63, 64, n - 65, n - 64, n - 1], rng.integers(0, n, 2048)]))
    want = oracle.leaf_pair_hash(f[idx], fn[idx // m], 1)
    assert (h[idx] == want).all()


def test_merkle_2pow18_root_against_oracle(gpu_ctx, oracle):
    leaves = oracle.synth_column(21, 3, 0, 1 << 18)
    t = gpu_ctx.merkle_new(leaves, gpu_ctx.merkle_cfg(16, 5))
    o = oracle.merkle_build(16, 5, leaves)
    assert t.num_levels == 6 and (t.root() == o.root()).all()
    assert (t.level(2) == o.level(2)).all()
    t.free(); o.free()


def test_fold_and_ntt_properties_at_full_size(gpu_ctx, oracle):
    """n = 2^22: fold is linear in f; NTT round trip and Parseval-free checks (delta, constant) on the device."""
    n = 1 << 22
    f, g = oracle.synth_column(22, 0, 0, n), oracle.synth_column(22, 1, 0, n)
    z = oracle.fri_sample_z_ell(0xDEEFBAAD, 0, n)
    ff, fg = gpu_ctx.fri_fold_layer(f, z, 16), gpu_ctx.fri_fold_layer(g, z, 16)
    import ctypes as C
    # (f + g) computed limb-wise by the oracle on a sample is enough: fold(f+g)[b] == fold(f)[b] + fold(g)[b]
    bs = [0, 1, 12345, (n // 16) - 1]
    for b in bs:
        seg = np.array([oracle.add(f[16 * b + t], g[16 * b + t]) for t in range(16)])
        assert (oracle.fri_fold_layer(seg, z, 16)[0] == oracle.add(ff[b], fg[b])).all()
        assert (oracle.fri_fold_layer(f[16 * b:16 * b + 16], z, 16)[0] == ff[b]).all()
    y = gpu_ctx.fft(f, field=PALLAS_FR)
    assert (gpu_ctx.ifft(y, field=PALLAS_FR) == f).all()
    s = oracle.from_u64(0)
    # DC term = sum of inputs (checked on a strided subsample via linearity: NTT of a constant vector is n*c at 0)
    c = np.tile(oracle.from_u64(3), (n, 1))
    yc = gpu_ctx.fft(c, field=PALLAS_FR)
    assert (yc[0] == oracle.from_u64(3 * n)).all() and not yc[1:].any()


# ---- remaining shapes of the reference's presets and edge cases ------------------------------------------------
@pytest.mark.parametrize("arity,n", [(64, 4096), (128, 1 << 14), (64, 70), (128, 200)])
def test_merkle_wide_arities(gpu_ctx, oracle, arity, n):
    """arity 64 / 128 (t = 65 / 129, bench presets uni64x2x8, uni128...): rows longer than one wide chunk."""
    leaves = oracle.synth_column(31, 3, 0, n)
    t = gpu_ctx.merkle_new(leaves, gpu_ctx.merkle_cfg(arity, 2))
    o = oracle.merkle_build(arity, 2, leaves)
    assert t.num_levels == o.num_levels()
    for lvl in range(t.num_levels):
        assert (t.level(lvl) == o.level(lvl)).all()
    t.free(); o.free()


@pytest.mark.parametrize("n0,sched,r", [(16, [16], 3), (64, [8, 8], 4), (2, [2], 1), (1 << 12, [64, 64], 6)])
def test_prove_degenerate_and_preset_shapes(gpu_ctx, oracle, n0, sched, r):
    """last layer of a single element (arity 1 pair tree), tiny domains, and a 64-ary preset."""
    f0 = oracle.synth_column(41, 0, 0, n0)
    got, est, _ = gpu_ctx.deep_fri_prove(None, None, None, None, n0, DeepFriParams(sched, r, 0xDEEFBAAD), f0=f0)
    ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, r, 0xDEEFBAAD, f0=f0)
    assert got == ref.bytes() and est == ref.size_estimate()
    assert oracle.deep_fri_verify(got, sched, r, 0xDEEFBAAD) == 1
    ref.free()
    with pytest.raises(StarkError):
        gpu_ctx.deep_fri_prove(None, None, None, None, n0, DeepFriParams([3], r, 1), f0=f0)       # schedule not dividing the domain
    with pytest.raises(StarkError):
        gpu_ctx.deep_fri_prove(None, None, None, None, 24, DeepFriParams([2], r, 1), f0=oracle.synth_column(1, 0, 0, 24))   # not a radix-2 domain


def test_bench_step_shape_against_oracle(gpu_ctx, oracle):
    """The bench workload at a size the oracle finishes in seconds: LDE of 4 columns (blow-up 8, shift 5),
    DEEP-ALI merge with a fixed z, fri_build_transcript [16,16,8] — every root identical."""
    lg, lb = 8, 3
    n, N = 1 << lg, 1 << (lg + lb)
    cols = [oracle.synth_column(0x5EED0000 + lg, c, 0, n) for c in range(4)]
    g, z, omega = oracle.from_u64(5), oracle.from_u64(0xC0FFEE), oracle.root_of_unity(lg + lb)
    ext_g = [gpu_ctx.lde(c, lb, field=PALLAS_FR, coset=g) for c in cols]
    ext_o = [oracle.lde(0, c, lb, g) for c in cols]
    for a, b in zip(ext_g, ext_o):
        assert (a == b).all()
    f0_g, _, _ = gpu_ctx.deep_ali_merge_evals(ext_g[0], ext_g[1], ext_g[2], ext_g[3], omega, z, want_c_star=False)
    f0_o, _ = oracle.ali_merge(ext_o[0], ext_o[1], ext_o[2], ext_o[3], omega, z, want_c_star=False)
    assert (f0_g == f0_o).all()
    st = gpu_ctx.fri_build_transcript(f0_g, [16, 16, 8], 0xDEEFBAAD)
    ref = oracle.deep_fri_prove(None, None, None, None, N, [16, 16, 8], 1, 0xDEEFBAAD, f0=f0_o)
    for l in range(4):
        assert (st.root(l) == ref.root(l)).all()
    st.free(); ref.free()


def test_commitment_adapter_and_legacy_prover(gpu_ctx, oracle):
    """commitment/src/lib.rs:80-114 MerkleCommitment::commit: arity 16, params "POSEIDON-T17-X5-SEED",
    tree_label = ds_tag (test :121-136: seed 42, n = 64, ds_tag 123)."""
    from stark_mlwe_amd.api import MerkleChannelCfg
    leaves = oracle.rand_fr_columns(42, 64)[0]
    p = gpu_ctx.generate_params_t17_x5(b"POSEIDON-T17-X5-SEED")
    t = gpu_ctx.merkle_new(leaves, MerkleChannelCfg(16, p, 123))
    o = oracle.merkle_build(16, 123, leaves, params_kind=2)
    assert (t.root() == o.root()).all() and (t.level(1) == o.level(1)).all()
    assert o.open_verify([0, 15, 16, 31, 47, 63], leaves[[0, 15, 16, 31, 47, 63]])[0] == 1
    t.free(); o.free(); p.free()


def test_ntt_2pow24_device_properties(gpu_ctx, oracle):
    """BASELINE size 2^24 (three-pass plan): round trip and closed-form spectra, no oracle needed."""
    n = 1 << 24
    x = oracle.synth_column(24, 7, 0, n)
    y = gpu_ctx.fft(x, field=PALLAS_FR)
    assert (gpu_ctx.ifft(y, field=PALLAS_FR) == x).all()
    d = np.zeros((n, 4), np.uint64); d[3] = oracle.from_u64(1)          # delta at j = 3  ->  X[k] = w^(3k)
    yd = gpu_ctx.fft(d, field=PALLAS_FR)
    w = oracle.root_of_unity(24); w3 = oracle.mul(oracle.mul(w, w), w)
    assert (yd[0] == oracle.from_u64(1)).all() and (yd[1] == w3).all() and (yd[n // 2] == oracle.pow(w3, n // 2)).all()
    assert (yd[n - 1] == oracle.pow(w3, n - 1)).all()


# ---- one trace sharded over ranks: the composable pieces on one GPU (world size 1) ---------------------------------
def test_dist_prover_world1_and_shard_pieces(gpu_ctx, oracle):
    """DistProver with a single rank walks the sharded code path (local subtree + top tree, plan / fetch /
    assemble) and must give the bytes of the monolithic prove; the shard merge with a non-zero offset and the
    challenge derivation are compared with the oracle's build_f0."""
    import torch
    from stark_mlwe_amd import dist as sd
    n0, sched, r = 1 << 11, [16, 16, 8], 32
    cols = oracle.rand_fr_columns(99, n0, 4)
    dev = [torch.from_numpy(c.view(np.int64).copy()).cuda() for c in cols]
    prov = sd.HipProvider(gpu_ctx)
    dp = sd.DistProver(prov, n0, sched, r, 0xDEEFBAAD)
    proof, est = dp.prove(*dev)
    ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, sched, r, 0xDEEFBAAD)
    assert proof == ref.bytes() and est == ref.size_estimate()
    ref.free()
    # pieces: digests -> challenges, and the merge of the block [j0, j0 + nl) alone
    f0, aux = oracle.build_f0(cols[0], cols[1], cols[2], cols[3], n0)
    ch = gpu_ctx.ali_challenges(aux[:4], n0)
    assert (ch == aux[4:7]).all()
    j0, nl = 3 * n0 // 4, n0 // 4
    part = prov.ali_merge_shard(*[d[j0:j0 + nl].contiguous() for d in dev], aux[5], j0, n0)
    gpu_ctx.sync()
    assert (part.cpu().numpy().view(np.uint64) == f0[j0:j0 + nl]).all()


def test_ali_cstar_from_shard_partials(gpu_ctx, oracle):
    """c* = (1/n) sum_j phi_j w^j/(z - w^j) assembled from two blocks' partial sums (deep_ali/src/lib.rs:44,94)."""
    import ctypes as C
    import torch
    n = 1 << 10
    cols = oracle.rand_fr_columns(7, n, 4)
    w = oracle.domain_omega(n); z = oracle.from_u64(0xC0FFEE)
    f0, cs = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], w, z)
    dev = [torch.from_numpy(c.view(np.int64).copy()).cuda() for c in cols]
    parts = np.zeros((2, 4), np.uint64); out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    zz = np.ascontiguousarray(z)
    for b in range(2):
        j0, nl = b * n // 2, n // 2
        ptrs = [C.c_void_p(d[j0:j0 + nl].data_ptr()) for d in dev]
        gpu_ctx._chk(gpu_ctx.lib.stark_ali_merge_shard_dev(gpu_ctx.h, *ptrs, None, None, None, zz.ctypes.data_as(C.c_void_p), nl, j0, n,
                                                          C.c_void_p(out[j0:j0 + nl].data_ptr()), parts[b].ctypes.data_as(C.c_void_p)))
    gpu_ctx.sync()
    assert (out.cpu().numpy().view(np.uint64) == f0).all()
    got = np.zeros(4, np.uint64)
    gpu_ctx._chk(gpu_ctx.lib.stark_ali_cstar_from_partials(gpu_ctx.h, parts.ctypes.data_as(C.c_void_p), 2, n, got.ctypes.data_as(C.c_void_p)))
    assert (got == cs).all()


def test_gpu_proof_tamper_rejected(gpu_ctx, oracle):
    """N3: a proof produced on the GPU is accepted by deep_fri_verify (fri.rs:643-762, oracle restatement) and
    any single-byte change in an opened value, a sibling digest, a root or the query count is rejected."""
    n0, sched, r = 1 << 10, [16, 8], 8
    cols = oracle.rand_fr_columns(2024, n0, 4)
    got, _, _ = gpu_ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, 0xDEEFBAAD))
    assert oracle.deep_fri_verify(got, sched, r, 0xDEEFBAAD) == 1
    assert oracle.deep_fri_verify(got, sched, r + 1, 0xDEEFBAAD) == 0
    rejected = 0
    for pos in (8 + 5, 8 + 32 + 7, len(got) // 3, len(got) // 2, len(got) - 200, len(got) - 45):
        bad = bytearray(got); bad[pos] ^= 1
        rejected += oracle.deep_fri_verify(bytes(bad), sched, r, 0xDEEFBAAD) != 1
    assert rejected >= 5      # roots, siblings, opened values: caught; the trailing (n0, omega) words are not read by the reference's verifier


@pytest.mark.parametrize("log_n0,r", [(20, 32), (22, 40), (23, 32)])
def test_full_size_proof_accepted_by_reference_verifier(gpu_ctx, oracle, log_n0, r):
    """BASELINE sizes (2^20 trace; 2^23 = its blow-up-8 extension): the commit + query phases on the GPU, then
    deep_fri_verify (fri.rs:643-762, oracle restatement) on the proof bytes — every opened leaf, every Merkle
    multiproof up to the L+1 roots and the final layer must check out; the sharded code path must agree byte for byte."""
    import torch
    from stark_mlwe_amd import dist as sd
    n0, sched = 1 << log_n0, [16, 16, 8]        # (22, 40) is BASELINE configs[2]: 2^22 trace, full FRI, 40 queries
    f0 = torch.empty((n0, 4), dtype=torch.int64, device="cuda")
    gpu_ctx._chk(gpu_ctx.lib.stark_synth_column_dev(gpu_ctx.h, 0x5EED0000 + log_n0, 5, 0, n0, C.c_void_p(f0.data_ptr())))
    sch = np.ascontiguousarray(sched, dtype=np.uint64); h = C.c_void_p()
    gpu_ctx._chk(gpu_ctx.lib.stark_deep_fri_prove_dev(gpu_ctx.h, None, None, None, None, C.c_void_p(f0.data_ptr()), n0, sch.ctypes.data_as(C.c_void_p), 3, r, 0xDEEFBAAD, C.byref(h)))
    proof, est = gpu_ctx._proof_out(h)
    assert oracle.deep_fri_verify(proof, sched, r, 0xDEEFBAAD) == 1
    assert oracle.proof_size_estimate_from_bytes(proof) == est
    dp = sd.DistProver(sd.HipProvider(gpu_ctx), n0, sched, r, 0xDEEFBAAD)
    proof2, est2 = dp.prove(None, None, None, None, f0_local=f0)
    assert proof2 == proof and est2 == est
    bad = bytearray(proof); bad[len(bad) // 2] ^= 0x10
    assert oracle.deep_fri_verify(bytes(bad), sched, r, 0xDEEFBAAD) == 0


def test_ntt_two_level_twiddle_path_matches_direct_tables(gpu_ctx, oracle):
    """Transforms above 2^24 points (BASELINE's 2^26 config) take the two-level power-table lookup instead of the direct
    twiddle / coset tables.  The same code path is forced at 2^21 on a second context (`stark_ctx_set_option
    "ntt_direct_max_log" = 0` — an explicit option, nothing is read from the environment) and must give the bytes of the
    direct-table path, for the plain and the coset transform, forward and inverse; other tile sizes / occupancies too."""
    from stark_mlwe_amd.api import Context, StarkError
    x = oracle.synth_column(21, 7, 0, 1 << 21); g = oracle.from_u64(5)
    y = gpu_ctx.fft(x, field=PALLAS_FR); z = gpu_ctx.fft(x, field=PALLAS_FR, coset=g)
    c = Context(0)
    try:
        c.set_option("ntt_direct_max_log", 0)
        assert (c.fft(x, field=PALLAS_FR) == y).all() and (c.fft(x, field=PALLAS_FR, coset=g) == z).all()
        assert (c.ifft(z, field=PALLAS_FR, coset=g) == x).all()
        for key, val in (("ntt_log_tile", 9), ("ntt_log_tile", 12), ("ntt_min_waves", 4), ("ntt_log_tile", -1)):
            c.set_option(key, val)
            assert (c.fft(x, field=PALLAS_FR, coset=g) == z).all(), (key, val)
        c.set_option("poseidon_lane_only", 1)
        f = oracle.synth_column(2, 1, 0, 200)
        assert (c.leaf_pair_hash(f, None, 1) == oracle.leaf_pair_hash(f, None, 1)).all()
        with pytest.raises(StarkError):
            c.set_option("no_such_option", 1)
        with pytest.raises(StarkError):
            c.set_option("ntt_log_tile", 5)
    finally:
        c.close()
    assert (gpu_ctx.ifft(z, field=PALLAS_FR, coset=g) == x).all()
