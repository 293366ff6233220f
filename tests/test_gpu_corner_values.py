"""Stored-limb corner values through the device kernels (C-ABI) against the oracle on identical stored inputs, bit for bit.

The inputs are corners of the four u64 limbs AS STORED (tests/corner_values.py), and for the Poseidon kernels inputs crafted so that the
S-box outputs of round 0 — the words the signed radix-256 recoding in front of the int8 matrix cores reads — are chosen byte patterns
(0x80 / 0x7f carry chains across every 32-bit word, all-0xff, the band [2^254, r) ...).  The device keeps its own copies of the recoding, the
fold and the carry pass, so only device runs on chosen digits can see a mistake in them.  tests/test_corner_values_host.py checks the
construction itself on the CPU.  Needs an MI355X: `pytest -m gpu`.

Still open: the non-canonical-lane bound of pair_lane_update (2.7 r after 16 blocks of partial rounds) would need control of the partial-round
S-box outputs 64 rounds deep; nothing here forces it."""
import numpy as np
import pytest

import corner_values as cv
import pyref

pytestmark = pytest.mark.gpu

from stark_mlwe_amd.api import BLS12_381_FR, PALLAS_FR, DeepFriParams, StarkError

P = pyref.P_PALLAS
R = pyref.R
PRIMES = {PALLAS_FR: pyref.P_PALLAS, BLS12_381_FR: pyref.P_BLS}


def with_options(ctx, opts, fn):
    """run fn with context options set to `opts` ({key: (value, value to restore)}), restoring them whatever happens"""
    try:
        for k, (v, _) in opts.items():
            ctx.set_option(k, v)
        return fn()
    finally:
        for k, (_, back) in opts.items():
            ctx.set_option(k, back)


def first_diff(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if bad.size == 0 else int(bad[0])


# ---- Poseidon: every kernel form on crafted levels ----------------------------------------------------------------------------------
# kernel forms of a Merkle level (capi_poseidon.hip poseidon_form): the default choice by size — five-wave up to 256 nodes, one-wave up to 4096,
# k_node16_pair above — and what the options force
FORMS = {"default": {}, "k_hash_ds2 (merkle_node16_pair = 0)": {"merkle_node16_pair": (0, 1)}, "lane (poseidon_lane_only = 1)": {"poseidon_lane_only": (1, 0)},
         "one-wave / wave-pair (sponge_one_wave = 1)": {"sponge_one_wave": (1, 0)}}


def check_level(ctx, oracle, dev_params, okind, params, nodes, level, pos0, label, last_children=None, forms=FORMS):
    t = params["t"]; arity = t - 1
    ch, slot_idx = cv.crafted_level(params, nodes, last_children=last_children)
    full = nodes if last_children is None else nodes - 1
    want = np.zeros((nodes, 4), np.uint64)
    want[:full] = oracle.hash_with_ds_dynamic(okind, t, cv.ds_words(oracle, arity, level, pos0, label, full), ch[:full * arity], arity, n=full).reshape(full, 4)
    if last_children is not None:
        want[full] = oracle.hash_with_ds_dynamic(okind, t, cv.ds_words(oracle, arity, level, pos0 + full, label, 1), ch[full * arity:], last_children)
    for name, opts in forms.items():
        got = with_options(ctx, opts, lambda: ctx.hash_ds_level(dev_params, arity, level, pos0, label, ch))
        assert got.shape == want.shape
        k = first_diff(got, want)
        assert k is None, "form %s, %d nodes, t = %d: node %d (lane %d) differs from the oracle; children (stored limbs) %s; round-0 S-box targets %s" % (
            name, nodes, t, k, k % 64, cv.hex_limbs(ch[arity * k:arity * k + arity]), cv.hex_limbs(cv.raw_array([cv.stored_corners(P)[i] for i in slot_idx[k]])))
    return slot_idx


@pytest.mark.parametrize("nodes,last", [(256, None), (257, None), (4096, None), (4097, None), (8193, None), (4100, 5)])
def test_crafted_merkle_levels_every_kernel_form(gpu_ctx, oracle, nodes, last):
    """hash_ds_level over crafted arity-16 nodes — every stored corner as the round-0 S-box output of every one of the twelve controllable
    state elements, in lanes of both 32-sponge column tiles — at the node counts on both sides of every form threshold, a ragged level, and
    under every option that changes the kernel: all forms equal the oracle's hash_with_ds_dynamic on EVERY node."""
    p17 = gpu_ctx.poseidon_params_for_width(17)
    slot_idx = check_level(gpu_ctx, oracle, p17, 0, pyref.params_for_width(17), nodes, 3, 1000, 42, last_children=last)
    if nodes > 4096:
        L = len(cv.stored_corners(P)); n_full = nodes if last is None else nodes - 1
        cover = np.zeros((L, 12, 2), bool)
        n = np.arange(n_full)
        for j in range(12):
            cover[slot_idx[:n_full, j], j, (n % 64) // 32] = True
        assert cover.all()                 # every corner in every slot in both halves of a 64-sponge block


def test_crafted_levels_other_parameter_sets_and_t9(gpu_ctx, oracle):
    """The fragment tables are derived per parameter set and t = 9 takes the L*U pair path: crafted levels (targets crafted with the set's own
    round constants) for `POSEIDON-T17-X5` and for arity 8."""
    pb = gpu_ctx.generate_params_t17_x5(b"POSEIDON-T17-X5")
    try:
        bench = pyref.derive_params(b"POSEIDON-T17-X5", 17, 8, 64)
        for nodes, last in ((257, None), (4097, None), (4099, 5)):
            check_level(gpu_ctx, oracle, pb, 3, bench, nodes, 4, 100, 42, last_children=last)
    finally:
        pb.free()
    p9 = gpu_ctx.poseidon_params_for_width(9)
    forms = {k: v for k, v in FORMS.items() if "node16" not in k}
    for nodes, last in ((300, None), (4097, None), (4098, 3)):
        check_level(gpu_ctx, oracle, p9, 0, pyref.params_for_width(9), nodes, 1, 7, 5, last_children=last, forms=forms)


@pytest.mark.parametrize("t", [9, 17, 33])
def test_permute_on_corner_and_crafted_states(gpu_ctx, oracle, t):
    corners = cv.stored_corners(P); L = len(corners)
    params = pyref.params_for_width(t)
    rows = [[corners[(i + j) % L] for j in range(t)] for i in range(L)] + [[v] * t for v in corners]
    rows += [cv.crafted_state(params, [corners[(i + 2 * j) % L] for j in range(t)]) for i in range(L)]
    st = np.stack([cv.raw_array(r) for r in rows])
    assert st.shape[0] % 64
    got = gpu_ctx.permute(st, gpu_ctx.poseidon_params_for_width(t))
    want = oracle.permute(0, t, st)
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, "t = %d, state %d: %s" % (t, bad[0], cv.hex_limbs(st[bad[0]]))


@pytest.mark.parametrize("n", [2048, 2049, 4096, 4097, 1 << 13])
def test_leaf_pair_hash_on_corners(gpu_ctx, oracle, n):
    corners = cv.raw_array(cv.stored_corners(P)); L = corners.shape[0]
    rng = np.random.default_rng(n)
    f = corners[rng.integers(0, L, n)]; fn = corners[rng.integers(0, L, (n + 15) // 16)]
    f[:L] = corners; f[n - L:] = corners[::-1]; fn[:L] = corners
    for m, nxt in ((16, fn), (1, None)):
        got, want = gpu_ctx.leaf_pair_hash(f, nxt, m), oracle.leaf_pair_hash(f, nxt, m)
        k = first_diff(got, want)
        assert k is None, "m = %d, %d leaves: leaf %d f = %s" % (m, n, k, cv.hex_limbs(f[k]))
    got = with_options(gpu_ctx, {"poseidon_lane_only": (1, 0)}, lambda: gpu_ctx.leaf_pair_hash(f, fn, 16))
    assert (got == oracle.leaf_pair_hash(f, fn, 16)).all()


@pytest.mark.parametrize("n", [512, 513, 4097])
def test_tr_hash_on_corners(gpu_ctx, oracle, n):
    x = cv.pattern_d(P, 3 * n)
    got = gpu_ctx.tr_hash_fields_tagged(b"FRI/index", x, n=n)
    for i in range(n):
        assert (got[i] == oracle.tr_hash_fields_tagged(b"FRI/index", x[3 * i:3 * i + 3])).all(), (n, i, cv.hex_limbs(x[3 * i:3 * i + 3]))


def test_merkle_tree_over_crafted_leaves(gpu_ctx, oracle):
    """arity-16 merkle_new over 2^17 leaves that are the children of 8192 crafted nodes: every level against the oracle's tree."""
    leaves, _ = cv.crafted_level(pyref.params_for_width(17), 1 << 13)
    assert leaves.shape[0] == 1 << 17
    t = gpu_ctx.merkle_new(leaves, gpu_ctx.merkle_cfg(16, 3)); o = oracle.merkle_build(16, 3, leaves)
    try:
        assert t.num_levels == o.num_levels()
        for lvl in range(o.num_levels()):
            assert (t.level(lvl) == o.level(lvl)).all(), lvl
    finally:
        t.free(); o.free()


# ---- NTT ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,gen", [(PALLAS_FR, 5), (BLS12_381_FR, 7)])
@pytest.mark.parametrize("lg", [3, 10, 12, 13, 16, 20, 21])
def test_ntt_on_stored_extremes(gpu_ctx, oracle, field, gen, lg):
    """fft / ifft / coset fft / lde on whole vectors of stored p - 1, stored 2^254 - 1, two alternating patterns and the corner list by index."""
    p = PRIMES[field]; n = 1 << lg
    g = oracle.from_u64(gen, field)
    for name, x in cv.patterns(p, n).items():
        assert (gpu_ctx.fft(x, field=field) == oracle.ntt(field, x)).all(), (field, lg, name, "fft")
        assert (gpu_ctx.ifft(x, field=field) == oracle.ntt(field, x, inverse=True)).all(), (field, lg, name, "ifft")
        assert (gpu_ctx.fft(x, field=field, coset=g) == oracle.ntt(field, x, coset=g)).all(), (field, lg, name, "coset fft")
        assert (gpu_ctx.ifft(x, field=field, coset=g) == oracle.ntt(field, x, inverse=True, coset=g)).all(), (field, lg, name, "coset ifft")
        if lg < 4:
            continue
        ev = x[:n >> 3]
        assert (gpu_ctx.lde(ev, 3, field=field, coset=g) == oracle.lde(field, ev, 3, g)).all(), (field, lg, name, "lde")


def test_ntt_two_level_twiddles_and_tiles_on_stored_extremes(oracle):
    """The two-level twiddle lookup (ntt_direct_max_log = 0) and the 2^9 / 2^12 tiles on a second context, at 2^21, on the corner list by index
    and on all-(p - 1), against the oracle."""
    from stark_mlwe_amd.api import Context
    g = oracle.from_u64(5)
    pats = cv.patterns(P, 1 << 21)
    c = Context(0)
    try:
        c.set_option("ntt_direct_max_log", 0)
        for name in ("corners by index", "all p-1"):
            x = pats[name]; y = oracle.ntt(0, x); z = oracle.ntt(0, x, coset=g)
            assert (c.fft(x, field=PALLAS_FR) == y).all() and (c.fft(x, field=PALLAS_FR, coset=g) == z).all(), name
            assert (c.ifft(z, field=PALLAS_FR, coset=g) == x).all(), name
            for tile in (9, 12, -1):
                c.set_option("ntt_log_tile", tile)
                assert (c.fft(x, field=PALLAS_FR, coset=g) == z).all(), (name, tile)
    finally:
        c.close()


@pytest.mark.parametrize("log_n,log_rows", [(16, 8), (20, 10)])
def test_six_step_building_blocks_on_stored_extremes(gpu_ctx, oracle, log_n, log_rows):
    import torch
    from stark_mlwe_amd import dist as sd
    n = 1 << log_n
    pats = cv.patterns(P, n)
    plan = sd.DistNtt(sd.HipProvider(gpu_ctx), log_n, log_rows, inverse=False)
    for name in ("corners by index", "all p-1", "alternating 29-bit limb phases"):
        x = pats[name]
        slab = torch.from_numpy(x[plan.local_input_indices().reshape(-1).numpy()].view(np.int64).copy()).cuda()
        rows = plan.forward(slab, None)
        gpu_ctx.sync()
        nat = plan.to_natural_blocks(rows).cpu().numpy().view(np.uint64)
        assert (nat == oracle.ntt(0, x)).all(), name


# ---- FRI fold / ALI merge ---------------------------------------------------------------------------------------------------------------
Z_STORED = [P - 1, (1 << 254) - 1, 1 << 254, R % P]


@pytest.mark.parametrize("m", [2, 4, 8, 16, 32, 64, 128, 3, 6])
def test_fri_fold_on_corners(gpu_ctx, oracle, m):
    n = m * 37 if m in (3, 6) else max(m * 5, 1 << 11)
    f = cv.pattern_d(P, n)
    for zs in Z_STORED:
        z = cv.raw(zs)
        assert (gpu_ctx.fri_fold_layer(f, z, m) == oracle.fri_fold_layer(f, z, m)).all(), (m, hex(zs))
        assert (gpu_ctx.compute_s_layer(f, z, m) == oracle.compute_s_layer(f, z, m)).all(), (m, hex(zs))


@pytest.mark.parametrize("n", [64, 1000, 1 << 12])
def test_ali_merge_on_corners(gpu_ctx, oracle, n):
    c = cv.pattern_d(P, n + 4 * 7)
    cols = [c[7 * k:7 * k + n] for k in range(5)]                      # the corner list by index, each column at its own offset
    lg = (n - 1).bit_length()
    omega, beta = oracle.root_of_unity(lg), cv.raw((1 << 254) + 1)
    for zs in Z_STORED:
        z = cv.raw(zs)
        if pow(zs * pow(R, -1, P) % P, 1 << lg, P) == 1:               # z in the domain (stored R mod p is the logical 1)
            with pytest.raises(StarkError):
                gpu_ctx.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z)
            continue
        f0, _, cs = gpu_ctx.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z)
        w0, wc = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z)
        assert (f0 == w0).all(), (n, hex(zs))
        if n == 1 << lg:
            assert (cs == wc).all(), (n, hex(zs))
        f1, _, _ = gpu_ctx.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z, r_eval=cols[4], beta=beta, want_c_star=False)
        w1, _ = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z, r=cols[4], beta=beta, want_c_star=False)
        assert (f1 == w1).all(), (n, hex(zs))
    assert any(pow(zs * pow(R, -1, P) % P, 1 << lg, P) == 1 for zs in Z_STORED)


def test_fri_transcript_and_prove_on_corners(gpu_ctx, oracle):
    n0, sched, r, seed_z = 1 << 11, [16, 16, 8], 32, 0xDEEFBAAD
    c = cv.pattern_d(P, n0 + 33)
    f0 = c[:n0]
    st = gpu_ctx.fri_build_transcript(f0, sched, seed_z)
    ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, 1, seed_z, f0=f0)
    try:
        for l in range(st.num_layers):
            assert (st.f_layer(l) == ref.layer_f(l)).all() and (st.root(l) == ref.root(l)).all(), l
            if l < len(sched):
                assert (st.z(l) == ref.z(l)).all()
    finally:
        st.free(); ref.free()
    cols = [c[11 * k:11 * k + n0] for k in range(4)]
    got, est, _ = gpu_ctx.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, seed_z))
    ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, sched, r, seed_z)
    try:
        assert got == ref.bytes() and est == ref.size_estimate()
        assert oracle.deep_fri_verify(got, sched, r, seed_z) == 1
    finally:
        ref.free()


# ---- sum-check ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 12])
def test_sumcheck_on_corners(gpu_ctx, oracle, k):
    import torch
    pats = cv.patterns(P, 1 << k)
    ws = [pats["corners by index"], pats["all p-1"], pats["alternating 29-bit limb phases"]]
    labels = [2025, 7, 5050]; q = 2
    want = [[oracle.sumcheck_prove(mf, k, labels[b], ws[b], q=q) for b in range(3)] for mf in (0, 1)]
    for mf in (0, 1):
        for b in range(3):
            assert oracle.sumcheck_verify(mf, k, labels[b], want[mf][b], q=q) == 1
    for b in range(2):
        assert gpu_ctx.prove_plain(k, labels[b], ws[b]) == want[0][b], b
        assert gpu_ctx.prove_mf(k, labels[b], q, ws[b]) == want[1][b], b
    ts = [torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to("cuda") for w in ws]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in ts]
    for B in (1, 3):
        assert gpu_ctx.prove_plain_batch_dev(k, labels[:B], ptrs[:B]) == want[0][:B], B
        assert gpu_ctx.prove_mf_batch_dev(k, labels[:B], q, ptrs[:B]) == want[1][:B], B
    assert gpu_ctx.verify_plain(k, labels[0], want[0][0]) is True and gpu_ctx.verify_mf(k, labels[0], q, want[1][0]) is True
