"""What the library reads from its own temporaries, on the device.  The context's allocator recycles released blocks without clearing them, the NTT
scratch vector lives across calls, and fresh driver memory is normally zero: a kernel or driver that reads a scratch element nobody wrote usually
finds either the right answer of an identical earlier call or zeros.  The context option "pool_poison" fills every pooled block the library hands to
itself (the whole rounded block, recycled or fresh) and the scratch vector with a byte of the test's choice.

Every case below runs in a context of its own, under fill 0x5A (the byte of the project's SENTINEL; as limbs a non-zero stored element above the
Pallas modulus) and under fill 0x00, twice under each so that the second run recycles the blocks of the first.  Each of the four results must be
byte-equal to the ORACLE's result on the same inputs; no result is compared with another library call.  The shapes are the smallest the suite
already uses that still cross every kernel form and every chunked pass.  The shared drivers run under the same two fills on the CPU in
tests/test_pool_poison_host.py.  Needs an MI355X (`pytest -m gpu`)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import lde_shapes as ls
import merkle_batch_cases as mc
import mle_cases as mle

pytestmark = pytest.mark.gpu

from stark_mlwe_amd.api import BLS12_381_FR, PALLAS_FR, Context, DeepFriParams, StarkError

FILLS = (0x5A, 0x00)
SEED_Z = 0xDEEFBAAD
SEED = 0xB47C
vp = C.c_void_p


def pool_round(nbytes):
    """the block size of ctx_alloc (csrc/capi_core.hip pool_round): 256 B at least, powers of two up to 1 MiB, whole MiB above"""
    if nbytes < 256:
        return 256
    if nbytes <= 1 << 20:
        r = 256
        while r < nbytes:
            r <<= 1
        return r
    return (nbytes + (1 << 20) - 1) & ~((1 << 20) - 1)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


@contextlib.contextmanager
def own_context(**options):
    """a context of the test's own (the session's keeps its options), closed whatever happens"""
    c = Context(0)
    try:
        for k, v in options.items():
            c.set_option(k, v)
        yield c
    finally:
        c.close()


def equal(got, want):
    if isinstance(want, np.ndarray):
        return isinstance(got, np.ndarray) and got.shape == want.shape and bool((got == want).all())
    if isinstance(want, (list, tuple)):
        return isinstance(got, (list, tuple)) and len(got) == len(want) and all(equal(g, w) for g, w in zip(got, want))
    return got == want


def under_both_fills(c, cases):
    """cases: (name, run(c) -> result, the oracle's result).  Every case under 0x5A and under 0x00, twice each, in the one context."""
    for fill in FILLS:
        c.set_option("pool_poison", fill)
        for rep in (1, 2):
            for name, run, want in cases:
                assert equal(run(c), want), "%s: differs from the oracle under fill 0x%02X, run %d" % (name, fill, rep)


# ---- the option itself ------------------------------------------------------------------------------------------------------------------------
def test_option_range_and_unknown_key():
    with own_context() as c:
        for bad in (-2, 256, 1 << 20, -(1 << 40)):
            with pytest.raises(StarkError) as e:
                c.set_option("pool_poison", bad)
            assert "pool_poison" in str(e.value) and "0..255" in str(e.value), str(e.value)
        for ok in (0, 255, 0x5A, -1):
            c.set_option("pool_poison", ok)
        with pytest.raises(StarkError) as e:
            c.set_option("no_such_option", 1)
        assert str(e.value).find("unknown option 'no_such_option' (") >= 0 and "pool_poison" in str(e.value), str(e.value)


def test_fill_covers_the_rounded_block_and_no_level_writes_past_itself(oracle):
    """arity 16 over 257 leaves under 0x5A: every level is a block of its own, and the bytes between the end of the level and the end of its rounded
    block are still the fill after the build — the fill ran on the whole block and no level kernel wrote past its level inside its block"""
    arity, n, label = 16, 257, 0x5EED
    f = mc.leaves_of(oracle, SEED, 0, n); want = oracle.merkle_build(arity, label, f)
    with own_context() as c:
        c.set_option("pool_poison", 0x5A)
        for rep in (1, 2):
            t = c.merkle_new(f, c.merkle_cfg(arity, label))
            try:
                assert t.num_levels == want.num_levels() == 4
                for v in range(t.num_levels):
                    ln = c.lib.stark_merkle_level_len(t.h, v); p = c.lib.stark_merkle_level_dev(t.h, v)
                    assert ln == [257, 17, 2, 1][v] and p
                    pad = pool_round(32 * ln) - 32 * ln
                    assert pad > 0
                    tail = np.zeros(pad, np.uint8)
                    c._chk(c.lib.stark_memcpy_d2h(c.h, tail.ctypes.data_as(vp), vp(p + 32 * ln), pad))
                    assert (tail == 0x5A).all(), "run %d, level %d: %d of the %d bytes behind the level are not the fill" % (rep, v, int((tail != 0x5A).sum()), pad)
                    assert (t.level(v) == want.level(v)).all(), (rep, v)
            finally:
                t.free()
    want.free()


# ---- Merkle levels and leaf layers ------------------------------------------------------------------------------------------------------------
def tree_case(oracle, arity, n, pairs=False, label=0x5EED):
    """(run, want): every level and one opening (duplicates, the last leaf) of MerkleTree::new / new_pairs over n leaves"""
    f = mc.leaves_of(oracle, SEED, 0, n); cp = mc.leaves_of(oracle, SEED, 100, n) if pairs else None
    o = oracle.merkle_build(arity, label, f, cp); ix = mc.index_lists(n, 1)
    want = [o.level(v) for v in range(o.num_levels())] + [o.open_bytes(ix)]
    o.free()

    def run(c):
        cfg = c.merkle_cfg(arity, label)
        t = c.merkle_new_pairs(f, cp, cfg) if pairs else c.merkle_new(f, cfg)
        try:
            return t.levels + [t.open_many(ix)]
        finally:
            t.free()
    return run, want


def leaf_case(oracle, n, m):
    f = oracle.synth_column(0x1EAF, 0, 0, n); fn = oracle.synth_column(0x1EAF, 1, 0, (n + m - 1) // m)
    return (lambda c: c.leaf_pair_hash(f, fn, m)), oracle.leaf_pair_hash(f, fn, m)


@pytest.mark.parametrize("n", [256, 257, 4096, 4097, 8193])
def test_merkle_arity_16_levels(oracle, n):
    """level 1 holds 16, 17, 256, 257 and 513 hashes: both sides of the bounds of the five-wave (<= 256 hashes), the one-wave (<= 4096) and the
    wave-pair form for the leaf-rate levels above, with ragged last nodes"""
    with own_context() as c:
        under_both_fills(c, [("arity 16, n = %d" % n,) + tree_case(oracle, 16, n)])


@pytest.mark.parametrize("arity,n", [(8, 19), (32, 100)])
def test_merkle_other_widths(oracle, arity, n):
    with own_context() as c:
        under_both_fills(c, [("arity %d, n = %d" % (arity, n),) + tree_case(oracle, arity, n)])


@pytest.mark.parametrize("arity,n", [(2, 2), (16, 64)])
def test_merkle_pair_leaves(oracle, arity, n):
    with own_context() as c:
        under_both_fills(c, [("pairs, arity %d, n = %d" % (arity, n),) + tree_case(oracle, arity, n, pairs=True)])


@pytest.mark.parametrize("n,m", [(2049, 1), (4097, 16)])
def test_leaf_pair_hash(oracle, n, m):
    with own_context() as c:
        under_both_fills(c, [("leaf_pair_hash, n = %d, m = %d" % (n, m),) + leaf_case(oracle, n, m)])


@pytest.mark.parametrize("option", ["poseidon_lane_only", "sponge_one_wave"])
def test_other_kernel_forms_at_4097(oracle, option):
    with own_context(**{option: 1}) as c:
        under_both_fills(c, [("%s: arity 16, n = 4097" % option,) + tree_case(oracle, 16, 4097), ("%s: leaf_pair_hash, n = 4097" % option,) + leaf_case(oracle, 4097, 16)])


def deep_fri_verify_cases(oracle, n0, sched, r, seed):
    """one honest proof, one of another n0, one truncated and eight bit flips, all made and judged by the oracle: the batch call and the single calls"""
    def prove(n, s):
        cols = oracle.rand_fr_columns(s, n, 4)
        ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n, sched, r, SEED_Z)
        b = ref.bytes(); ref.free()
        return b
    proof = prove(n0, seed); batch = [proof, prove(2 * n0, seed + 1), proof[:-1]]
    for i, pos in enumerate((0, 8, 8 + 31, len(proof) // 3, len(proof) // 2, len(proof) - 41, len(proof) - 33, len(proof) - 1)):
        bad = bytearray(proof); bad[pos] ^= 1 << i; batch.append(bytes(bad))
    want = [oracle.deep_fri_verify(p, sched, r, SEED_Z) == 1 for p in batch]
    assert want[:3] == [True, True, False] and len(batch) == 11
    prm = DeepFriParams(sched, r, SEED_Z); what = "deep_fri_verify (%d, %s, %d)" % (n0, sched, r)
    return [(what + ", batch", lambda c: c.deep_fri_verify_batch(prm, batch), want), (what + ", single", lambda c: [c.deep_fri_verify(prm, p) for p in batch], want)]


def test_wide_widths(oracle):
    """t = 65 and t = 129 in ONE test: a context derives the kernel constants of a width on the host when it first meets it, which for t = 129 takes far
    longer than everything else here together — the trees (64, 70) and (128, 200) and deep_fri_verify at (2^12, [128], 8) share that context"""
    with own_context() as c:
        under_both_fills(c, [("arity 64, n = 70",) + tree_case(oracle, 64, 70), ("arity 128, n = 200",) + tree_case(oracle, 128, 200)] + deep_fri_verify_cases(oracle, 1 << 12, [128], 8, 2025))


# ---- NTT / LDE --------------------------------------------------------------------------------------------------------------------------------
def ntt_cases(oracle, field, lg):
    """forward, inverse, and both on the coset of the field's generator; lg 12 and 13 take two passes through the scratch vector"""
    x = oracle.synth_column(0xBA7C000 + lg, field, 0, 1 << lg)                  # stored values below 2^254: elements of both fields
    g = oracle.from_u64(5 if field == 0 else 7, field); what = "field %d, lg %d: " % (field, lg)
    return [(what + "forward", lambda c: c.fft(x, field=field), oracle.ntt(field, x)),
            (what + "inverse", lambda c: c.ifft(x, field=field), oracle.ntt(field, x, inverse=True)),
            (what + "forward on a coset", lambda c: c.fft(x, field=field, coset=g), oracle.ntt(field, x, coset=g)),
            (what + "inverse on a coset", lambda c: c.ifft(x, field=field, coset=g), oracle.ntt(field, x, inverse=True, coset=g))]


@pytest.mark.parametrize("field", [PALLAS_FR, BLS12_381_FR])
def test_ntt_default_tile(oracle, field):
    with own_context() as c:
        under_both_fills(c, [case for lg in (3, 12, 13) for case in ntt_cases(oracle, field, lg)])


def test_ntt_small_tile(oracle):
    """lg 10 in tiles of 2^8: the strided passes at the smallest tile"""
    with own_context(ntt_log_tile=8) as c:
        under_both_fills(c, ntt_cases(oracle, PALLAS_FR, 10) + ntt_cases(oracle, BLS12_381_FR, 10))


LDE_SHAPES = [(0, 3), (3, 0), (8, 2), (4, 7), (8, 3), (7, 4), (5, 6), (10, 1), (11, 0)]         # the smallest shape on every first-pass route


def test_lde_shape_list_reaches_every_route():
    names = {ls.route(log_n, lb, pre)[1] for log_n, lb in LDE_SHAPES for pre in (0, 1)}
    assert names == {ls.NO_EXTENSION, ls.PADDED, ls.FAST, ls.FAST_ZERO, ls.FAST_ZERO_ONE, ls.GENERAL, ls.UNIT}


def test_lde_first_pass_routes(oracle):
    cases = []
    for log_n, lb in LDE_SHAPES:
        x = oracle.synth_column(0xBA7C000 + 64 * log_n + lb, 0, 0, 1 << log_n)
        for g in (None, oracle.from_u64(5)):
            what = "lde (%d, %d), route '%s'" % (log_n, lb, ls.route(log_n, lb, g is not None)[1])
            cases.append((what, (lambda x, lb, g: lambda c: c.lde(x, lb, field=PALLAS_FR, coset=g))(x, lb, g), oracle.lde(0, x, lb, g)))
    with own_context() as c:
        under_both_fills(c, cases)


def batch_transform_cases(oracle, B):
    """stark_ntt_batch_dev at lg 12 (two passes: the scratch vector holds the batch) and lg 8, stark_lde_batch_dev at (8, 3) and (10, 1)"""
    import torch
    g = oracle.from_u64(5); cases = []
    for lg, inverse, coset in ((12, False, g), (12, True, None), (8, False, None)):
        xs = [oracle.synth_column(0xBA7C100 + lg, b, 0, 1 << lg) for b in range(B)]

        def run(c, xs=xs, lg=lg, inverse=inverse, coset=coset):
            d = [dev(x) for x in xs]
            c.ntt_batch_dev(PALLAS_FR, [t.data_ptr() for t in d], lg, inverse, coset); c.sync()
            return [host(t) for t in d]
        cases.append(("ntt batch, lg %d, B = %d" % (lg, B), run, [oracle.ntt(0, x, inverse=inverse, coset=coset) for x in xs]))
    for log_n, lb, coset in ((8, 3, g), (10, 1, None), (10, 1, g)):
        xs = [oracle.synth_column(0xBA7C200 + log_n, b, 0, 1 << log_n) for b in range(B)]

        def run(c, xs=xs, log_n=log_n, lb=lb, coset=coset):
            d = [dev(x) for x in xs]; outs = [torch.full((1 << (log_n + lb), 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda") for _ in xs]
            c.sync()
            c.lde_batch_dev(PALLAS_FR, [t.data_ptr() for t in d], log_n, lb, [o.data_ptr() for o in outs], coset); c.sync()
            return [host(o) for o in outs]
        cases.append(("lde batch (%d, %d), B = %d" % (log_n, lb, B), run, [oracle.lde(0, x, lb, coset) for x in xs]))
    return cases


@pytest.mark.parametrize("B,max_elems", [(3, None), (3, 1 << 11), (5, 1 << 12)])
def test_ntt_and_lde_batches(oracle, B, max_elems):
    """one pass for the whole batch; three passes of one column (each takes the single path); passes of 2, 2 and 1 columns at 2^11 outputs and of one
    column at 2^12 — a pass reads nothing the pass before it left in the scratch vector"""
    with own_context(**({} if max_elems is None else {"ntt_batch_max_elems": max_elems})) as c:
        under_both_fills(c, batch_transform_cases(oracle, B))


# ---- FRI --------------------------------------------------------------------------------------------------------------------------------------
def test_fri_fold(oracle):
    n = 4128                                                                  # 2 * 3 * 16 * 43: every m divides it, and the layer spans several workgroups
    f = oracle.synth_column(0xF01D, 0, 0, n); z = oracle.from_u64(0xC0FFEE)
    with own_context() as c:
        under_both_fills(c, [("fold, m = %d" % m, (lambda m: lambda c: c.fri_fold_layer(f, z, m))(m), oracle.fri_fold_layer(f, z, m)) for m in (2, 16, 3)])


@pytest.mark.parametrize("n0,sched", [(1 << 9, [8, 4, 2]), (1 << 11, [16, 16, 8])])
def test_fri_build_transcript(oracle, n0, sched):
    """every layer, root and fold challenge of the commit phase, with the small layers' trees on the side stream in the wave-pair form and in the latency forms"""
    f0 = oracle.rand_fr_columns(0xF0 + n0, n0, 1)[0]
    ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, 1, SEED_Z, f0=f0)
    L = len(sched)
    want = [ref.layer_f(l) for l in range(L + 1)] + [ref.root(l) for l in range(L + 1)] + [ref.z(l) for l in range(L)]
    ref.free()

    def run(c):
        st = c.fri_build_transcript(f0, sched, SEED_Z)
        try:
            assert st.num_layers == L + 1
            return [st.f_layer(l) for l in range(L + 1)] + [st.root(l) for l in range(L + 1)] + [st.z(l) for l in range(L)]
        finally:
            st.free()
    with own_context() as c:
        for side_pair in (1, 0):
            c.set_option("fri_side_pair", side_pair)
            under_both_fills(c, [("fri_build_transcript (%d, %s), fri_side_pair = %d" % (n0, sched, side_pair), run, want)])


@pytest.mark.parametrize("n0,sched,r", [(1 << 10, [16, 8], 8), (2, [2], 1)])
def test_deep_fri_prove(oracle, n0, sched, r):
    cols = oracle.rand_fr_columns(0xD0 + n0, n0, 4)
    ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, sched, r, SEED_Z)
    want = (ref.bytes(), ref.size_estimate()); ref.free()
    with own_context() as c:
        under_both_fills(c, [("deep_fri_prove (%d, %s, %d)" % (n0, sched, r), lambda c: c.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, SEED_Z))[:2], want)])


def test_ali_merge(oracle):
    """n = 1000: no power of two, the last workgroup ragged; plain with c*'s partial sums running, and blinded"""
    n = 1000
    cols = [oracle.synth_column(8, col, 0, n) for col in range(5)]
    omega, z, beta = oracle.root_of_unity(10), oracle.from_u64(0xC0FFEE), oracle.from_u64(12345)
    plain = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z)[0]
    blind = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z, r=cols[4], beta=beta, want_c_star=False)[0]
    with own_context() as c:
        under_both_fills(c, [("ali_merge, n = 1000", lambda c: c.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z)[0], plain),
                             ("ali_merge, n = 1000, blinded", lambda c: c.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z, r_eval=cols[4], beta=beta, want_c_star=False)[0], blind)])


def test_batched_prove_f0_and_commit_in_three_passes(oracle):
    """k = 10, B = 5 with passes of at most 2 n0 rows: two traces, two traces, one trace (which takes the single tail)"""
    k, B, sched, r = 10, 5, [16, 8], 8
    n0 = 1 << k; prm = DeepFriParams(sched, r, SEED_Z)
    traces = [oracle.rand_fr_columns(0x7A11 + b, n0, 4) for b in range(B)]
    f0s = oracle.rand_fr_columns(0xF00 + k, n0, B)
    want_prove, want_f0, want_roots = [], [], np.zeros((B, len(sched) + 1, 4), np.uint64)
    for b in range(B):
        ref = oracle.deep_fri_prove(traces[b][0], traces[b][1], traces[b][2], traces[b][3], n0, sched, r, SEED_Z)
        want_prove.append((ref.bytes(), ref.size_estimate())); ref.free()
        ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, r, SEED_Z, f0=f0s[b])
        want_f0.append((ref.bytes(), ref.size_estimate()))
        for l in range(len(sched) + 1):
            want_roots[b, l] = ref.root(l)
        ref.free()

    def prove(c):
        d = [[dev(col) for col in tr] for tr in traces]
        return [g[:2] for g in c.deep_fri_prove_batch_dev([[col.data_ptr() for col in tr] for tr in d], n0, prm)]

    def prove_f0(c):
        d = [dev(f) for f in f0s]
        return [g[:2] for g in c.deep_fri_prove_f0_batch_dev([f.data_ptr() for f in d], n0, prm)]

    def commit(c):
        d = [dev(f) for f in f0s]
        return c.fri_commit_batch_dev([f.data_ptr() for f in d], n0, sched, SEED_Z)
    with own_context(prove_batch_max_rows=2 * n0) as c:
        under_both_fills(c, [("deep_fri_prove_batch_dev", prove, want_prove), ("deep_fri_prove_f0_batch_dev", prove_f0, want_f0), ("fri_commit_batch_dev", commit, want_roots)])


# ---- sum-check --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 5, 12])
@pytest.mark.parametrize("mf", [0, 1])
def test_sumcheck_prove(oracle, mf, k):
    """prove_plain / prove_mf (q = 2) of one witness and of five in one pass"""
    B, q = 5, 2
    ws = oracle.rand_fr_columns(0x900 + 2 * k + mf, 1 << k, B); labels = [2025, 7, 2025, 11, 6060]
    want = [oracle.sumcheck_prove(mf, k, labels[b], ws[b], q=q) for b in range(B)]

    def batch(c):
        d = [dev(w) for w in ws]; ptrs = [t.data_ptr() for t in d]
        return c.prove_mf_batch_dev(k, labels, q, ptrs) if mf else c.prove_plain_batch_dev(k, labels, ptrs)
    single = lambda c: c.prove_mf(k, labels[0], q, ws[0]) if mf else c.prove_plain(k, labels[0], ws[0])
    with own_context() as c:
        under_both_fills(c, [("sum-check prove, mf = %d, k = %d, single" % (mf, k), single, want[0]), ("sum-check prove, mf = %d, k = %d, B = 5" % (mf, k), batch, want)])


@pytest.mark.parametrize("max_slots", [None, 1])
@pytest.mark.parametrize("mf", [0, 1])
def test_sumcheck_verify_batch(oracle, mf, max_slots):
    """k = 5, B = 8: eight honest proofs, and the same eight with one flipped byte each; max_slots = 1: one plan run per proof (eight runs)"""
    k, B, q = 5, 8, 2
    ws = oracle.rand_fr_columns(0x5C + mf, 1 << k, B); labels = [2025 + b for b in range(B)]
    honest = [oracle.sumcheck_prove(mf, k, labels[b], ws[b], q=q) for b in range(B)]
    flipped = []
    for b, p in enumerate(honest):
        bad = bytearray(p); bad[[8, 39, 40, len(p) - 1, len(p) - 33, len(p) // 2, len(p) // 3, 47][b]] ^= 1 << b; flipped.append(bytes(bad))
    want_h = [oracle.sumcheck_verify(mf, k, labels[b], honest[b], q=q) == 1 for b in range(B)]
    want_f = [oracle.sumcheck_verify(mf, k, labels[b], flipped[b], q=q) == 1 for b in range(B)]
    assert all(want_h) and not all(want_f)
    call = lambda ps: (lambda c: c.verify_mf_batch(k, labels, q, ps) if mf else c.verify_plain_batch(k, labels, ps))
    with own_context(**({} if max_slots is None else {"sumcheck_verify_batch_max_slots": max_slots})) as c:
        under_both_fills(c, [("sum-check verify, mf = %d, honest" % mf, call(honest), want_h), ("sum-check verify, mf = %d, one flipped byte each" % mf, call(flipped), want_f)])


# ---- verify -----------------------------------------------------------------------------------------------------------------------------------
def test_deep_fri_verify(oracle):
    with own_context() as c:
        under_both_fills(c, deep_fri_verify_cases(oracle, 1 << 9, [8, 4, 2], 5, 77))


def test_merkle_verify(oracle):
    """stark_merkle_verify_many_ds_batch and the single verify_many_ds over the openings and tamperings of merkle_batch_cases at (16, 257); the single
    verify_pairs_ds on a pair tree (4, 64), honest and with one flipped bit in cp"""
    arity, n, label = 16, 257, 0x5EED
    f = mc.leaves_of(oracle, SEED, 0, n); o = oracle.merkle_build(arity, label, f); ix = mc.index_lists(n, 1)
    items = [it[1:] for it in mc.tamperings(label, o.root(), ix, f[ix], o.open_bytes(ix), n)]; o.free()
    want = [mc.oracle_verify(arity, lab, root, i, v, pr) == 1 for lab, root, i, v, pr in items]
    assert want[0] and not any(want[1:])
    batch = lambda c: c.merkle_verify_single_batch(arity, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items], [it[3] for it in items], [it[4] for it in items])
    single = lambda c: [c.merkle_verify_single(c.merkle_cfg(arity, lab), root, i, v, pr) for lab, root, i, v, pr in items]
    pa, pn = 4, 64
    pf = mc.leaves_of(oracle, SEED, 1, pn); pc = mc.leaves_of(oracle, SEED, 101, pn); po = oracle.merkle_build(pa, label, pf, pc); pix = sorted({0, pn - 1, pn // 2})
    proot, ppr = po.root(), po.open_bytes(pix); po.free()
    bad = mc.flip_bit(pc[pix], 4 * 2 + 1, 9)
    want_pairs = [mc.oracle_verify_pairs(pa, label, proot, pix, pf[pix], cv, ppr) == 1 for cv in (pc[pix], bad)]
    assert want_pairs == [True, False]
    pairs = lambda c: [c.merkle_verify_pairs(c.merkle_cfg(pa, label), proot, pix, pf[pix], cv, ppr) for cv in (pc[pix], bad)]
    with own_context() as c:
        under_both_fills(c, [("merkle_verify_many_ds_batch", batch, want), ("merkle_verify_many_ds", single, want), ("merkle_verify_pairs_ds", pairs, want_pairs)])


# ---- MLE --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,log_tile", [(7, 3), (13, -1), (0, -1)])
def test_mle_evaluate(oracle, k, log_tile):
    """k = 7 in tiles of 2^3: three passes through pooled intermediate layers; k = 13 at the default tile: two; k = 0: none.  One table, and three in one batch."""
    import torch
    B = 3
    tabs, pts = mle.tables_and_points(oracle, k, B); want = mle.reference(oracle, tabs, k, pts)

    def batch(c):
        d = [dev(t) for t in tabs]; out = torch.full((B, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        c.sync(); c.mle_evaluate_batch_dev([t.data_ptr() for t in d], k, pts, out.data_ptr()); c.sync()
        return host(out)

    def single(c):
        d = dev(tabs[0]); out = torch.full((1, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        c.sync(); c.mle_evaluate_dev(d.data_ptr(), k, pts[0], out.data_ptr()); c.sync()
        return host(out)
    with own_context(mle_log_tile=log_tile) as c:
        under_both_fills(c, [("mle_evaluate_dev, k = %d" % k, single, want[:1]), ("mle_evaluate_batch_dev, k = %d, B = 3" % k, batch, want)])
