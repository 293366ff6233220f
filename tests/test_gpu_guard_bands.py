"""Where the device-pointer entry points write, not only what: every `*_dev` call of include/stark_mlwe.h on buffers that sit between guard bands.

Each case checks (a) the payload against the CPU oracle on the same inputs, bit for bit, (b) that the bands around every buffer are untouched and every
`const` input equals its host copy byte for byte, bands included, and, where the entry point has an output buffer, (c) that the result does not depend
on what the output held before: the case runs with the output pre-filled with the sentinel and again pre-filled with zeros.  Outputs and inputs of a
batch are consecutive payloads of ONE allocation with a sentinel row between them, so a wrong per-trace offset lands in a gap.  The sentinel is a
non-zero stored element (above the Pallas modulus): a read past the end of an input changes the result instead of reading zeros.
Left out: the stark_comm_*_dev collectives and the real stark_lde_sharded_dev / stark_fri_build_sharded_dev / stark_deep_fri_prove_sharded_dev, which
need a communicator (their phase code runs through the emulated entry points below); stark_lde_dev has its own test in test_gpu_lde_blowups.py.
The GPU tests need an MI355X (`pytest -m gpu`); the helper's own test runs on the CPU."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pyref

gpu = pytest.mark.gpu
vp = C.c_void_p
SENTINEL = 0x5A5A5A5A5A5A5A5A
BAND = 4096            # rows per side: the largest NTT tile (2^12 elements) and two merge workgroups
SEED_Z = 0xDEEFBAAD
PRIMES = {0: pyref.P_PALLAS, 1: pyref.P_BLS}
PREFILLS = (SENTINEL, 0)


def hp(a):
    """host pointer of a numpy array (None stays NULL)"""
    return None if a is None else a.ctypes.data_as(vp)


class Band:
    """One int64 tensor of band + payload rows + band rows of 4 words, filled with the sentinel.  `parts`: a row count (an output, pre-filled with
    `prefill`) or an (n, 4) uint64 array (an input) per payload; consecutive payloads are `gap` sentinel rows apart."""

    def __init__(self, parts, band=BAND, prefill=SENTINEL, device="cuda", gap=1):
        import torch
        self.band, self.spans = band, []
        rows = [p if isinstance(p, int) else p.shape[0] for p in parts]
        total = 2 * band + sum(rows) + gap * max(len(rows) - 1, 0)
        host = np.full((total, 4), SENTINEL, np.uint64)
        pos = band
        for p, n in zip(parts, rows):
            host[pos:pos + n] = prefill if isinstance(p, int) else p
            self.spans.append((pos, n)); pos += n + gap
        self.image = host                                                  # what the tensor held before the call
        self.guard = np.ones(total, bool)
        for s, n in self.spans:
            self.guard[s:s + n] = False
        self.buf = torch.from_numpy(host.view(np.int64).copy()).to(device)

    def view(self, i=0):
        s, n = self.spans[i]
        return self.buf[s:s + n]

    def ptr(self, i=0):
        return vp(self.buf.data_ptr() + 32 * self.spans[i][0])

    def host(self):
        return self.buf.cpu().numpy().view(np.uint64)

    def payload(self, i=0, host=None):
        s, n = self.spans[i]
        return (self.host() if host is None else host)[s:s + n]

    def _where(self, row):
        """(payload index, signed distance) of a guard row: rows in front of the nearest payload count negative, rows behind it from 1"""
        best = None
        for i, (s, n) in enumerate(self.spans):
            d = row - s if row < s else row - (s + n) + 1
            if best is None or abs(d) < abs(best[1]):
                best = (i, d)
        return best

    def dirty(self, host=None):
        """the first dirty row of every guard region (front band, gaps, back band) as (row, payload index, distance from that payload)"""
        host = self.host() if host is None else host
        bad = np.nonzero(self.guard & (host != SENTINEL).any(axis=1))[0]
        out, edges = [], [0] + [s for s, _ in self.spans] + [host.shape[0] + 1]
        for lo, hi in zip(edges[:-1], edges[1:]):
            r = bad[(bad >= lo) & (bad < hi)]
            if r.size:
                out.append((int(r[0]),) + self._where(int(r[0])))
        return out

    def check(self, what="", host=None):
        """both bands (and the gaps) still hold the sentinel"""
        d = self.dirty(host)
        assert not d, "%s: written outside the payload: %s" % (what, "; ".join(
            "row %d, %d row(s) %s payload %d" % (r, abs(k), "in front of" if k < 0 else "behind the end of", i) for r, i, k in d))

    def check_unchanged(self, what=""):
        """a const input: every byte, bands included, equals the host copy"""
        host = self.host()
        self.check(what, host)
        bad = np.nonzero((host != self.image).any(axis=1))[0]
        if bad.size:
            i = max(k for k, (s, _) in enumerate(self.spans) if s <= bad[0])
            raise AssertionError("%s: an input was modified, first at row %d of payload %d" % (what, bad[0] - self.spans[i][0], i))


def banded(rows_or_array, band=BAND, **kw):
    """-> (payload view, check) of one payload between two bands"""
    b = Band([rows_or_array], band=band, **kw)
    return b.view(0), b.check


# ---- the helper can fail (CPU, no GPU needed) --------------------------------------------------------------------------------------------
def test_band_check_reports_a_row_on_either_side():
    n, band = 10, 16
    data = np.arange(4 * n, dtype=np.uint64).reshape(n, 4)
    for arg in (n, data):
        view, check = banded(arg, band=band, device="cpu")
        assert view.shape == (n, 4)
        check()                                                            # untouched: passes
        view[:] = 7; check()                                               # writing the payload is allowed
    for row, text in ((band - 1, "row %d, 1 row(s) in front of payload 0" % (band - 1)), (band + n, "row %d, 1 row(s) behind the end of payload 0" % (band + n))):
        b = Band([n], band=band, device="cpu")
        b.buf[row, 2] = 0
        with pytest.raises(AssertionError) as e:
            b.check("case")
        assert text in str(e.value), str(e.value)
    b = Band([n], band=band, device="cpu")
    b.buf[band - 1, 0] = 1; b.buf[band + n, 3] = 1; b.buf[0, 0] = 1           # the first dirty row of each side is reported
    with pytest.raises(AssertionError) as e:
        b.check("both")
    assert "row 0, %d row(s) in front of payload 0" % band in str(e.value) and "row %d, 1 row(s) behind" % (band + n) in str(e.value)
    # two payloads: the gap row belongs to the guard, and an input must keep every byte
    b = Band([data, data[:3]], band=band, device="cpu")
    b.check_unchanged()
    assert b.spans == [(band, n), (band + n + 1, 3)] and (b.payload(1) == data[:3]).all()
    b.buf[band + n, 1] = 5
    with pytest.raises(AssertionError) as e:
        b.check("gap")
    assert "row %d, 1 row(s) behind the end of payload 0" % (band + n) in str(e.value)
    b = Band([data], band=band, device="cpu")
    b.buf[band + 4, 0] ^= 1
    b.check()
    with pytest.raises(AssertionError) as e:
        b.check_unchanged("input")
    assert "first at row 4 of payload 0" in str(e.value)


# ---- running a case ---------------------------------------------------------------------------------------------------------------------------
def sync(ctx):
    import torch
    ctx.sync(); torch.cuda.synchronize()


def same(got, want, what):
    want = np.ascontiguousarray(want, dtype=np.uint64).reshape(-1, 4)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d rows differ from the reference, first at row %d" % (what, bad.size, got.shape[0], bad[0] if bad.size else -1)


def guarded(ctx, ins, outs, call, wants, what, prefills=PREFILLS):
    """(a), (b), (c) for an entry point with output buffers.  ins: host arrays (each between its own bands) or ready Bands; outs: the row count of
    every output payload (one Band, gaps between); call(in_bands, out_band, prefill) -> status or a host result; wants: one reference per output
    payload, or a function of the pre-fill.  Returns what `call` returned per pre-fill."""
    inb = [x if isinstance(x, Band) else Band([x]) for x in ins]
    runs, rets = [], []
    for pre in prefills:
        ob = Band(list(outs), prefill=pre)
        sync(ctx)
        ret = call(inb, ob, pre)
        if isinstance(ret, int):
            ctx._chk(ret)
        sync(ctx)
        w = "%s, output pre-filled with %#x" % (what, pre)
        host = ob.host()
        ob.check(w, host)
        for b in inb:
            b.check_unchanged(w)
        got = [ob.payload(i, host) for i in range(len(outs))]
        for i, (g, want) in enumerate(zip(got, wants(pre) if callable(wants) else wants)):
            same(g, want, "%s, output %d" % (w, i))
        runs.append(got); rets.append(ret)
    if not callable(wants):
        for got in runs[1:]:
            assert all((a == b).all() for a, b in zip(runs[0], got)), "%s: the result depends on what the output held before" % what
    return rets


def in_place(ctx, x, call, want, what):
    """(a), (b) for an in-place entry point: the slab itself sits between the bands"""
    b = Band([x])
    sync(ctx)
    ctx._chk(call(b))
    sync(ctx)
    host = b.host()
    b.check(what, host)
    same(b.payload(0, host), want, what)


def preserved(ctx, bands, what):
    sync(ctx)
    for b in bands:
        b.check_unchanged(what)


def sched_arr(s):
    return np.ascontiguousarray(s, dtype=np.uint64)


def proof_out(ctx, h):
    return ctx._proof_out(h)[0]


# field arithmetic on stored (Montgomery) rows through Python integers: the six-step twiddles and pre-scales of the references
def to_ints(rows, field):
    return [pyref.from_limbs(r, PRIMES[field]) for r in rows]


def to_rows(vals, field):
    return np.array([pyref.to_limbs(v % PRIMES[field], PRIMES[field]) for v in vals], np.uint64).reshape(-1, 4)


def root_int(oracle, log_n, field):
    return pyref.from_limbs(oracle.root_of_unity(log_n, field), PRIMES[field])


def F(oracle, x, field=0):
    return oracle.from_u64(x, field)


# ---- FRI fold ----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("m,n", [(m, m * c) for m in (2, 16, 128) for c in (37, 300)] + [(3, 3 * 257), (6, 6 * 257)])
def test_fri_fold_dev(gpu_ctx, oracle, m, n):
    """stark_fri_fold_dev with an output count that is no multiple of the 256-thread block: the last block of k_fri_fold_pow2 is partial"""
    f = oracle.synth_column(0x6B01, m, 0, n); z = oracle.fri_sample_z_ell(SEED_Z, 0, 1 << 11)
    assert (n // m) % 256
    guarded(gpu_ctx, [f], [n // m], lambda i, o, _: gpu_ctx.lib.stark_fri_fold_dev(gpu_ctx.h, i[0].ptr(), n, hp(z), m, o.ptr()),
            [oracle.fri_fold_layer(f, z, m)], "stark_fri_fold_dev m = %d, n = %d" % (m, n))


# ---- DEEP-ALI merges --------------------------------------------------------------------------------------------------------------------------
def merge_inputs(oracle, seed, n):
    cols = [oracle.synth_column(seed, c, 0, n) for c in range(5)]
    lg = max(1, (n - 1).bit_length())
    return cols, lg, oracle.root_of_unity(lg), F(oracle, 0xC0FFEE), F(oracle, 12345)


@gpu
@pytest.mark.parametrize("n", [2, 1000, 2048, 4098])
def test_ali_merge_dev(gpu_ctx, oracle, n):
    """stark_ali_merge_dev with and without r_opt, with and without c_star; the domain generator has order 2^ceil(log2 n).  c* is a statement about
    the full domain: it is compared with the oracle when n is that order, and is independent of the pre-fill always."""
    cols, lg, omega, z, beta = merge_inputs(oracle, 0xA110 + n, n)
    inb = [Band([c]) for c in cols]
    for blind in (False, True):
        want_f0, want_cs = oracle.ali_merge(*cols[:4], omega, z, r=cols[4] if blind else None, beta=beta if blind else None)
        for with_cs in (False, True):
            what = "stark_ali_merge_dev n = %d, r_opt %s, c_star %s" % (n, blind, with_cs)

            def call(i, o, pre):
                cs = np.full(4, pre, np.uint64) if with_cs else None
                gpu_ctx._chk(gpu_ctx.lib.stark_ali_merge_dev(gpu_ctx.h, i[0].ptr(), i[1].ptr(), i[2].ptr(), i[3].ptr(), i[4].ptr() if blind else None,
                                                             hp(beta) if blind else None, hp(omega), hp(z), n, o.ptr(), hp(cs)))
                return cs
            cs = guarded(gpu_ctx, inb, [n], call, [want_f0], what)
            if with_cs:
                assert (cs[0] == cs[1]).all(), what
                if n == 1 << lg:
                    assert (cs[0] == want_cs).all(), what


@gpu
@pytest.mark.parametrize("j0", [0, 3096])
def test_ali_merge_shard_dev(gpu_ctx, oracle, j0):
    """stark_ali_merge_shard_dev on the block [j0, j0 + 1000) of a 4096-point domain against the matching slice of the oracle's whole merge; only the
    block is on the device, between bands.  The two blocks' partial sums are independent of the pre-fill."""
    ng, nl = 4096, 1000
    cols, lg, omega, z, _ = merge_inputs(oracle, 0xA115, ng)
    want = oracle.ali_merge(*cols[:4], omega, z)[0][j0:j0 + nl]
    for om in (None, omega):
        def call(i, o, pre):
            part = np.full(4, pre, np.uint64)
            gpu_ctx._chk(gpu_ctx.lib.stark_ali_merge_shard_dev(gpu_ctx.h, i[0].ptr(), i[1].ptr(), i[2].ptr(), i[3].ptr(), None, None, hp(om), hp(z), nl, j0, ng, o.ptr(), hp(part)))
            return part
        parts = guarded(gpu_ctx, [c[j0:j0 + nl] for c in cols[:4]], [nl], call, [want], "stark_ali_merge_shard_dev j0 = %d" % j0)
        assert (parts[0] == parts[1]).all() and (parts[0] != SENTINEL).any()


@gpu
@pytest.mark.parametrize("n", [64, 4096])
def test_ali_merge_batch_dev(gpu_ctx, oracle, n):
    """stark_ali_merge_batch_dev, B = 3 (trace 1 blinded): the three outputs are consecutive payloads one sentinel row apart, each trace's five
    tables likewise"""
    B = 3
    cols = oracle.rand_fr_columns(0xA11B + n, n, 5 * B).reshape(B, 5, n, 4)
    omega = oracle.domain_omega(n)
    zs = np.stack([F(oracle, 1000003 + 17 * b) for b in range(B)]); betas = np.stack([F(oracle, 77 + b) for b in range(B)])
    inb = [Band([cols[b, c] for c in range(5)]) for b in range(B)]
    want = [oracle.ali_merge(*cols[b, :4], omega, zs[b], r=cols[b, 4] if b == 1 else None, beta=betas[b] if b == 1 else None) for b in range(B)]

    def call(i, o, pre):
        traces = [[i[b].ptr(c).value for c in range(4)] for b in range(B)]
        return gpu_ctx.ali_merge_batch_dev(traces, omega, zs, n, [o.ptr(b).value for b in range(B)], [None, i[1].ptr(4).value, None], betas)
    cs = guarded(gpu_ctx, inb, [n] * B, call, [w[0] for w in want], "stark_ali_merge_batch_dev n = %d" % n)
    for got in cs:
        assert (got == np.stack([w[1] for w in want])).all()


# ---- Poseidon: leaf and level hashes, transcript hashes, permutations -----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", [(1, 1), (300, 4), (2049, 16), (4097, 2)])
def test_leaf_pair_hash_dev(gpu_ctx, oracle, n, m):
    f, fn = oracle.synth_column(0x1EAF, 0, 0, n), oracle.synth_column(0x1EAF, 1, 0, (n + m - 1) // m)
    tp = gpu_ctx.transcript_params().h
    guarded(gpu_ctx, [f, fn], [n], lambda i, o, _: gpu_ctx.lib.stark_leaf_pair_hash_dev(gpu_ctx.h, tp, i[0].ptr(), i[1].ptr(), n, m, o.ptr()),
            [oracle.leaf_pair_hash(f, fn, m)], "stark_leaf_pair_hash_dev n = %d, m = %d" % (n, m))
    guarded(gpu_ctx, [f], [n], lambda i, o, _: gpu_ctx.lib.stark_leaf_pair_hash_dev(gpu_ctx.h, None, i[0].ptr(), None, n, m, o.ptr()),
            [oracle.leaf_pair_hash(f, None, m)], "stark_leaf_pair_hash_dev n = %d, no next layer" % n)


def level_reference(oracle, arity, level, pos0, label, ch):
    """hash_with_ds_dynamic([arity, level, pos0 + k, label], children of node k) per node; the last node may be short"""
    t = 9 if arity <= 8 else 17 if arity <= 16 else 33
    nodes, full = (ch.shape[0] + arity - 1) // arity, ch.shape[0] // arity
    ds = np.array([[pyref.to_limbs(v) for v in (arity, level, pos0 + k, label)] for k in range(nodes)], np.uint64)
    out = np.zeros((nodes, 4), np.uint64)
    if full:
        out[:full] = oracle.hash_with_ds_dynamic(0, t, ds[:full], ch[:full * arity], arity, n=full).reshape(full, 4)
    if nodes > full:
        out[full] = oracle.hash_with_ds_dynamic(0, t, ds[full], ch[full * arity:], ch.shape[0] - full * arity)
    return out


@gpu
@pytest.mark.parametrize("arity,n_in", [(16, 3), (16, 256 * 16 + 3), (16, 4096 * 16 + 3), (8, 19), (32, 70)])
def test_poseidon_hash_ds_batch_dev(gpu_ctx, oracle, arity, n_in):
    """stark_poseidon_hash_ds_batch_dev with a ragged last node (arity 16: 1, 257 and 4097 nodes, the last of 3 children), in the default form and
    under poseidon_lane_only and sponge_one_wave"""
    level, pos0, label = 3, 32, 42
    ch = oracle.synth_column(0xD5, arity, 0, n_in)
    nodes = (n_in + arity - 1) // arity
    want = level_reference(oracle, arity, level, pos0, label, ch)
    p = gpu_ctx.poseidon_params_for_arity(arity)
    inb = [Band([ch])]
    for opt in (None, "poseidon_lane_only", "sponge_one_wave"):
        try:
            if opt:
                gpu_ctx.set_option(opt, 1)
            guarded(gpu_ctx, inb, [nodes], lambda i, o, _: gpu_ctx.lib.stark_poseidon_hash_ds_batch_dev(gpu_ctx.h, p.h, arity, level, pos0, label, i[0].ptr(), n_in, o.ptr()),
                    [want], "stark_poseidon_hash_ds_batch_dev arity %d, %d children, %s" % (arity, n_in, opt or "default form"))
        finally:
            if opt:
                gpu_ctx.set_option(opt, 0)


@gpu
@pytest.mark.parametrize("k,n", [(0, 3), (17, 3), (40, 513), (5, 4097)])
def test_tr_hash_fields_tagged_dev(gpu_ctx, oracle, k, n):
    fields = oracle.synth_column(0x7A6, k, 0, k * n) if k else np.zeros((0, 4), np.uint64)
    with ThreadPoolExecutor(8) as pool:                                        # the oracle hashes one transcript per call
        want = np.stack(list(pool.map(lambda i: oracle.tr_hash_fields_tagged(b"FRI/index", fields[i * k:(i + 1) * k]), range(n))))
    guarded(gpu_ctx, [fields], [n], lambda i, o, _: gpu_ctx.lib.stark_tr_hash_fields_tagged_dev(gpu_ctx.h, None, b"FRI/index", i[0].ptr(), k, n, o.ptr()),
            [want], "stark_tr_hash_fields_tagged_dev k = %d, n = %d" % (k, n))


@gpu
@pytest.mark.parametrize("nstates", [1, 65, 300])
@pytest.mark.parametrize("t", [9, 17, 33])
def test_poseidon_permute_batch_dev(gpu_ctx, oracle, t, nstates):
    st = oracle.synth_column(0x9E2, t, 0, nstates * t)
    p = gpu_ctx.poseidon_params_for_width(t)
    in_place(gpu_ctx, st, lambda b: gpu_ctx.lib.stark_poseidon_permute_batch_dev(gpu_ctx.h, p.h, b.ptr(), nstates), oracle.permute(0, t, st),
             "stark_poseidon_permute_batch_dev t = %d, %d states" % (t, nstates))


# ---- Merkle and the FRI commit -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("arity,n", [(16, 55), (8, 19), (2, 1), (64, 70)])
def test_merkle_build_dev(gpu_ctx, oracle, arity, n):
    leaves = oracle.synth_column(0x3E2, arity, 0, n)
    b = Band([leaves]); h = vp()
    sync(gpu_ctx)
    gpu_ctx._chk(gpu_ctx.lib.stark_merkle_build_dev(gpu_ctx.h, gpu_ctx.poseidon_params_for_arity(arity).h, arity, 7, b.ptr(), n, 0, None, 0, 0, 0, C.byref(h)))
    from stark_mlwe_amd.api import MerkleTree
    t = MerkleTree(gpu_ctx, h, None); o = oracle.merkle_build(arity, 7, leaves)
    try:
        preserved(gpu_ctx, [b], "stark_merkle_build_dev arity %d, %d leaves" % (arity, n))
        assert t.num_levels == o.num_levels()
        for lvl in range(t.num_levels):
            same(t.level(lvl), o.level(lvl), "level %d" % lvl)
        assert (t.root() == o.root()).all()
    finally:
        t.free(); o.free()


@gpu
@pytest.mark.parametrize("n0,sched", [(1 << 9, [8, 4, 2]), (1 << 7, [128])])
def test_fri_build_dev(gpu_ctx, oracle, n0, sched):
    """stark_fri_build_dev: f0 preserved, every layer and root the oracle's.  (2^7, [128]) is the first user of the t = 129 constants in a session
    and pays their one-time derivation, which the later arity-128 tests then find cached."""
    from stark_mlwe_amd.api import FriProverState
    f0 = oracle.synth_column(0xF21, 0, 0, n0)
    b = Band([f0]); h = vp(); sch = sched_arr(sched)
    sync(gpu_ctx)
    gpu_ctx._chk(gpu_ctx.lib.stark_fri_build_dev(gpu_ctx.h, b.ptr(), n0, hp(sch), len(sched), SEED_Z, C.byref(h)))
    st = FriProverState(gpu_ctx, h, sched); ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, 1, SEED_Z, f0=f0)
    try:
        preserved(gpu_ctx, [b], "stark_fri_build_dev 2^%d" % (n0.bit_length() - 1))
        assert st.num_layers == len(sched) + 1
        for l in range(st.num_layers):
            same(st.f_layer(l), ref.layer_f(l), "layer %d" % l)
            assert (st.root(l) == ref.root(l)).all(), l
    finally:
        st.free(); ref.free()


@gpu
@pytest.mark.parametrize("k,sched,r", [(6, [4, 2], 4), (10, [16, 8], 8)])
def test_fri_commit_batch_dev_and_prove_f0_batch_dev(gpu_ctx, oracle, k, sched, r):
    """stark_fri_commit_batch_dev and stark_deep_fri_prove_f0_batch_dev, B = 5: the f0 vectors are consecutive payloads one sentinel row apart; the
    host roots are pre-filled both ways"""
    from stark_mlwe_amd.api import DeepFriParams
    B, n0 = 5, 1 << k
    h = oracle.rand_fr_columns(0xF0B + k, n0, B)
    b = Band([h[i] for i in range(B)]); ptrs = [b.ptr(i).value for i in range(B)]
    refs = [oracle.deep_fri_prove(None, None, None, None, n0, sched, r, SEED_Z, f0=h[i]) for i in range(B)]
    try:
        want = np.stack([np.stack([p.root(l) for l in range(len(sched) + 1)]) for p in refs])
        tab = (vp * B)(*ptrs); sch = sched_arr(sched)
        for pre in PREFILLS:                                                # the host result buffer gets both pre-fills too
            roots = np.full((B, len(sched) + 1, 4), pre, np.uint64)
            sync(gpu_ctx)
            gpu_ctx._chk(gpu_ctx.lib.stark_fri_commit_batch_dev(gpu_ctx.h, B, tab, n0, hp(sch), len(sched), SEED_Z, hp(roots)))
            preserved(gpu_ctx, [b], "stark_fri_commit_batch_dev k = %d" % k)
            assert (roots == want).all(), (k, pre)
        sync(gpu_ctx)
        got = gpu_ctx.deep_fri_prove_f0_batch_dev(ptrs, n0, DeepFriParams(sched, r, SEED_Z))
        preserved(gpu_ctx, [b], "stark_deep_fri_prove_f0_batch_dev k = %d" % k)
        for i in range(B):
            assert got[i][0] == refs[i].bytes() and got[i][1] == refs[i].size_estimate(), (k, i)
    finally:
        for p in refs:
            p.free()


# ---- build_f0 and the provers ------------------------------------------------------------------------------------------------------------------
PROVE = (1 << 9, [8, 4, 2], 5)


@gpu
def test_build_f0_dev_and_deep_fri_prove_dev(gpu_ctx, oracle):
    """stark_build_f0_dev (f0 between bands, both pre-fills) and stark_deep_fri_prove_dev from the columns and from f0 alone, at 2^9 [8,4,2] r = 5"""
    n0, sched, r = PROVE
    cols = oracle.rand_fr_columns(0xB0F0, n0, 4); sch = sched_arr(sched)
    inb = [Band([c]) for c in cols]
    want_f0, want_aux = oracle.build_f0(*cols, n0)

    def call(i, o, pre):
        aux = np.full((7, 4), pre, np.uint64)
        gpu_ctx._chk(gpu_ctx.lib.stark_build_f0_dev(gpu_ctx.h, i[0].ptr(), i[1].ptr(), i[2].ptr(), i[3].ptr(), n0, o.ptr(), hp(aux)))
        return aux
    for aux in guarded(gpu_ctx, inb, [n0], call, [want_f0], "stark_build_f0_dev"):
        assert (aux == want_aux).all()
    h = vp()
    gpu_ctx._chk(gpu_ctx.lib.stark_deep_fri_prove_dev(gpu_ctx.h, inb[0].ptr(), inb[1].ptr(), inb[2].ptr(), inb[3].ptr(), None, n0, hp(sch), len(sched), r, SEED_Z, C.byref(h)))
    got = proof_out(gpu_ctx, h)
    preserved(gpu_ctx, inb, "stark_deep_fri_prove_dev from the columns")
    ref = oracle.deep_fri_prove(*cols, n0, sched, r, SEED_Z)
    assert got == ref.bytes(); ref.free()
    fb = Band([want_f0]); h = vp()
    sync(gpu_ctx)
    gpu_ctx._chk(gpu_ctx.lib.stark_deep_fri_prove_dev(gpu_ctx.h, None, None, None, None, fb.ptr(), n0, hp(sch), len(sched), r, SEED_Z, C.byref(h)))
    got = proof_out(gpu_ctx, h)
    preserved(gpu_ctx, [fb], "stark_deep_fri_prove_dev from f0")
    ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, r, SEED_Z, f0=want_f0)
    assert got == ref.bytes(); ref.free()


@gpu
def test_deep_fri_prove_batch_dev(gpu_ctx, oracle):
    """stark_deep_fri_prove_batch_dev, B = 3 at 2^9: the four columns of a trace are consecutive payloads"""
    from stark_mlwe_amd.api import DeepFriParams
    n0, sched, r = PROVE; B = 3
    cols = oracle.rand_fr_columns(0xBA7C, n0, 4 * B).reshape(B, 4, n0, 4)
    inb = [Band([cols[b, c] for c in range(4)]) for b in range(B)]
    sync(gpu_ctx)
    got = gpu_ctx.deep_fri_prove_batch_dev([[inb[b].ptr(c).value for c in range(4)] for b in range(B)], n0, DeepFriParams(sched, r, SEED_Z))
    preserved(gpu_ctx, inb, "stark_deep_fri_prove_batch_dev")
    for b in range(B):
        ref = oracle.deep_fri_prove(*cols[b], n0, sched, r, SEED_Z)
        assert got[b][0] == ref.bytes() and got[b][1] == ref.size_estimate(), b
        ref.free()


@gpu
def test_sharded_emulated_commit_and_prove(gpu_ctx, oracle):
    """stark_diag_fri_build_sharded_emulated_dev and stark_diag_deep_fri_prove_sharded_emulated_dev, W = 2 at 2^10: the whole inputs are preserved,
    every virtual rank's roots and proof bytes are the oracle's"""
    from stark_mlwe_amd.api import DeepFriParams
    W, n0, sched, r = 2, 1 << 10, [16, 8], 8
    cols = oracle.rand_fr_columns(0x5BA2, n0, 4); sch = sched_arr(sched)
    f0 = oracle.build_f0(*cols, n0)[0]
    ref = oracle.deep_fri_prove(*cols, n0, sched, r, SEED_Z)
    try:
        want_roots = np.stack([ref.root(l) for l in range(len(sched) + 1)])
        fb = Band([f0])
        for pre in PREFILLS:
            roots = np.full((W, len(sched) + 1, 4), pre, np.uint64)
            sync(gpu_ctx)
            gpu_ctx._chk(gpu_ctx.lib.stark_diag_fri_build_sharded_emulated_dev(gpu_ctx.h, W, fb.ptr(), n0, hp(sch), len(sched), SEED_Z, hp(roots)))
            preserved(gpu_ctx, [fb], "stark_diag_fri_build_sharded_emulated_dev")
            for q in range(W):
                assert (roots[q] == want_roots).all(), (q, pre)
        inb = [Band([c]) for c in cols]
        sync(gpu_ctx)
        proofs = gpu_ctx.diag_deep_fri_prove_sharded_emulated(W, *[b.ptr().value for b in inb], n0, DeepFriParams(sched, r, SEED_Z))
        preserved(gpu_ctx, inb, "stark_diag_deep_fri_prove_sharded_emulated_dev")
        assert len(proofs) == W
        for q in range(W):
            assert proofs[q][0] == ref.bytes() and proofs[q][1] == ref.size_estimate(), q
    finally:
        ref.free()


# ---- sum-check -----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [1, 5])
def test_sumcheck_prove_dev(gpu_ctx, oracle, k):
    """stark_sumcheck_prove_plain_dev and stark_sumcheck_prove_mf_dev: witness preserved, bytes the oracle's"""
    w = oracle.rand_fr_columns(0x5C0 + k, 1 << k, 1)[0]; q, label = 2, 77
    b = Band([w])
    for mf in (0, 1):
        h = vp()
        sync(gpu_ctx)
        if mf:
            gpu_ctx._chk(gpu_ctx.lib.stark_sumcheck_prove_mf_dev(gpu_ctx.h, b.ptr(), k, label, q, C.byref(h)))
        else:
            gpu_ctx._chk(gpu_ctx.lib.stark_sumcheck_prove_plain_dev(gpu_ctx.h, b.ptr(), k, label, C.byref(h)))
        got = proof_out(gpu_ctx, h)
        preserved(gpu_ctx, [b], "sum-check prove, mf = %d, k = %d" % (mf, k))
        assert got == oracle.sumcheck_prove(mf, k, label, w, q=q), (mf, k)


@gpu
def test_sumcheck_prove_batch_dev(gpu_ctx, oracle):
    """stark_sumcheck_prove_plain_batch_dev and stark_sumcheck_prove_mf_batch_dev, B = 3, k = 5: the witnesses are consecutive payloads"""
    B, k, q = 3, 5, 2
    ws = oracle.rand_fr_columns(0x5CB, 1 << k, B); labels = [11, 22, 33]
    b = Band([ws[i] for i in range(B)]); ptrs = [b.ptr(i).value for i in range(B)]
    for mf in (0, 1):
        sync(gpu_ctx)
        got = gpu_ctx.prove_mf_batch_dev(k, labels, q, ptrs) if mf else gpu_ctx.prove_plain_batch_dev(k, labels, ptrs)
        preserved(gpu_ctx, [b], "sum-check batch prove, mf = %d" % mf)
        for i in range(B):
            assert got[i] == oracle.sumcheck_prove(mf, k, labels[i], ws[i], q=q), (mf, i)


# ---- NTT ---------------------------------------------------------------------------------------------------------------------------------------
GEN = {0: 5, 1: 7}


@gpu
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n", [0, 1, 10, 11, 13])
def test_ntt_dev(gpu_ctx, oracle, field, log_n):
    """stark_ntt_dev in place: forward, inverse and on the coset of the generator; one pass, the smallest two-pass size and a general two-pass size"""
    x = oracle.synth_column(0x277, log_n, 0, 1 << log_n)                      # below 2^254: elements of both fields
    g = F(oracle, GEN[field], field)
    for inverse, coset in ((0, None), (1, None), (0, g)):
        in_place(gpu_ctx, x, lambda b: gpu_ctx.lib.stark_ntt_dev(gpu_ctx.h, field, b.ptr(), log_n, inverse, hp(coset)),
                 oracle.ntt(field, x, inverse=bool(inverse), coset=coset), "stark_ntt_dev field %d, 2^%d, inverse %d, coset %s" % (field, log_n, inverse, coset is not None))


@gpu
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("W", [2, 4])
def test_lde_sharded_emulated_dev(gpu_ctx, oracle, field, W):
    log_n, lb = 8, 2
    ev = oracle.synth_column(0xE3D, W, 0, 1 << log_n); sh = F(oracle, GEN[field], field)
    guarded(gpu_ctx, [ev], [1 << (log_n + lb)], lambda i, o, _: gpu_ctx.lib.stark_diag_lde_sharded_emulated_dev(gpu_ctx.h, field, W, i[0].ptr(), log_n, lb, hp(sh), o.ptr()),
            [oracle.lde(field, ev, lb, sh)], "stark_diag_lde_sharded_emulated_dev field %d, W = %d" % (field, W))


@gpu
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("nrows,log_cols", [(1, 6), (3, 6), (5, 11)])
def test_ntt_rows_dev(gpu_ctx, oracle, field, nrows, log_cols):
    """stark_ntt_rows_dev in place: forward; inverse with scale4 = N^-1 (N = 8 * 2^log_cols, a whole transform these rows would be a phase of): every
    output is the unscaled inverse times N^-1; inverse with scale4 = NULL: no per-row n^-1, the oracle's inverse times 2^log_cols"""
    p, n = PRIMES[field], 1 << log_cols
    x = oracle.synth_column(0x205, nrows, 0, nrows * n)
    rows = [x[i * n:(i + 1) * n] for i in range(nrows)]
    fwd = np.concatenate([oracle.ntt(field, r) for r in rows])
    inv = [v for r in rows for v in to_ints(oracle.ntt(field, r, inverse=True), field)]
    ninv = pow(8 * n, -1, p); scale = to_rows([ninv], field)[0]
    for inverse, sc, want in ((0, None, fwd), (1, scale, to_rows([v * n * ninv for v in inv], field)), (1, None, to_rows([v * n for v in inv], field))):
        in_place(gpu_ctx, x, lambda b: gpu_ctx.lib.stark_ntt_rows_dev(gpu_ctx.h, field, b.ptr(), nrows, log_cols, inverse, hp(sc)), want,
                 "stark_ntt_rows_dev field %d, %d rows of 2^%d, inverse %d, scale4 %s" % (field, nrows, log_cols, inverse, sc is not None))


SIX = dict(log_n=12, log_rows=6, ncols=16)


@gpu
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("col0", [0, 48])
def test_ntt_columns_dev_and_coset(gpu_ctx, oracle, field, col0):
    """stark_ntt_columns_dev (forward, inverse) and stark_ntt_columns_coset_dev in place on a [64][16] slab of the 64 columns of a 2^12-point
    six-step transform.  The expected slab is the six-step identity: out[k][c] = w_N^(+-(col0 + c) k) * DFT_64(column c)[k] (the inverse phase is
    unscaled: N^-1 enters once, in the row phase), and for the coset form x[j] *= shift^j first, j = row * 64 + col0 + c."""
    log_n, log_rows, ncols = SIX["log_n"], SIX["log_rows"], SIX["ncols"]
    p, R, Cc = PRIMES[field], 1 << log_rows, 1 << (log_n - log_rows)
    slab = oracle.synth_column(0xC01, col0, 0, R * ncols).reshape(R, ncols, 4)
    wN = root_int(oracle, log_n, field); shift = GEN[field]

    def expected(src, inverse):
        out = np.zeros_like(src)
        w = pow(wN, -1, p) if inverse else wN
        for c in range(ncols):
            col = to_ints(oracle.ntt(field, src[:, c], inverse=inverse), field)
            out[:, c] = to_rows([v * (R if inverse else 1) * pow(w, (col0 + c) * k, p) for k, v in enumerate(col)], field)
        return out

    for inverse in (0, 1):
        in_place(gpu_ctx, slab.reshape(-1, 4), lambda b: gpu_ctx.lib.stark_ntt_columns_dev(gpu_ctx.h, field, b.ptr(), log_rows, ncols, col0, log_n, inverse),
                 expected(slab, bool(inverse)), "stark_ntt_columns_dev field %d, col0 = %d, inverse %d" % (field, col0, inverse))
    pre = np.stack([to_rows([v * pow(shift, row * Cc + col0 + c, p) for c, v in enumerate(to_ints(slab[row], field))], field) for row in range(R)])
    sh = F(oracle, shift, field)
    in_place(gpu_ctx, slab.reshape(-1, 4), lambda b: gpu_ctx.lib.stark_ntt_columns_coset_dev(gpu_ctx.h, field, b.ptr(), log_rows, ncols, col0, log_n, hp(sh)),
             expected(pre, False), "stark_ntt_columns_coset_dev field %d, col0 = %d" % (field, col0))


@gpu
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("row0", [0, 48])
def test_ntt_rows_coset_dev(gpu_ctx, oracle, field, row0):
    """stark_ntt_rows_coset_dev: dst[i][m] = w_n^(k1 m) * sum_k' src[i][k'] shift^(k' R + k1) w_C^(k' m), k1 = row0 + i; src is preserved"""
    log_n, log_cols, nrows = 12, 6, 16
    p, Cc, R = PRIMES[field], 1 << log_cols, 1 << (log_n - log_cols)
    src = oracle.synth_column(0xC02, row0, 0, nrows * Cc).reshape(nrows, Cc, 4)
    wn = root_int(oracle, log_n, field); shift = GEN[field]; sh = F(oracle, shift, field)
    want = np.zeros_like(src)
    for i in range(nrows):
        k1 = row0 + i
        pre = to_rows([v * pow(shift, kp * R + k1, p) for kp, v in enumerate(to_ints(src[i], field))], field)
        want[i] = to_rows([v * pow(wn, k1 * m, p) for m, v in enumerate(to_ints(oracle.ntt(field, pre), field))], field)
    guarded(gpu_ctx, [src.reshape(-1, 4)], [nrows * Cc],
            lambda i, o, _: gpu_ctx.lib.stark_ntt_rows_coset_dev(gpu_ctx.h, field, i[0].ptr(), o.ptr(), nrows, log_cols, row0, log_n, hp(sh)),
            [want], "stark_ntt_rows_coset_dev field %d, row0 = %d" % (field, row0))
    b = Band([src.reshape(-1, 4)])
    assert gpu_ctx.lib.stark_ntt_rows_coset_dev(gpu_ctx.h, field, b.ptr(), b.ptr(), nrows, log_cols, row0, log_n, hp(sh)) == -1      # src == dst is rejected
    preserved(gpu_ctx, [b], "stark_ntt_rows_coset_dev with src == dst")


# ---- layout kernels, power tables, synthetic columns ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims,perm", [((3, 5, 7), q) for q in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))] + [((2, 300, 1), (1, 0, 2)), ((2, 300, 1), (2, 1, 0))])
def test_permute3_dev(gpu_ctx, oracle, dims, perm):
    n = dims[0] * dims[1] * dims[2]
    src = oracle.synth_column(0x9E3, 0, 0, n)
    want = np.ascontiguousarray(np.transpose(src.reshape(*dims, 4), perm + (3,))).reshape(-1, 4)
    guarded(gpu_ctx, [src], [n], lambda i, o, _: gpu_ctx.lib.stark_permute3_dev(gpu_ctx.h, i[0].ptr(), o.ptr(), *dims, *perm), [want],
            "stark_permute3_dev dims %s, permutation %s" % (dims, perm))


@gpu
@pytest.mark.parametrize("n,stride,offset", [(300, 4, 3), (257, 1, 0), (5, 64, 63)])
def test_interleave_dev(gpu_ctx, oracle, n, stride, offset):
    """stark_interleave_dev: dst[k * stride + offset] = src[k]; every other row of dst still holds the pre-fill"""
    src = oracle.synth_column(0x171, stride, 0, n)

    def want(pre):
        w = np.full((n * stride, 4), pre, np.uint64); w[offset::stride] = src
        return [w]
    guarded(gpu_ctx, [src], [n * stride], lambda i, o, _: gpu_ctx.lib.stark_interleave_dev(gpu_ctx.h, i[0].ptr(), o.ptr(), n, stride, offset), want,
            "stark_interleave_dev n = %d, stride %d, offset %d" % (n, stride, offset))


@gpu
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 1000, 1025])
def test_compute_powers_dev(gpu_ctx, oracle, field, n):
    """stark_compute_powers_dev: the two-level table covers 2^(bits + 1) > n entries, the output exactly n; reference by repeated multiplication"""
    base = oracle.from_int(pow(3, 1000003, PRIMES[field]), field)
    want = np.zeros((n, 4), np.uint64); want[0] = F(oracle, 1, field)
    for i in range(1, n):
        want[i] = oracle.mul(want[i - 1], base, field)
    guarded(gpu_ctx, [], [n], lambda i, o, _: gpu_ctx.lib.stark_compute_powers_dev(gpu_ctx.h, field, hp(base), n, o.ptr()), [want],
            "stark_compute_powers_dev field %d, n = %d" % (field, n))


@gpu
def test_synth_column_dev(gpu_ctx, oracle):
    n, i0 = 1000, 12345
    guarded(gpu_ctx, [], [n], lambda i, o, _: gpu_ctx.lib.stark_synth_column_dev(gpu_ctx.h, 0x5EED0014, 2, i0, n, o.ptr()),
            [oracle.synth_column(0x5EED0014, 2, i0, n)], "stark_synth_column_dev")
