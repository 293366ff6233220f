"""The cases of tests/test_gpu_alloc_refusal.py: (name, run(c) -> result, the oracle's result) over every family of entry points, at the smallest
shapes the suite already trusts to cross every kernel form.  The tables of tests/test_gpu_pool_poison.py are taken as they are (tree_case, leaf_case,
ntt_cases, batch_transform_cases, deep_fri_verify_cases); its inline cases are restated here with the same shapes and seeds; the rest come from the
case modules of their own tests.  A run frees every handle it made, whatever happens, and a run that fails raises StarkError before it made one.
Every reference is computed once per session (`group()` memoises the tables) and never written to.

The shapes whose Poseidon width is 65 or 129 are kept out of the COLD sweeps (test_wide_widths; the [128] trace of mixed_prove_cases.PROVE_ORDER): a
context derives the kernel constants of a width on the host when it first meets it — minutes at t = 129 — and a cold sweep makes a context per
request.  The whole PROVE_ORDER runs warm and in the retry modes on the session's context (SESSION_GROUPS)."""
import ctypes as C

import numpy as np

import corner_values as cv
import lagrange_cases as lc
import lagrange_shard_cases as lsc
import merkle_batch_cases as mc
import mixed_batch_cases as xc
import mixed_prove_cases as mp
import mle_cases as mle
import pyref
import test_gpu_pool_poison as pp
from stark_mlwe_amd.api import PALLAS_FR, DeepFriParams

SEED_Z = pp.SEED_Z
vp = C.c_void_p
dev, host = pp.dev, pp.host
SENTINEL = 0x5A5A5A5A5A5A5A5A
MIXED_LOGS, MIXED_BLOWUP = [8, 5, 11], 3                       # tests/test_gpu_lde_mixed_batch.py SMALL
BIG_LOG = 21                                                   # the smallest three-pass NTT plan (ntt_split): the only one with two tw_direct tables
_memo = {}


def out_rows(n):
    import torch
    return torch.full((n, 4), SENTINEL, dtype=torch.int64, device="cuda")


def fold_cases(oracle):
    n = 4128; f = oracle.synth_column(0xF01D, 0, 0, n); z = oracle.from_u64(0xC0FFEE)
    return [("fold, m = %d" % m, (lambda m: lambda c: c.fri_fold_layer(f, z, m))(m), oracle.fri_fold_layer(f, z, m)) for m in (2, 16, 3)]


def fri_build_case(oracle, n0, sched):
    f0 = oracle.rand_fr_columns(0xF0 + n0, n0, 1)[0]
    ref = oracle.deep_fri_prove(None, None, None, None, n0, sched, 1, SEED_Z, f0=f0); L = len(sched)
    want = [ref.layer_f(l) for l in range(L + 1)] + [ref.root(l) for l in range(L + 1)] + [ref.z(l) for l in range(L)]
    ref.free()

    def run(c):
        st = c.fri_build_transcript(f0, sched, SEED_Z)
        try:
            return [st.f_layer(l) for l in range(L + 1)] + [st.root(l) for l in range(L + 1)] + [st.z(l) for l in range(L)]
        finally:
            st.free()
    return [("fri_build_transcript (%d, %s)" % (n0, sched), run, want)]


def prove_case(oracle, n0, sched, r):
    cols = oracle.rand_fr_columns(0xD0 + n0, n0, 4)
    ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, sched, r, SEED_Z)
    want = (ref.bytes(), ref.size_estimate()); ref.free()
    return [("deep_fri_prove (%d, %s, %d)" % (n0, sched, r), lambda c: c.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, DeepFriParams(sched, r, SEED_Z))[:2], want)]


def ali_merge_cases(oracle):
    n = 1000
    cols = [oracle.synth_column(8, col, 0, n) for col in range(5)]
    omega, z, beta = oracle.root_of_unity(10), oracle.from_u64(0xC0FFEE), oracle.from_u64(12345)
    plain = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z)[0]
    blind = oracle.ali_merge(cols[0], cols[1], cols[2], cols[3], omega, z, r=cols[4], beta=beta, want_c_star=False)[0]
    return [("ali_merge, n = 1000", lambda c: c.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z)[0], plain),
            ("ali_merge, n = 1000, blinded", lambda c: c.deep_ali_merge_evals(cols[0], cols[1], cols[2], cols[3], omega, z, r_eval=cols[4], beta=beta, want_c_star=False)[0], blind)]


PROVE3 = dict(k=10, B=5, sched=[16, 8], r=8)                   # test_batched_prove_f0_and_commit_in_three_passes: under prove_batch_max_rows = 2 n0 passes of 2, 2 and 1 traces


def batched_prove_cases(oracle):
    """-> [prove, f0, commit]: they need the context option prove_batch_max_rows = 2 * 2^k (options_of)"""
    k, B, sched, r = PROVE3["k"], PROVE3["B"], PROVE3["sched"], PROVE3["r"]
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
    return [("deep_fri_prove_batch_dev, three passes", prove, want_prove), ("deep_fri_prove_f0_batch_dev, three passes", prove_f0, want_f0),
            ("fri_commit_batch_dev, three passes", commit, want_roots)]


def sumcheck_prove_cases(oracle, mf, k):
    if ("sc", mf, k) in _memo:
        return _memo[("sc", mf, k)]
    B, q = 5, 2
    ws = oracle.rand_fr_columns(0x900 + 2 * k + mf, 1 << k, B); labels = [2025, 7, 2025, 11, 6060]
    want = [oracle.sumcheck_prove(mf, k, labels[b], ws[b], q=q) for b in range(B)]

    def batch(c):
        d = [dev(w) for w in ws]; ptrs = [t.data_ptr() for t in d]
        return c.prove_mf_batch_dev(k, labels, q, ptrs) if mf else c.prove_plain_batch_dev(k, labels, ptrs)
    single = lambda c: c.prove_mf(k, labels[0], q, ws[0]) if mf else c.prove_plain(k, labels[0], ws[0])
    _memo[("sc", mf, k)] = [("sum-check prove, mf = %d, k = %d, single" % (mf, k), single, want[0]), ("sum-check prove, mf = %d, k = %d, B = 5" % (mf, k), batch, want)]
    return _memo[("sc", mf, k)]


def sumcheck_verify_cases(oracle, mf):
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
    return [("sum-check verify, mf = %d, honest" % mf, call(honest), want_h), ("sum-check verify, mf = %d, one flipped byte each" % mf, call(flipped), want_f)]


def merkle_verify_cases(oracle):
    arity, n, label = 16, 257, 0x5EED
    f = mc.leaves_of(oracle, pp.SEED, 0, n); o = oracle.merkle_build(arity, label, f); ix = mc.index_lists(n, 1)
    items = [it[1:] for it in mc.tamperings(label, o.root(), ix, f[ix], o.open_bytes(ix), n)]; o.free()
    want = [mc.oracle_verify(arity, lab, root, i, v, pr) == 1 for lab, root, i, v, pr in items]
    assert want[0] and not any(want[1:])
    batch = lambda c: c.merkle_verify_single_batch(arity, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items], [it[3] for it in items], [it[4] for it in items])
    single = lambda c: [c.merkle_verify_single(c.merkle_cfg(arity, lab), root, i, v, pr) for lab, root, i, v, pr in items[:3]]
    return [("merkle_verify_many_ds_batch", batch, want), ("merkle_verify_many_ds", single, want[:3])]


def mle_cases(oracle, k, B=3):
    tabs, pts = mle.tables_and_points(oracle, k, B); want = mle.reference(oracle, tabs, k, pts)

    def batch(c):
        d = [dev(t) for t in tabs]; out = out_rows(B)
        c.sync(); c.mle_evaluate_batch_dev([t.data_ptr() for t in d], k, pts, out.data_ptr()); c.sync()
        return host(out)
    return [("mle_evaluate_batch_dev, k = %d, B = 3" % k, batch, want)]


def lagrange_cases(oracle):
    """the batch call on whole columns (two points outside H, two inside), one block's share, the combination of the shares"""
    n = 1 << 12; cols = lc.columns(oracle, n, 3)
    inside = lc.inside_points(oracle, n)[:2]
    zs = np.ascontiguousarray(np.concatenate([lc.points(oracle, n, 2)] + [z.reshape(1, 4) for z, _ in inside]))
    want = np.concatenate([lc.matrix_reference(oracle, n)[:2, :3]] + [np.stack([v[j] for v in cols]).reshape(1, 3, 4) for _, j in inside])
    P = zs.shape[0]

    def batch(c):
        d = [dev(v) for v in cols]; out = out_rows(P * 3)
        c.sync(); c.lagrange_eval_on_h_batch_dev([t.data_ptr() for t in d], n, zs, out.data_ptr()); c.sync()
        return host(out).reshape(P, 3, 4)
    _, blocks = lsc.PARTITIONS[5]                                           # uneven blocks of 2^12: 1000, 1, 3095 rows

    def shares_of(c):
        parts = out_rows(len(blocks) * P * 3); keep = []
        for q, (j0, nl) in enumerate(blocks):
            d = [dev(v[j0:j0 + nl]) for v in cols]; keep.append(d)
            c.lagrange_eval_shard_dev([t.data_ptr() for t in d], nl, j0, n, zs, parts.data_ptr() + 32 * q * P * 3)
        c.sync()
        return parts, keep

    def sharded(c):
        parts, keep = shares_of(c); out = out_rows(P * 3)
        c.lagrange_eval_from_partials_dev(len(blocks), parts.data_ptr(), 3, n, zs, out.data_ptr()); c.sync()
        return host(out).reshape(P, 3, 4)
    return [("lagrange_eval_on_h_batch_dev, n = 2^12", batch, want), ("lagrange_eval_shard_dev x 3 + from_partials_dev, n = 2^12", sharded, want)]


def mixed_merkle_cases(oracle):
    """stark_merkle_build_mixed_batch_dev over the arity-16 set (pair leaves, real and NULL cp entries) and the mixed commit over the same lengths"""
    arity = 16; ns = xc.SETS[arity]; labels = xc.labels_of(len(ns))
    cols = [xc.leaves_of(oracle, b, n) for b, n in enumerate(ns)]; cps = xc.cps_of(oracle, ns)
    want_pairs = [xc.oracle_tree(oracle, arity, b, n, True, labels[b]) for b, n in enumerate(ns)]
    want = [[t.level(v) for v in range(t.num_levels())] for t in want_pairs]
    commit_want = [oracle.commitment_root(labels[b], cols[b]) for b in range(len(ns))]

    def build(c):
        d = [dev(v) for v in cols]; dc = [None if v is None else dev(v) for v in cps]
        trees = c.merkle_build_mixed_batch_dev([t.data_ptr() for t in d], ns, arity, labels, c.poseidon_params_for_arity(arity), cp=[None if t is None else t.data_ptr() for t in dc])
        try:
            return [t.levels for t in trees]
        finally:
            for t in trees:
                t.free()

    def commit(c):
        d = [dev(v) for v in cols]
        trees = c.commitment_commit_mixed_batch_dev(labels, [t.data_ptr() for t in d], ns)
        try:
            return [r for r in c.merkle_roots_batch(trees)]
        finally:
            for t in trees:
                t.free()
    return [("merkle_build_mixed_batch_dev, pairs, arity 16", build, want), ("commitment_commit_mixed_batch_dev", commit, commit_want)]


def mixed_prove_case(oracle, with_128):
    """mixed_prove_cases.PROVE_ORDER: seven traces, a group of three (2^6), a group of two (2^10), two singletons (2^7 under [128], 2^8 unfolded).
    with_128 False: without the [128] trace, whose t = 129 constants a context derives for minutes (the cold sweep makes a context per request)"""
    order = [k for k in mp.PROVE_ORDER if with_128 or k != 7]
    shapes = [(1 << k,) + mp.PROVE_SHAPES[k] for k in order]
    traces = [oracle.rand_fr_columns(mp.SEED + i, sh[0], 4) for i, sh in enumerate(shapes)]
    want = []
    for tr, (n0, sched, r) in zip(traces, shapes):
        ref = oracle.deep_fri_prove(tr[0], tr[1], tr[2], tr[3], n0, sched, r, SEED_Z); want.append((ref.bytes(), ref.size_estimate())); ref.free()

    def run(c):
        d = [[dev(col) for col in tr] for tr in traces]
        return [g[:2] for g in c.deep_fri_prove_mixed_batch_dev([[col.data_ptr() for col in tr] for tr in d], shapes, SEED_Z)]
    return [("deep_fri_prove_mixed_batch_dev, %d traces of %d shapes" % (len(order), len(set(order))), run, want)]


def mixed_lde_inputs(oracle):
    return [oracle.synth_column(0xBA7C300 + lg, b, 0, 1 << lg) for b, lg in enumerate(MIXED_LOGS)]


def mixed_lde_run(xs, g, logs=None):
    logs = MIXED_LOGS if logs is None else logs

    def run(c):
        d = [dev(x) for x in xs]; outs = [out_rows(1 << (lg + MIXED_BLOWUP)) for lg in logs]
        c.sync(); c.lde_mixed_batch_dev(PALLAS_FR, [t.data_ptr() for t in d], logs, MIXED_BLOWUP, [o.data_ptr() for o in outs], g); c.sync()
        return [host(o) for o in outs]
    return run


def mixed_transform_cases(oracle):
    """stark_lde_mixed_batch_dev of {8, 5, 11} at blow-up 3 on the generator's coset, and stark_ntt_mixed_batch_dev of {11, 3, 10}"""
    g = oracle.from_u64(5); xs = mixed_lde_inputs(oracle)
    nl = [11, 3, 10]; ys = [oracle.synth_column(0xBA7C400 + lg, b, 0, 1 << lg) for b, lg in enumerate(nl)]

    def ntt(c):
        d = [dev(y) for y in ys]
        c.ntt_mixed_batch_dev(PALLAS_FR, [t.data_ptr() for t in d], nl, False, g); c.sync()
        return [host(t) for t in d]
    return [("lde_mixed_batch_dev {8, 5, 11}, blow-up 3, coset", mixed_lde_run(xs, g), [oracle.lde(0, x, MIXED_BLOWUP, g) for x in xs]),
            ("ntt_mixed_batch_dev {11, 3, 10}, coset", ntt, [oracle.ntt(0, y, coset=g) for y in ys])]


def tr_hash_many_case(oracle):
    tags = [b"FRI/index", b"ALI/A", b"alloc/item"]; ks = [33, 17, 1]
    fields = [oracle.synth_column(0x7A65, i, 0, k) for i, k in enumerate(ks)]
    want = np.stack([oracle.tr_hash_fields_tagged(t, f) for t, f in zip(tags, fields)])

    def run(c):
        d = [dev(f) for f in fields]; out = out_rows(3)
        c.sync(); c.tr_hash_many_dev([(t, x.data_ptr(), k) for t, x, k in zip(tags, d, ks)], out.data_ptr()); c.sync()
        return host(out)
    return [("tr_hash_many_dev, three tags", run, want)]


def steered_params_case(oracle):
    """stark_poseidon_params_upload of a steered set (corner_values.steered_set) and one node hashed under it: the digest the construction predicts"""
    base = pyref.params_for_width(17); LEVEL, LABEL = 3, 42
    nd = cv.steered_set(base, cv.target_schedules(base)[0], 1, 5000, LEVEL, LABEL)
    arrays = cv.params_arrays(nd["params"]); kids = nd["children"]; want = nd["digest"].reshape(1, 4)

    def run(c):
        p = c.params_upload(*arrays)
        try:
            return c.hash_ds_level(p, 16, LEVEL, nd["pos"], LABEL, kids)
        finally:
            p.free()
    return [("poseidon_params_upload of a steered set + one node", run, want)]


def open_batch_case(oracle):
    """stark_merkle_open_batch over two trees of different shapes"""
    shapes = [(16, 257), (4, 64)]; label = 0x5EED
    leaves = [mc.leaves_of(oracle, pp.SEED, b, n) for b, (_, n) in enumerate(shapes)]; ixs = [mc.index_lists(n, b) for b, (_, n) in enumerate(shapes)]
    want = []
    for (arity, n), f, ix in zip(shapes, leaves, ixs):
        o = oracle.merkle_build(arity, label, f); want.append(o.open_bytes(ix)); o.free()

    def run(c):
        trees = []
        try:
            for (arity, n), f in zip(shapes, leaves):
                trees.append(c.merkle_new(f, c.merkle_cfg(arity, label)))
            return c.merkle_open_batch(trees, ixs)
        finally:
            for t in trees:
                t.free()
    return [("merkle_open_batch, two shapes", run, want)]


def sharded_emulated_cases(oracle):
    """the two emulated sharded calls at their guard-band shapes (tests/test_gpu_guard_bands.py): W = 2 at 2^10, [16, 8], r = 8"""
    if "sharded" in _memo:
        return _memo["sharded"]
    W, n0, sched, r = 2, 1 << 10, [16, 8], 8
    cols = oracle.rand_fr_columns(0x5BA2, n0, 4); f0 = oracle.build_f0(*cols, n0)[0]
    ref = oracle.deep_fri_prove(*cols, n0, sched, r, SEED_Z)
    roots = np.stack([ref.root(l) for l in range(len(sched) + 1)]); proof = (ref.bytes(), ref.size_estimate()); ref.free()

    def build(c):
        d = dev(f0)
        return c.diag_fri_build_sharded_emulated(W, d.data_ptr(), n0, sched, SEED_Z)

    def prove(c):
        d = [dev(x) for x in cols]
        return [p[:2] for p in c.diag_deep_fri_prove_sharded_emulated(W, *[t.data_ptr() for t in d], n0, DeepFriParams(sched, r, SEED_Z))]
    _memo["sharded"] = [("diag_fri_build_sharded_emulated, W = 2", build, np.stack([roots] * W)), ("diag_deep_fri_prove_sharded_emulated, W = 2", prove, [proof] * W)]
    return _memo["sharded"]


def big_ntt_case(oracle):
    """ONE forward coset NTT at 2^21 on Pallas: the three-pass plan, tw_direct[0] and tw_direct[1], the merged coset tables.  The only large case."""
    x = oracle.synth_column(0xBA7C000 + BIG_LOG, 0, 0, 1 << BIG_LOG); g = oracle.from_u64(5)
    return [("fft 2^21 on a coset", lambda c: c.fft(x, field=PALLAS_FR, coset=g), oracle.ntt(0, x, coset=g))]


# group name -> (builder(oracle) -> cases, the context options they run under).  A group is built when first asked for and kept for the session.
def _three(i):
    return lambda o: _memo.setdefault("three", batched_prove_cases(o))[i:i + 1]


PROVE3_OPT = {"prove_batch_max_rows": 2 << PROVE3["k"]}
BUILDERS = {
    "merkle 16 x 257": (lambda o: [("arity 16, n = 257",) + pp.tree_case(o, 16, 257)], {}),
    "merkle 16 x 4097": (lambda o: [("arity 16, n = 4097",) + pp.tree_case(o, 16, 4097)], {}),
    "merkle 8 x 19": (lambda o: [("arity 8, n = 19",) + pp.tree_case(o, 8, 19)], {}),
    "merkle pairs 16 x 64": (lambda o: [("pairs, arity 16, n = 64",) + pp.tree_case(o, 16, 64, pairs=True)], {}),
    "leaf pairs": (lambda o: [("leaf_pair_hash, n = 4097, m = 16",) + pp.leaf_case(o, 4097, 16)], {}),
    "ntt lg 3, 12": (lambda o: [case for lg in (3, 12) for case in pp.ntt_cases(o, PALLAS_FR, lg)], {}),
    "ntt lg 13": (lambda o: pp.ntt_cases(o, PALLAS_FR, 13), {}),
    "batch transforms": (lambda o: pp.batch_transform_cases(o, 3), {}),
    "deep_fri_verify": (lambda o: pp.deep_fri_verify_cases(o, 1 << 9, [8, 4, 2], 5, 77), {}),
    "fold": (fold_cases, {}),
    "fri_build_transcript": (lambda o: fri_build_case(o, 1 << 9, [8, 4, 2]), {}),
    "deep_fri_prove": (lambda o: prove_case(o, 1 << 10, [16, 8], 8), {}),
    "ali_merge": (ali_merge_cases, {}),
    "batched prove": (_three(0), PROVE3_OPT), "batched prove f0": (_three(1), PROVE3_OPT), "batched commit": (_three(2), PROVE3_OPT),
    "sumcheck prove plain": (lambda o: sumcheck_prove_cases(o, 0, 5), {}),
    "sumcheck prove mf, single": (lambda o: sumcheck_prove_cases(o, 1, 5)[:1], {}),
    "sumcheck prove mf, batch": (lambda o: sumcheck_prove_cases(o, 1, 5)[1:], {}),
    "sumcheck verify": (lambda o: sumcheck_verify_cases(o, 0)[:1] + sumcheck_verify_cases(o, 1)[1:], {}),
    "merkle verify": (merkle_verify_cases, {}),
    "mle": (lambda o: mle_cases(o, 7), {"mle_log_tile": 3}),
    "lagrange": (lagrange_cases, {}),
    "mixed merkle": (mixed_merkle_cases, {}),
    "mixed prove": (lambda o: mixed_prove_case(o, False), {}),
    "mixed transforms": (mixed_transform_cases, {}),
    "tr_hash_many": (tr_hash_many_case, {}),
    "steered params": (steered_params_case, {}),
    "open batch": (open_batch_case, {}),
    "sharded emulated commit": (lambda o: sharded_emulated_cases(o)[:1], {}),
    "sharded emulated prove": (lambda o: sharded_emulated_cases(o)[1:], {}),
    "ntt 2^21": (big_ntt_case, {}),
}
GROUPS = list(BUILDERS)
# The whole PROVE_ORDER, the [128] trace included: swept warm and in the retry modes on the SESSION's context, which derives the t = 129 constants
# once for every test of the session that needs them (the cold sweep, a context per request, runs "mixed prove", the same batch without that trace)
BUILDERS["mixed prove, all shapes"] = (lambda o: mixed_prove_case(o, True), {})
SESSION_GROUPS = ["mixed prove, all shapes"]


def group(oracle, name):
    """-> (cases, options) of the group, built once"""
    if name not in _memo:
        _memo[name] = BUILDERS[name][0](oracle)
    return _memo[name], BUILDERS[name][1]
