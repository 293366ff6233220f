"""Queued calls: the harness and the cases of test_gpu_queued_calls.py (device) and test_queued_cases_host.py (CPU).

include/stark_mlwe.h promises that every `*_dev` entry point is stream-ordered on the context's stream and that some of them return without a host
synchronisation, their host arrays "copied before the call returns" (PROMISED below).  A pipeline here issues such calls back to back behind a
Blocker — one long serial sponge that keeps the stream busy while the host enqueues — and destroys every host argument (clobber) the moment each
call returns.  Every pipeline runs three times: (a) each call bracketed by a synchronisation (also the warm-up: tag frames, NTT plans, parameter sets,
pool blocks), (b) queued behind the blocker with ONE download of all outputs at the end, (c) on the CPU oracle; three_way asserts (a) == (c) and
(b) == (c) byte for byte and names the first differing call and row.  A queued run is only evidence while the stream was still busy, so the blocker's
event must be incomplete after the last call of the section: Run.end records it and require_busy asserts it, naming the first promised call after
which the stream had drained.  No time is asserted anywhere; RECORDS keeps what was measured (profiles/queued_calls.jsonl)."""
import contextlib
import ctypes as C
import time

import numpy as np

import lagrange_cases as lc
from test_gpu_guard_bands import SENTINEL, Band, hp, level_reference

vp = C.c_void_p
N8, N11 = 1 << 8, 1 << 11
COSET = 5                                  # the generator of Pallas Fr: a non-unit coset
SEED_Z = 0xDEEFBAAD
FRI_SCHEDULE = [8, 4, 2]                   # test_gpu_guard_bands.PROVE's schedule: 64 divides 2^11
TAGS = (b"FRI/index", b"ALI/A", b"queued/item")
BLOCKER_TAG = b"queued/blocker"
# K fields of the blocker's sponge.  Measured warm on an MI355X (profiles/queued_calls.jsonl): the longest queued section, Q3's 300 calls, takes
# 8.0 ms of host time on the torch-stream context (7.3 ms on the default stream; every other section 0.15 - 0.31 ms); the blocker at K = 2^16 runs
# 295.1 - 298.9 ms on the device (4.5 us per field), 37 times the longest section where 10 times was asked for (K = 2^15, 149 ms, would leave
# 18 times; 2^17 ran 595 ms and made the first test of a session take 6 s).  The tests assert the condition itself, never these numbers.
BLOCKER_K = 1 << 16
Q3_CALLS, Q3_KS = 300, (0, 1, 17, 33)
PROMISED = ("stark_tr_hash_many_dev", "stark_merkle_build_batch_dev", "stark_commitment_commit_batch_dev", "stark_lagrange_eval_on_h_dev",
            "stark_lagrange_eval_on_h_batch_dev", "stark_mle_evaluate_dev", "stark_mle_evaluate_batch_dev", "stark_ntt_batch_dev", "stark_lde_batch_dev",
            "stark_ntt_dev", "stark_lde_dev", "stark_merkle_free")
RECORDS = []                               # one dict per queued run: pipeline, context, K, enqueue_ms, blocker_ms, busy_at_end, returns_while_busy
_cache = {}


# ---- the harness ------------------------------------------------------------------------------------------------------------------------------
def clobber(*args):
    """destroy host arguments in place: numpy arrays and ctypes value tables become 0xFF bytes, pointer tables 0, string buffers b"?" """
    for a in args:
        if a is None:
            continue
        if isinstance(a, np.ndarray):
            assert a.flags.c_contiguous and a.flags.writeable
            a.reshape(-1).view(np.uint8)[:] = 0xFF
        elif isinstance(a, C.Array) and a._type_ is C.c_char:
            C.memset(a, 0, C.sizeof(a)); a[0:1] = b"?"
        elif isinstance(a, C.Array) and a._type_ in (C.c_void_p, C.c_char_p):
            C.memset(a, 0, C.sizeof(a))
        elif isinstance(a, C.Array):
            C.memset(a, 0xFF, C.sizeof(a))
        else:
            raise TypeError("clobber: %r is neither a numpy array nor a ctypes table" % type(a))


def table(ptrs):
    """a host table of device pointers (ints, c_void_p or None)"""
    vals = [p.value if isinstance(p, vp) else p for p in ptrs]
    return (vp * max(len(vals), 1))(*[int(v) if v else None for v in vals])


def rows(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def first_difference(got, want):
    """got, want: lists of (call, rows) in issue order -> None, or (call, row) of the first difference (row None: another shape or call)"""
    if [c for c, _ in got] != [c for c, _ in want]:
        return ("the list of calls", None)
    for (call, g), (_, w) in zip(got, want):
        g, w = rows(g), rows(w)
        if g.shape != w.shape:
            return (call, None)
        bad = np.nonzero((g != w).any(axis=1))[0]
        if bad.size:
            return (call, int(bad[0]))
    return None


def three_way(sync, queued, ref, what):
    """(a) == (c) and (b) == (c), byte for byte; the first differing call and row by name"""
    for run, got in (("synchronised", sync), ("queued", queued)):
        d = first_difference(got, ref)
        if d is not None:
            call, row = d
            g = dict(got).get(call); w = dict(ref).get(call)
            n_bad = int((rows(g) != rows(w)).any(axis=1).sum()) if row is not None else -1
            raise AssertionError("%s, the %s run differs from the reference: %s, %s" % (what, run, call, "another shape" if row is None else
                                 "%d of %d rows differ, first at row %d" % (n_bad, rows(w).shape[0], row)))


def blocker_input(oracle, k):
    key = ("blocker", k)
    if key not in _cache:
        f = oracle.synth_column(0xB10C, 0, 0, k)
        _cache[key] = (f, oracle.tr_hash_fields_tagged(BLOCKER_TAG, f))
    return _cache[key]


def dev(a):
    import torch
    return torch.from_numpy(rows(a).view(np.int64).copy()).cuda()


class Blocker:
    """One serial sponge of k fields (one item of stark_tr_hash_many_dev under a warm tag: the five-wave kernel, one workgroup, one dependent
    permutation after another) and an event recorded behind it on the same stream.  still_busy() is `not event.query()`; check() compares the digest
    with the oracle's, so the blocker is itself a queued call whose tables were clobbered."""

    def __init__(self, ctx, oracle, k=BLOCKER_K):
        self.ctx, self.oracle, self.k = ctx, oracle, k
        self.event = self.t0 = self.out = None

    def start(self):
        import torch
        fields, self.want = blocker_input(self.oracle, self.k)
        key = ("blocker dev", self.k)
        if key not in _cache:
            _cache[key] = dev(fields); torch.cuda.synchronize()
        self.fields = _cache[key]
        self.out = torch.full((1, 4), SENTINEL, dtype=torch.int64, device="cuda")
        tag = C.create_string_buffer(BLOCKER_TAG); tags = table([C.addressof(tag)]); flds = table([self.fields.data_ptr()]); ks = (C.c_size_t * 1)(self.k)
        self.t0, self.event = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.t0.record()
        rc = self.ctx.lib.stark_tr_hash_many_dev(self.ctx.h, 1, tags, flds, ks, vp(self.out.data_ptr()))
        self.event.record()
        self.host_t0 = time.perf_counter()
        clobber(tag, tags, flds, ks)
        self.ctx._chk(rc)
        return self

    def still_busy(self):
        return not self.event.query()

    def ms(self):
        """device time of the sponge (after a synchronisation)"""
        return self.t0.elapsed_time(self.event)

    def check(self):
        got = self.out.cpu().numpy().view(np.uint64)
        assert (got[0] == self.want).all(), "the blocker's own digest (k = %d) differs from the oracle's" % self.k


class Run:
    """One run of a pipeline on `ctx`: mode "sync" brackets every call with ctx.sync(); mode "queued" starts a Blocker in begin() and notes after
    every call whether it returned while the blocker still ran.  call() clobbers the host arguments the moment the entry point has returned."""

    def __init__(self, ctx, oracle, mode, k=BLOCKER_K):
        assert mode in ("sync", "queued")
        self.ctx, self.oracle, self.mode, self.k = ctx, oracle, mode, k
        self.blocker, self.table, self.waited, self.busy_at_end, self.enqueue_ms, self.ncalls = None, {}, None, None, None, 0

    def begin(self):
        if self.mode == "sync":                                            # the blocker's tag frame is made here, so that the queued run finds it
            b = Blocker(self.ctx, self.oracle, 16).start(); self.ctx.sync(); b.check()
        else:
            self.blocker = Blocker(self.ctx, self.oracle, self.k).start()
        self.t0 = time.perf_counter()

    def call(self, name, fn, *host):
        if self.mode == "sync":
            self.ctx.sync()
        rc = fn()
        busy = self.blocker.still_busy() if self.blocker else None
        clobber(*host)
        self.ctx._chk(rc)
        self.ncalls += 1
        if self.mode == "sync":
            self.ctx.sync()
        else:
            self.table[name] = self.table.get(name, True) and busy
            if not busy and self.waited is None and name in PROMISED:
                self.waited = (name, self.ncalls, 1e3 * (time.perf_counter() - self.t0))

    def end(self):
        self.enqueue_ms = 1e3 * (time.perf_counter() - self.t0)
        if self.blocker:
            self.busy_at_end = self.blocker.still_busy()

    def require_busy(self, what):
        """the condition of a queued run: the blocker's event was incomplete after the last call of the section"""
        if self.mode != "queued":
            return
        assert self.waited is None, ("%s: %s (call %d of the section) returned only after the stream had drained, %.2f ms into a section behind a blocker "
                                     "of %.1f ms: it waited for the stream" % ((what,) + self.waited + (self.blocker.ms(),)))
        assert self.busy_at_end, "%s: the blocker (%.1f ms) had finished before the last queued call returned (%.2f ms of enqueueing)" % (what, self.blocker.ms(), self.enqueue_ms)

    def record(self, pipeline, context):
        if self.mode == "queued":
            RECORDS.append(dict(pipeline=pipeline, context=context, K=self.k, calls=self.ncalls, enqueue_ms=round(self.enqueue_ms, 3), blocker_ms=round(self.blocker.ms(), 3),
                                busy_at_end=bool(self.busy_at_end), first_promised_call_that_waited=self.waited[0] if self.waited else None,
                                returns_while_busy={k: bool(v) for k, v in self.table.items()}))


def finish(run, out, inputs, what, strict):
    """the end of a pipeline: ONE download of every output, then the guard bands, the inputs and the blocker's digest; -> the host image of `out`"""
    run.end()
    host = out.host()
    run.ctx.sync()
    if run.blocker:
        run.blocker.check()
        if strict:
            run.require_busy(what)
    out.check(what, host)
    for b in inputs:
        b.check_unchanged(what)
    return host


def hash_many(run, items, out_ptr):
    """stark_tr_hash_many_dev over items (tag, device pointer or None, k) into out_ptr; every table is the test's own and is clobbered on return"""
    n = len(items); bufs = [C.create_string_buffer(t) for t, _, _ in items]
    tags = table([C.addressof(b) for b in bufs]); flds = table([p for _, p, _ in items]); ks = (C.c_size_t * n)(*[k for _, _, k in items])
    lib, h = run.ctx.lib, run.ctx.h
    run.call("stark_tr_hash_many_dev", lambda: lib.stark_tr_hash_many_dev(h, n, tags, flds, ks, vp(out_ptr)), tags, flds, ks, *bufs)


def root_ptr(lib, tree):
    return lib.stark_merkle_level_dev(tree, lib.stark_merkle_num_levels(tree) - 1)


def free_trees(run, trees):
    lib = run.ctx.lib
    while trees:
        t = trees.pop()
        run.call("stark_merkle_free", lambda: lib.stark_merkle_free(t))


# ---- the references (CPU only, built once) ----------------------------------------------------------------------------------------------------
def F(oracle, x):
    return oracle.from_u64(x)


def digest(oracle, tag, fields):
    return oracle.tr_hash_fields_tagged(tag, rows(fields) if len(fields) else np.zeros((0, 4), np.uint64))


def tree_root(oracle, arity, label, leaves, commit=False):
    if commit:
        return oracle.commitment_root(label, leaves)
    t = oracle.merkle_build(arity, label, leaves)
    try:
        return t.root()
    finally:
        t.free()


Q1_LABELS, Q1_LABELS2 = (7, 8, 9), (17, 18, 19)


def q1_inputs(oracle):
    if "q1 in" not in _cache:
        cols = oracle.rand_fr_columns(0x51A1, N8, 3); coset = F(oracle, COSET)
        _cache["q1 in"] = dict(cols=cols, coset=coset, lde=[oracle.lde(0, c, 3, coset) for c in cols], other=oracle.rand_fr_columns(0x51A2, N11, 3))
    return _cache["q1 in"]


def q1_items(roots, lde0):
    """step 3: (tag, fields, k) of the five items — the three roots in place, an empty item, the first 200 elements of LDE output 0"""
    return [(TAGS[i], roots[i].reshape(1, 4), 1) for i in range(3)] + [(TAGS[0], lde0[:0], 0), (TAGS[1], lde0[:200], 200)]


def q1_refs(oracle, commit):
    key = ("q1", commit)
    if key not in _cache:
        I = q1_inputs(oracle)
        r1 = [tree_root(oracle, 16, l, v, commit) for l, v in zip(Q1_LABELS, I["lde"])]
        r2 = [tree_root(oracle, 16, l, v, commit) for l, v in zip(Q1_LABELS2, I["other"])]
        _cache[key] = dict(roots=r1, roots2=r2, results=[("stark_lde_batch_dev, output %d" % i, I["lde"][i]) for i in range(3)] + [
            ("stark_tr_hash_many_dev over the first trees", np.stack([digest(oracle, t, f) for t, f, _ in q1_items(r1, I["lde"][0])])),
            ("stark_tr_hash_many_dev over the rebuilt trees", np.stack([digest(oracle, TAGS[i], r2[i].reshape(1, 4)) for i in range(3)]))])
    return _cache[key]


def q2_inputs(oracle):
    if "q2 in" not in _cache:
        cols = q1_inputs(oracle)["lde"]
        outside = lc.points(oracle, N11, 2); inside, j = lc.inside_points(oracle, N11)[2]
        _cache["q2 in"] = dict(cols=cols, zs=np.ascontiguousarray(np.stack([outside[0], inside, outside[1]])), inside=(1, j),
                               r=oracle.synth_column(0x51B1, 0, 0, 3 * 11).reshape(3, 11, 4), coset=F(oracle, COSET))
    return _cache["q2 in"]


def q2_refs(oracle):
    if "q2" not in _cache:
        I = q2_inputs(oracle); cols, zs, r, g = I["cols"], I["zs"], I["r"], I["coset"]
        lag = lc.r2(oracle, cols, zs)
        _cache["q2"] = [("stark_lagrange_eval_on_h_batch_dev", lag.reshape(-1, 4)), ("stark_lagrange_eval_on_h_dev", lag[2, 1].reshape(1, 4)),
                        ("stark_mle_evaluate_batch_dev", np.stack([oracle.mle_evaluate(cols[i], r[i]) for i in range(3)])),
                        ("stark_mle_evaluate_dev", oracle.mle_evaluate(cols[2], r[0]).reshape(1, 4))] + [
                        ("stark_ntt_batch_dev inverse, then forward on the coset, column %d" % i, oracle.ntt(0, oracle.ntt(0, cols[i], inverse=True), coset=g)) for i in range(3)] + [
                        ("stark_ntt_dev", oracle.ntt(0, cols[0], inverse=True, coset=g)), ("stark_lde_dev", oracle.lde(0, cols[1], 1, g))]
    return _cache["q2"]


def q3_pool(oracle):
    if "q3 pool" not in _cache:
        _cache["q3 pool"] = oracle.synth_column(0x51C1, 0, 0, 64)
    return _cache["q3 pool"]


def q3_items(j):
    """the two items of call j as (tag, offset into the pool, k): k cycles over Q3_KS, the tag over TAGS, the offset over 0..30"""
    return [(TAGS[(j + i) % 3], (7 * j + 3 * i) % 31, Q3_KS[(j + i) % 4]) for i in (0, 1)]


def q3_refs(oracle):
    if "q3" not in _cache:
        pool = q3_pool(oracle); memo = {}

        def d(item):
            if item not in memo:
                tag, off, k = item
                memo[item] = digest(oracle, tag, pool[off:off + k])
            return memo[item]
        _cache["q3"] = [("stark_tr_hash_many_dev, 300 calls of two items", np.stack([d(it) for j in range(Q3_CALLS) for it in q3_items(j)]))]
    return _cache["q3"]


Q4_LABELS = (21, 22)


def q4_inputs(oracle):
    if "q4 in" not in _cache:
        cols = oracle.rand_fr_columns(0x51D1, N8, 4); coset = F(oracle, COSET)
        _cache["q4 in"] = dict(cols=cols, coset=coset, omega=oracle.domain_omega(N11), z=F(oracle, 0xC0FFEE), zfold=oracle.fri_sample_z_ell(SEED_Z, 0, N11))
    return _cache["q4 in"]


def q4_refs(oracle):
    if "q4" not in _cache:
        I = q4_inputs(oracle)
        lde = [oracle.lde(0, c, 3, I["coset"]) for c in I["cols"]]
        f0 = oracle.ali_merge(*lde, I["omega"], I["z"], want_c_star=False)[0]
        p = oracle.deep_fri_prove(None, None, None, None, N11, FRI_SCHEDULE, 1, SEED_Z, f0=f0)
        try:
            fri_roots = np.stack([p.root(l) for l in range(len(FRI_SCHEDULE) + 1)])
        finally:
            p.free()
        fold = oracle.fri_fold_layer(lde[0], I["zfold"], 8)
        leaf = oracle.leaf_pair_hash(lde[1], fold, 8)
        level = level_reference(oracle, 16, 3, 32, 42, leaf)
        _cache["q4"] = [("stark_lde_batch_dev, output %d" % i, lde[i]) for i in range(4)] + [
            ("stark_ali_merge_dev", f0), ("stark_fri_build_dev, the roots", fri_roots),
            ("stark_merkle_build_batch_dev, the roots", np.stack([tree_root(oracle, 8, l, v[:128]) for l, v in zip(Q4_LABELS, lde)])),
            ("stark_fri_fold_dev", fold), ("stark_leaf_pair_hash_dev", leaf), ("stark_poseidon_hash_ds_batch_dev", level),
            ("stark_tr_hash_fields_tagged_dev", np.stack([digest(oracle, TAGS[0], level[16 * i:16 * i + 16]) for i in range(8)]))]
    return _cache["q4"]


# ---- the pipelines (device) -------------------------------------------------------------------------------------------------------------------
def results_of(out, host, ref):
    return [(call, out.payload(i, host)) for i, (call, _) in enumerate(ref)]


def q1(run, commit=False, strict=True):
    """extend, commit, hash the roots, free, rebuild into the same blocks"""
    ctx, oracle = run.ctx, run.oracle; lib, h = ctx.lib, ctx.h
    I, R = q1_inputs(oracle), q1_refs(oracle, commit)
    what = "Q1 (%s), %s run" % ("stark_commitment_commit_batch_dev" if commit else "stark_merkle_build_batch_dev", run.mode)
    inb, other = Band(list(I["cols"])), Band(list(I["other"])); out = Band([N11, N11, N11, 5, 3])
    p = None if commit else ctx.poseidon_params_for_arity(16)
    live = []

    def build(ptrs, labels):
        lab = np.array(labels, np.uint64); tab = table(ptrs); outh = (vp * 3)()
        if commit:
            run.call("stark_commitment_commit_batch_dev", lambda: lib.stark_commitment_commit_batch_dev(h, 3, hp(lab), tab, N11, outh), lab, tab)
        else:
            run.call("stark_merkle_build_batch_dev", lambda: lib.stark_merkle_build_batch_dev(h, p.h, 16, 3, hp(lab), tab, N11, 0, None, outh), lab, tab)
        live.extend(vp(outh[i]) for i in range(3))
        return [root_ptr(lib, t) for t in live[-3:]]

    ctx.sync()
    try:
        run.begin()
        ev, ot, coset = table([inb.ptr(i) for i in range(3)]), table([out.ptr(i) for i in range(3)]), np.array(I["coset"])
        run.call("stark_lde_batch_dev", lambda: lib.stark_lde_batch_dev(h, 0, 3, ev, 8, 3, hp(coset), ot), ev, ot, coset)
        roots = build([out.ptr(i) for i in range(3)], Q1_LABELS)
        hash_many(run, [(TAGS[0], roots[0], 1), (TAGS[1], roots[1], 1), (TAGS[2], roots[2], 1), (TAGS[0], None, 0), (TAGS[1], out.ptr(0).value, 200)], out.ptr(3).value)
        free_trees(run, live)                                              # all three at once: the hash of their roots is still queued
        cached_first = lib.stark_ctx_cached_bytes(h)
        roots = build([other.ptr(i) for i in range(3)], Q1_LABELS2)        # takes the level blocks released above
        hash_many(run, [(TAGS[i], roots[i], 1) for i in range(3)], out.ptr(4).value)
        free_trees(run, live)
        cached_second = lib.stark_ctx_cached_bytes(h)
        host = finish(run, out, [inb, other], what, strict)
    finally:
        ctx.sync()
        while live:
            lib.stark_merkle_free(live.pop())
    assert cached_first == cached_second, "%s: the pool grew between the two batches (%d -> %d cached bytes): the rebuild did not take the released level blocks" % (what, cached_first, cached_second)
    return results_of(out, host, R["results"])


def q2(run, strict=True):
    """open and evaluate: every call queued on the three 2^11 columns"""
    ctx, oracle = run.ctx, run.oracle; lib, h = ctx.lib, ctx.h
    I, R = q2_inputs(oracle), q2_refs(oracle)
    what = "Q2, %s run" % run.mode
    cols = Band(list(I["cols"]))
    out = Band([9, 1, 3, 1, I["cols"][0], I["cols"][1], I["cols"][2], I["cols"][0], 2 * N11])
    c = [cols.ptr(i).value for i in range(3)]
    ctx.sync()
    run.begin()
    t, zs = table(c), np.array(I["zs"])
    run.call("stark_lagrange_eval_on_h_batch_dev", lambda: lib.stark_lagrange_eval_on_h_batch_dev(h, 3, t, N11, None, 3, hp(zs), out.ptr(0)), t, zs)
    z = np.array(I["zs"][2])
    run.call("stark_lagrange_eval_on_h_dev", lambda: lib.stark_lagrange_eval_on_h_dev(h, vp(c[1]), N11, hp(z), None, out.ptr(1)), z)
    t2, r = table(c), np.array(I["r"])
    run.call("stark_mle_evaluate_batch_dev", lambda: lib.stark_mle_evaluate_batch_dev(h, 3, t2, 11, hp(r), out.ptr(2)), t2, r)
    r0 = np.array(I["r"][0])
    run.call("stark_mle_evaluate_dev", lambda: lib.stark_mle_evaluate_dev(h, vp(c[2]), 11, hp(r0), out.ptr(3)), r0)
    t3 = table([out.ptr(i) for i in (4, 5, 6)])
    run.call("stark_ntt_batch_dev", lambda: lib.stark_ntt_batch_dev(h, 0, 3, t3, 11, 1, None), t3)
    t4, g = table([out.ptr(i) for i in (4, 5, 6)]), np.array(I["coset"])
    run.call("stark_ntt_batch_dev", lambda: lib.stark_ntt_batch_dev(h, 0, 3, t4, 11, 0, hp(g)), t4, g)
    g2 = np.array(I["coset"])
    run.call("stark_ntt_dev", lambda: lib.stark_ntt_dev(h, 0, out.ptr(7), 11, 1, hp(g2)), g2)
    g3 = np.array(I["coset"])
    run.call("stark_lde_dev", lambda: lib.stark_lde_dev(h, 0, vp(c[1]), 11, 1, hp(g3), out.ptr(8)), g3)
    host = finish(run, out, [cols], what, strict)
    return results_of(out, host, R)


def q3(run, strict=True):
    """many staged uploads in flight: 300 calls of two items each behind one blocker, distinct output slots"""
    ctx, oracle = run.ctx, run.oracle
    what = "Q3, %s run" % run.mode
    pool = Band([q3_pool(oracle)]); out = Band([2 * Q3_CALLS])
    base, o = pool.ptr(0).value, out.ptr(0).value
    ctx.sync()
    run.begin()
    for j in range(Q3_CALLS):
        hash_many(run, [(tag, base + 32 * off if k else None, k) for tag, off, k in q3_items(j)], o + 64 * j)
    host = finish(run, out, [pool], what, strict)
    return results_of(out, host, q3_refs(oracle))


def q4(run):
    """calls that are only stream-ordered consume queued producers; nothing about their return is asserted, Run.table records it"""
    ctx, oracle = run.ctx, run.oracle; lib, h = ctx.lib, ctx.h
    I, R = q4_inputs(oracle), q4_refs(oracle)
    what = "Q4, %s run" % run.mode
    L = len(FRI_SCHEDULE)
    inb = Band(list(I["cols"])); out = Band([N11] * 5 + [L + 1, 2, N11 // 8, N11, N11 // 16, 8])
    tp, p16, p8 = ctx.transcript_params(), ctx.poseidon_params_for_arity(16), ctx.poseidon_params_for_arity(8)
    state, live = vp(), []

    def copy_row(src, dst):                                                # dst[0] = src[0] on the stream: a root leaves its handle without a download
        run.call("stark_interleave_dev", lambda: lib.stark_interleave_dev(h, vp(src), vp(dst), 1, 1, 0))

    ctx.sync()
    try:
        run.begin()
        ev, ot, coset = table([inb.ptr(i) for i in range(4)]), table([out.ptr(i) for i in range(4)]), np.array(I["coset"])
        run.call("stark_lde_batch_dev", lambda: lib.stark_lde_batch_dev(h, 0, 4, ev, 8, 3, hp(coset), ot), ev, ot, coset)
        omega, z = np.array(I["omega"]), np.array(I["z"])
        run.call("stark_ali_merge_dev", lambda: lib.stark_ali_merge_dev(h, out.ptr(0), out.ptr(1), out.ptr(2), out.ptr(3), None, None, hp(omega), hp(z), N11, out.ptr(4), None), omega, z)
        sch = np.array(FRI_SCHEDULE, np.uint64)
        run.call("stark_fri_build_dev", lambda: lib.stark_fri_build_dev(h, out.ptr(4), N11, hp(sch), L, SEED_Z, C.byref(state)), sch)   # forks the side stream
        for l in range(L + 1):
            copy_row(root_ptr(lib, lib.stark_fri_layer_tree(state, l)), out.ptr(5).value + 32 * l)
        run.call("stark_fri_state_free", lambda: lib.stark_fri_state_free(state)); state = vp()
        lab, tab, outh = np.array(Q4_LABELS, np.uint64), table([out.ptr(0), out.ptr(1)]), (vp * 2)()      # recycles blocks the side stream touched
        run.call("stark_merkle_build_batch_dev", lambda: lib.stark_merkle_build_batch_dev(h, p8.h, 8, 2, hp(lab), tab, 128, 0, None, outh), lab, tab)
        live.extend(vp(outh[i]) for i in range(2))
        for i in range(2):
            copy_row(root_ptr(lib, live[i]), out.ptr(6).value + 32 * i)
        free_trees(run, live)
        zf = np.array(I["zfold"])
        run.call("stark_fri_fold_dev", lambda: lib.stark_fri_fold_dev(h, out.ptr(0), N11, hp(zf), 8, out.ptr(7)), zf)
        run.call("stark_leaf_pair_hash_dev", lambda: lib.stark_leaf_pair_hash_dev(h, tp.h, out.ptr(1), out.ptr(7), N11, 8, out.ptr(8)))
        run.call("stark_poseidon_hash_ds_batch_dev", lambda: lib.stark_poseidon_hash_ds_batch_dev(h, p16.h, 16, 3, 32, 42, out.ptr(8), N11, out.ptr(9)))
        tag = C.create_string_buffer(TAGS[0])
        run.call("stark_tr_hash_fields_tagged_dev", lambda: lib.stark_tr_hash_fields_tagged_dev(h, None, tag, out.ptr(9), 16, 8, out.ptr(10)), tag)
        host = finish(run, out, [inb], what, strict=False)
    finally:
        ctx.sync()
        if state:
            lib.stark_fri_state_free(state)
        while live:
            lib.stark_merkle_free(live.pop())
    return results_of(out, host, R)


def three_runs(ctx, oracle, pipeline, ref, what, context, **kw):
    """(a) synchronised, (b) queued, against (c) the reference; the queued run's measurements go to RECORDS"""
    a = pipeline(Run(ctx, oracle, "sync"), **kw)
    run = Run(ctx, oracle, "queued")
    try:
        b = pipeline(run, **kw)
    finally:
        if run.blocker and run.enqueue_ms is not None:
            ctx.sync(); run.record(what, context)
    three_way(a, b, ref, what)
    return run


@contextlib.contextmanager
def on_stream(stream):
    """torch's current stream for the length of the block (None: the default stream stays current)"""
    if stream is None:
        yield
    else:
        import torch
        with torch.cuda.stream(stream):
            yield


def measure(path):
    """`python tests/queued_cases.py [out.jsonl]` on an MI355X: every pipeline on both contexts with the busy condition recorded instead of asserted
    (the results are still compared); one line per queued run — enqueue time, blocker time, K, returns-while-busy — as in profiles/queued_calls.jsonl"""
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import oracle_lib
    from stark_mlwe_amd.api import Context
    oracle = oracle_lib.Oracle(); s = torch.cuda.Stream()
    small = dict(mle_log_tile=(4, -1), lagrange_max_partials=(1, -1), ntt_batch_max_elems=(N11, 1 << 24))
    for name, ctx, stream in (("default stream", Context(0), None), ("torch stream", Context(0, C.c_void_p(s.cuda_stream)), s)):
        jobs = [("Q1, stark_merkle_build_batch_dev", q1, q1_refs(oracle, False)["results"], dict(commit=False, strict=False), {}),
                ("Q1, stark_commitment_commit_batch_dev", q1, q1_refs(oracle, True)["results"], dict(commit=True, strict=False), {}),
                ("Q2, default options", q2, q2_refs(oracle), dict(strict=False), {}), ("Q2, small passes", q2, q2_refs(oracle), dict(strict=False), small),
                ("Q3", q3, q3_refs(oracle), dict(strict=False), {})] + ([("Q4", q4, q4_refs(oracle), {}, {})] if stream is None else [])
        try:
            for what, pipeline, ref, kw, opts in jobs:
                torch.cuda.synchronize()
                try:
                    for k, (v, _) in opts.items():
                        ctx.set_option(k, v)
                    with on_stream(stream):
                        three_runs(ctx, oracle, pipeline, ref, what, name, **kw)
                finally:
                    for k, (_, v) in opts.items():
                        ctx.set_option(k, v)
                print(json.dumps(RECORDS[-1]), flush=True)
        finally:
            ctx.close()
    with open(path, "w") as f:
        for r in RECORDS:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    import sys
    measure(sys.argv[1] if len(sys.argv) > 1 else "queued_calls.jsonl")
