"""Refused allocations on the device: every call fails cleanly or degrades byte-equal.  stark_diag_alloc_refusal (TESTS ONLY) makes the N-th
allocation request of the library — every request for a pooled block, every long-lived table — fail as out of memory, once.  For every case group
of tests/alloc_refusal_cases.py:

  cold sweep   N = 1, 2, ...: a fresh context, arm N, run; stop at the first N whose statistics say nothing was refused.  The requests that build
               plans, tag frames, parameter blobs and power tables are among them.
  warm sweep   one context, one unarmed run, then the same sweep without recreating anything: pooled temporaries, pointer tables, scratch growth.
  retry modes  mode 2 refuses only the first hipMalloc attempt of the m-th request the pool cannot serve: the pool gives its cached blocks back,
               tries again, and the call succeeds.  Mode 3 refuses the second attempt too: the last branch of a real failure, the call failing
               behind an emptied cache.  (A mode-1 refusal of a pooled request skips the give-back, so that it can sit behind a busy stream.)

A refusal that fired ends in exactly one of two ways.  (a) The call reports STARK_ERR_OOM (-4, never -2), every handle it returns through is NULL
and stark_last_error names the allocation; then, on the same context, stark_ctx_sync succeeds, an unarmed repeat equals the ORACLE byte for byte,
the live pooled blocks are those of before the call, and stark_ctx_trim brings the cached bytes to 0.  (b) The call succeeds and equals the oracle:
allowed only at the optional NTT tables, which leave a note where stark_last_error reads (capi_ntt.hip optional_table_note); DEGRADES lists, per
group, exactly the sites that may do so, and the sweep must meet each of them.  After a degraded success the group runs again (the plan stays
degraded), then under another coset and back (the tables are rebuilt).  A sweep that stops early hides sites: a cold sweep must fire at least as
many refusals as an unarmed cold run counts requests.

A real out-of-memory condition is never produced: hipMalloc's own failure is exercised only through the hook.  The shared drivers run the same
sweep on the CPU (tests/test_alloc_refusal_host.py; under sanitizers: tools/alloc_refusal_sanitize.sh).  Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import alloc_refusal_cases as ac
import merkle_batch_cases as mc
import queued_cases as qc
import test_gpu_pool_poison as pp

pytestmark = pytest.mark.gpu

from stark_mlwe_amd.api import PALLAS_FR, Context, DeepFriParams, StarkError

OOM = -4
vp = C.c_void_p
equal, own_context, dev, host = pp.equal, pp.own_context, pp.dev, pp.host
NOTE = "optional NTT table "
# The optional sites a sweep of the group meets (cold or warm): get_plan's tw_direct[i] for plans of two passes and of three (2^21), and build_coset's
# tables for forward transforms on a coset: small + tw_direct (the merged form: plans that have tw_direct[0]), direct (one-pass plans).  Groups that
# are not listed have none: a success after a refusal there is a swallowed failure.
PLAN2, MERGED, DIRECT = {"plan.tw_direct[0]"}, {"coset.small", "coset.tw_direct"}, {"coset.direct"}
# One request is refused per run, so coset.direct can be the refused one only where it is the FIRST choice: a forward coset transform on a one-pass
# plan (2^3 here).  Where the merged form comes first, a refusal of small or tw_direct is what makes build_coset ask for `direct`, and gets it: the
# state "direct without merged tables beside a plan that has tw_direct[0]" is reached through coset.small and coset.tw_direct.
DEGRADES = {
    "ntt lg 3, 12": PLAN2 | MERGED | DIRECT,                 # lg 12: two passes; lg 3: one pass, the coset's direct table
    "ntt lg 13": PLAN2 | MERGED,
    "batch transforms": PLAN2 | MERGED,                      # lg 12 on a coset; the LDEs on a coset at 2^11 outputs; lg 8 has no coset
    "mixed transforms": PLAN2 | MERGED | DIRECT,             # outputs of 2^11, 2^8, 2^14; NTTs of 2^11, 2^3 (one pass), 2^10
    "ntt 2^21": PLAN2 | {"plan.tw_direct[1]"} | MERGED,
}
ALT_LOGS = {"ntt lg 3, 12": [3, 12], "ntt lg 13": [13], "batch transforms": [12, 8, 11], "mixed transforms": [11, 8, 14, 3, 10], "ntt 2^21": [21]}
HANDLE_OUT = {"stark_commitment_commit", "stark_commitment_commit_batch_dev", "stark_commitment_commit_mixed_batch_dev", "stark_deep_fri_prove", "stark_deep_fri_prove_batch_dev",
              "stark_deep_fri_prove_f0_batch_dev", "stark_deep_fri_prove_mixed_batch_dev", "stark_fri_build", "stark_merkle_build", "stark_merkle_build_batch_dev",
              "stark_merkle_build_mixed_batch_dev", "stark_merkle_open_batch", "stark_poseidon_params_for_width", "stark_poseidon_params_t17_seed", "stark_poseidon_params_upload",
              "stark_sumcheck_prove_mf", "stark_sumcheck_prove_mf_batch_dev", "stark_sumcheck_prove_mf_mixed_batch_dev", "stark_sumcheck_prove_plain",
              "stark_sumcheck_prove_plain_batch_dev", "stark_sumcheck_prove_plain_mixed_batch_dev", "stark_diag_deep_fri_prove_sharded_emulated_dev"}
RECORDS = []                                                 # per group: the request counts the sweeps saw (a record, not an assertion)


class Spy:
    """stands in for a context's library handle: every call goes through, and a call that returns STARK_ERR_OOM is kept with its arguments"""

    def __init__(self, lib):
        self._lib, self.oom = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)

        def call(*a):
            rc = f(*a)
            if rc == OOM:
                self.oom.append((name, a))
            return rc
        return call


def handles_are_null(name, args):
    last = args[-1]
    if isinstance(last, C.Array):
        return all(not x for x in last)
    return not last._obj.value                                 # C.byref(handle)


@pytest.fixture(scope="module", autouse=True)
def write_records():
    yield
    path = os.environ.get("STARK_ALLOC_REFUSAL_RECORDS")
    if path and RECORDS:
        with open(path, "a") as f:
            for r in RECORDS:
                f.write(json.dumps(r) + "\n")


def run_all(c, cases):
    return [run(c) for _, run, _ in cases]


def check(got, cases, what):
    for (name, _, want), g in zip(cases, got):
        assert equal(g, want), "%s: %s differs from the oracle" % (what, name)
    assert len(got) == len(cases)


def stale_error(c):
    """puts a known text where stark_last_error reads, so that a note or a message found after a call is that call's"""
    assert c.lib.stark_ctx_set_option(c.h, b"no_such_option", 0) == -1


def last_error(c):
    return (c.lib.stark_last_error(c.h) or b"").decode()


def armed_run(c, cases, mode, n):
    """-> ("oom", message) | ("ok", results), and the statistics of the run; the hook is off afterwards"""
    stale_error(c)
    c.diag_alloc_refusal(mode, n)
    try:
        out = ("ok", run_all(c, cases))
    except StarkError as e:
        out = ("oom", e)
    st = c.diag_alloc_refusal(0)
    return out, st


def alt_coset_cases(oracle, logs):
    """a forward transform on the coset of 7 at each size: the plans of the group rebuild their coset tables"""
    g = oracle.from_u64(7); out = []
    for lg in logs:
        key = ("alt", lg)
        if key not in ac._memo:
            x = oracle.synth_column(0xA17C000 + lg, 0, 0, 1 << lg); ac._memo[key] = (x, oracle.ntt(0, x, coset=g))
        x, want = ac._memo[key]
        out.append(("fft 2^%d on the coset of 7" % lg, (lambda x: lambda c: c.fft(x, field=PALLAS_FR, coset=g))(x), want))
    return out


def after_refusal(c, oracle, name, cases, out, st, live_before, what, seen_sites, rewarm):
    """the two ways a fired refusal may end; `what` names the sweep and N for the messages"""
    kind, res = out
    assert st[1] == 1, what
    if kind == "oom":
        assert res.code == OOM, "%s: the call failed with %d (%s), not STARK_ERR_OOM" % (what, res.code, res)
        msg = last_error(c)
        assert ("alloc" in msg or "out of memory" in msg) and "no_such_option" not in msg, "%s: stark_last_error does not name the allocation: %r" % (what, msg)
        assert c.lib.oom, what
        for fn, args in c.lib.oom:
            if fn in HANDLE_OUT:
                assert handles_are_null(fn, args), "%s: %s returned STARK_ERR_OOM and left a handle" % (what, fn)
        c.sync()
        check(run_all(c, cases), cases, what + ", the unarmed repeat")
        live = c.diag_alloc_refusal(-1)[2]
        assert live == live_before, "%s: %d pooled blocks live after the refused call and its repeat, %d before" % (what, live, live_before)
        c.trim()
        assert c.cached_bytes() == 0, what
        if rewarm:
            check(run_all(c, cases), cases, what + ", after the trim")
    else:
        check(res, cases, what + ", the run that swallowed the refusal")
        note = last_error(c)
        assert note.startswith(NOTE), "%s: the call succeeded although request %d was refused, and not at an optional table (%r): a swallowed failure" % (what, st[0], note)
        site = note[len(NOTE):].split(" ")[0]
        assert site in DEGRADES.get(name, set()), "%s: degraded at %s, which the group's list does not hold" % (what, site)
        seen_sites.add(site)
        check(run_all(c, cases), cases, what + ", again on the degraded plan")
        alt = alt_coset_cases(oracle, ALT_LOGS[name])
        check(run_all(c, alt), alt, what + ", another coset")
        check(run_all(c, cases), cases, what + ", back on the first coset")


def spied(ctx, options):
    ctx.lib = Spy(ctx.lib)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def sweep(oracle, name, cases, options, fresh, session_ctx=None):
    """-> (requests of an unarmed run, refusals fired, sites that degraded).  session_ctx: the warm sweep on a context somebody else owns (the
    session's: it holds the t = 129 constants); its library handle and its hook are put back, and it is left open"""
    sites, fired = set(), 0
    assert not (fresh and session_ctx)
    ctx = session_ctx
    lib0 = ctx.lib if ctx else None
    try:
        ctx = spied(ctx if ctx else Context(0), options)
        if not fresh:
            check(run_all(ctx, cases), cases, "%s, the warming run" % name)
        ctx.diag_alloc_refusal(1, 0)                                          # count only
        check(run_all(ctx, cases), cases, "%s, the counting run" % name)
        total, none_fired, live_before = ctx.diag_alloc_refusal(0)[:3]
        assert none_fired == 0 and total > 0, (name, total)
        assert session_ctx or live_before == 0, "%s: %d pooled blocks live after a run that freed its handles" % (name, live_before)
        for n in range(1, 4 * total + 8):
            if fresh:
                ctx.close(); ctx = spied(Context(0), options)
            ctx.lib.oom.clear()
            what = "%s, %s sweep, request %d" % (name, "cold" if fresh else "warm", n)
            out, st = armed_run(ctx, cases, 1, n)
            if st[1] == 0:
                assert out[0] == "ok", "%s: nothing was refused and the call failed: %s" % (what, out[1])
                check(out[1], cases, what)
                break
            fired += 1
            after_refusal(ctx, oracle, name, cases, out, st, live_before, what, sites, rewarm=not fresh)
        else:
            pytest.fail("%s: the sweep did not end after %d requests" % (name, 4 * total + 8))
        assert fired >= total, "%s: the %s sweep fired %d refusals and an unarmed run makes %d requests" % (name, "cold" if fresh else "warm", fired, total)
        return total, fired, sites
    finally:
        if session_ctx is not None:
            session_ctx.diag_alloc_refusal(0); session_ctx.lib = lib0
        elif ctx is not None:
            ctx.close()


SITES = {}                                                   # group -> the sites its sweeps degraded at


@pytest.mark.parametrize("name", ac.GROUPS)
def test_cold_sweep(oracle, name):
    cases, options = ac.group(oracle, name)
    total, fired, sites = sweep(oracle, name, cases, options, fresh=True)
    RECORDS.append(dict(group=name, sweep="cold", requests=total, refusals=fired, degraded_at=sorted(sites)))
    SITES.setdefault(name, set()).update(sites)
    assert sites <= DEGRADES.get(name, set())


@pytest.mark.parametrize("name", ac.GROUPS)
def test_warm_sweep(oracle, name):
    cases, options = ac.group(oracle, name)
    total, fired, sites = sweep(oracle, name, cases, options, fresh=False)
    RECORDS.append(dict(group=name, sweep="warm", requests=total, refusals=fired, degraded_at=sorted(sites)))
    SITES.setdefault(name, set()).update(sites)
    assert sites <= DEGRADES.get(name, set())


@pytest.mark.parametrize("name", sorted(DEGRADES))
def test_the_list_of_optional_sites_is_exact(oracle, name):
    """the cold and the warm sweep of the group together met every site the list holds (they run first in this file; alone, this test runs them)"""
    if name not in SITES:
        cases, options = ac.group(oracle, name)
        for fresh in (True, False):
            SITES.setdefault(name, set()).update(sweep(oracle, name, cases, options, fresh=fresh)[2])
    assert SITES[name] == DEGRADES[name], "%s: the sweeps degraded at %s, the list holds %s" % (name, sorted(SITES[name]), sorted(DEGRADES[name]))


@pytest.mark.parametrize("name", ac.SESSION_GROUPS)
def test_warm_sweep_on_the_session_context(oracle, gpu_ctx, name):
    """the groups that need the t = 129 constants (the whole mixed_prove_cases.PROVE_ORDER): the warm sweep on the session's context, which derives
    them once; the same batch without the [128] trace is swept cold above"""
    cases, options = ac.group(oracle, name)
    total, fired, sites = sweep(oracle, name, cases, options, fresh=False, session_ctx=gpu_ctx)
    RECORDS.append(dict(group=name, sweep="warm", requests=total, refusals=fired, degraded_at=sorted(sites)))
    assert not sites


FOREIGN_LOG = 17                                             # a forward NTT of 2^17 points takes ONE pooled block, of 4 MiB: a size no case asks for
NEVER = (1 << 64) - 1


def retry_modes(oracle, c, name, cases):
    """Modes 2 and 3 for each pool miss m of the group.  Before each run the cache is trimmed and then holds a foreign block of 4 MiB,
    which serves no request of any case: the requests of the run miss.
      mode 2  the first hipMalloc of miss m is refused; ctx_alloc synchronises, hands the cached blocks back and its second attempt succeeds.  The call
              succeeds and equals the oracle.
      mode 3  the second attempt is refused too: the call fails with STARK_ERR_OOM behind an emptied cache, and its unarmed repeat equals the oracle.
    In both, the fifth statistic — the cached bytes by the give-back's own accounting, taken right after it — is 0, the foreign block is gone from
    the cache afterwards (the cached bytes are at least 4 MiB below those of the same run without a refusal), and the blocks of a tree built BEFORE,
    still held by its handle, are untouched: its root is read again and compared with the oracle's."""
    f = mc.leaves_of(oracle, pp.SEED, 0, 257); o = oracle.merkle_build(16, 0x5EED, f); want_root = o.root().copy(); o.free()
    key = ("foreign", FOREIGN_LOG)
    if key not in ac._memo:
        ac._memo[key] = oracle.synth_column(0xF0E16, 0, 0, 1 << FOREIGN_LOG)
    foreign = ac._memo[key]
    held = c.merkle_new(f, c.merkle_cfg(16, 0x5EED))
    try:
        def state():
            c.trim(); assert c.cached_bytes() == 0
            c.fft(foreign, field=PALLAS_FR)
            assert c.cached_bytes() >= 4 << 20, c.cached_bytes()
        check(run_all(c, cases), cases, name + ", the warming run")
        state(); c.diag_alloc_refusal(2, 0)
        check(run_all(c, cases), cases, name + ", the counting run")
        misses, none_fired, live, _, gave_back = c.diag_alloc_refusal(0); cached_plain = c.cached_bytes()
        assert none_fired == 0 and gave_back == NEVER and misses > 0, (misses, none_fired, gave_back)
        for m in range(1, misses + 1):
            what = "%s, pool miss %d of %d" % (name, m, misses)
            state(); c.diag_alloc_refusal(2, m)
            got = run_all(c, cases)
            st = c.diag_alloc_refusal(0)
            assert st[1] == 1 and st[2] == live and st[4] == 0, (what, st)
            check(got, cases, what + " retried")
            assert c.cached_bytes() <= cached_plain - (4 << 20), "%s: %d bytes cached after the give-back, %d without it" % (what, c.cached_bytes(), cached_plain)
            assert (held.root() == want_root).all(), "%s: the root of a tree built before changed" % what
            state(); stale_error(c); c.diag_alloc_refusal(3, m)
            with pytest.raises(StarkError) as e:
                run_all(c, cases)
            st = c.diag_alloc_refusal(0)
            assert e.value.code == OOM and ("alloc" in last_error(c) or "out of memory" in last_error(c)), (what, e.value)
            assert st[1] == 1 and st[4] == 0, (what, st)
            c.sync()
            assert c.cached_bytes() <= cached_plain - (4 << 20), what
            check(run_all(c, cases), cases, what + ", the repeat after both attempts were refused")
            assert c.diag_alloc_refusal(-1)[2] == live, what
            assert (held.root() == want_root).all(), "%s: the root of a tree built before changed" % what
        RECORDS.append(dict(group=name, pool_misses_after_trim=misses))
    finally:
        c.diag_alloc_refusal(0)
        held.free()


@pytest.mark.parametrize("name", ac.GROUPS)
def test_retry_after_giving_the_cache_back(oracle, name):
    cases, options = ac.group(oracle, name)
    with own_context(**options) as c:
        retry_modes(oracle, c, name, cases)


@pytest.mark.parametrize("name", ac.SESSION_GROUPS)
def test_retry_on_the_session_context(oracle, gpu_ctx, name):
    cases, options = ac.group(oracle, name)
    assert not options
    retry_modes(oracle, gpu_ctx, name, cases)


def test_the_hook_is_off_by_default_and_counts_what_it_says(oracle):
    """the helper can fail: unarmed nothing is counted; count-only counts and refuses nothing; a hook that fired disarms itself; the five numbers"""
    (name, run, want), = [("arity 16, n = 257",) + pp.tree_case(oracle, 16, 257)]
    with own_context() as c:
        assert c.diag_alloc_refusal(-1) == (0, 0, 0, 0, NEVER)
        assert equal(run(c), want) and c.diag_alloc_refusal(-1)[:2] == (0, 0)
        t = c.merkle_new(mc.leaves_of(oracle, pp.SEED, 0, 257), c.merkle_cfg(16, 0x5EED))
        st = c.diag_alloc_refusal(1, 0)
        assert st[2] == 4 and st[3] == sum(pp.pool_round(32 * n) for n in (257, 17, 2, 1)), st      # four levels, a block each
        t.free()
        assert equal(run(c), want)
        total, fired, live, nbytes = c.diag_alloc_refusal(1, 1)[:4]
        assert total > 0 and (fired, live, nbytes) == (0, 0, 0)
        with pytest.raises(StarkError) as e:
            run(c)
        assert e.value.code == OOM
        assert equal(run(c), want)                                               # disarmed by firing; still counting
        seen, fired = c.diag_alloc_refusal(0)[:2]
        assert fired == 1 and seen == 1 + total
        for bad in (-2, 4):
            with pytest.raises(StarkError):
                c.diag_alloc_refusal(bad)


def test_one_degraded_plan_inside_a_ragged_launch(oracle):
    """The mixed LDE of {8, 5, 11} at blow-up 3 after ONE of its plans was degraded by a single-column call at that size: each optional site of the
    single 2^11 -> 2^14 call in turn (a context each), then the ragged launch — shapes with and without direct and merged tables side by side —
    equals the oracle on every column, and so does stark_lde of each column alone."""
    g = oracle.from_u64(5); xs = ac.mixed_lde_inputs(oracle); want = [oracle.lde(0, x, ac.MIXED_BLOWUP, g) for x in xs]
    mixed = ac.mixed_lde_run(xs, g); seen = set()
    for col in (2, 0):                                                            # the 2^14 plan (two passes), then the 2^11 plan
        single = lambda c: c.lde(xs[col], ac.MIXED_BLOWUP, field=PALLAS_FR, coset=g)
        for n in range(1, 64):
            with own_context() as c:
                stale_error(c); c.diag_alloc_refusal(1, n)
                try:
                    got = single(c)
                except StarkError as e:
                    assert e.code == OOM
                    got = None
                fired = c.diag_alloc_refusal(0)[1]
                if not fired:
                    break
                if got is None:
                    continue
                note = last_error(c)
                assert equal(got, want[col]) and note.startswith(NOTE), (col, n, note)
                seen.add((col, note[len(NOTE):].split(" ")[0]))
                assert equal(mixed(c), want), "the ragged launch after the single call degraded at %s (column %d)" % (note, col)
                for b, x in enumerate(xs):
                    assert equal(c.lde(x, ac.MIXED_BLOWUP, field=PALLAS_FR, coset=g), want[b]), (col, n, b)
                assert equal(mixed(c), want)
        else:
            pytest.fail("the sweep of the single call did not end")
    RECORDS.append(dict(test="one degraded plan", degraded_at=sorted("column %d: %s" % cs for cs in seen)))
    assert PLAN2 | MERGED <= {s for col, s in seen if col == 2}, seen            # the 2^14 plan has two passes: its own direct table and the merged coset tables


# ---- behind a busy stream ---------------------------------------------------------------------------------------------------------------------
def busy_cases(oracle):
    """name -> (queue(c) -> finish() -> result, the oracle's result, refused(c) -> (rc, the handle table, free(handle)), the request to refuse or None
    for the middle one, the context's options)"""
    import torch
    arity, n, B = 16, 257, 3
    labels = mc.labels_of(B); leaves = [mc.leaves_of(oracle, pp.SEED, b, n) for b in range(B)]
    roots = []
    for b in range(B):
        o = oracle.merkle_build(arity, labels[b], leaves[b]); roots.append(o.root().copy()); o.free()
    dl = [dev(v) for v in leaves]

    def build_queue(c):
        trees = c.merkle_build_batch_dev([t.data_ptr() for t in dl], n, arity, labels, c.poseidon_params_for_arity(arity))

        def finish():
            try:
                return [r for r in c.merkle_roots_batch(trees)]
            finally:
                for t in trees:
                    t.free()
        return finish

    def build_refused(c):
        tab = (vp * B)(*[t.data_ptr() for t in dl]); lab = np.ascontiguousarray(labels, dtype=np.uint64); out = (vp * B)()
        rc = c.lib.stark_merkle_build_batch_dev(c.h, c.poseidon_params_for_arity(arity).h, arity, B, lab.ctypes.data_as(vp), tab, n, 0, None, out)
        return rc, out, c.lib.stark_merkle_free
    # four columns in passes of two (ntt_batch_max_elems = 2 * 2^11 outputs): a pass takes one pooled block, for its tables, before its launches, so
    # the second request of the call is refused after the first pass has been enqueued
    log_n, lb, g, BL = 10, 1, oracle.from_u64(5), 4
    xs = [oracle.synth_column(0xBA7C200 + log_n, b, 0, 1 << log_n) for b in range(BL)]; dx = [dev(x) for x in xs]
    lde_want = [oracle.lde(0, x, lb, g) for x in xs]

    def lde_call(c, outs):
        tab = (vp * BL)(*[t.data_ptr() for t in dx]); otab = (vp * BL)(*[o.data_ptr() for o in outs]); gg = np.ascontiguousarray(g, dtype=np.uint64)
        return c.lib.stark_lde_batch_dev(c.h, PALLAS_FR, BL, tab, log_n, lb, gg.ctypes.data_as(vp), otab)

    def lde_queue(c):
        outs = [ac.out_rows(1 << (log_n + lb)) for _ in xs]
        c._chk(lde_call(c, outs))
        return lambda: [host(o) for o in outs]
    scratch_outs = [ac.out_rows(1 << (log_n + lb)) for _ in xs]
    n0, sched, r = 1 << 10, [16, 8], 8
    traces = [[dev(col) for col in oracle.rand_fr_columns(0x7A11 + b, n0, 4)] for b in range(2)]

    def prove_refused(c):
        cols = [(vp * 2)(*[tr[k].data_ptr() for tr in traces]) for k in range(4)]; sch = np.ascontiguousarray(sched, dtype=np.uint64); out = (vp * 2)()
        rc = c.lib.stark_deep_fri_prove_batch_dev(c.h, 2, cols[0], cols[1], cols[2], cols[3], n0, sch.ctypes.data_as(vp), len(sched), r, pp.SEED_Z, out)
        return rc, out, c.lib.stark_proof_free
    torch.cuda.synchronize()
    # the batched prove downloads its column digests (a synchronisation) right after its second request: request 2 is the last one that can be
    # refused while the stream is still busy, and the block of request 1 goes back to the pool with A and the blocker pending
    opt = {"ntt_batch_max_elems": 2 << (log_n + lb)}
    return {"merkle batch build": (build_queue, roots, build_refused, None, {}), "lde batch": (lde_queue, lde_want, lambda c: (lde_call(c, scratch_outs), (), None), 2, opt),
            "batched prove": (lde_queue, lde_want, prove_refused, 2, opt)}


@pytest.mark.parametrize("name", ["merkle batch build", "lde batch", "batched prove"])
def test_refused_behind_a_busy_stream(oracle, name):
    """A long sponge holds the stream (queued_cases.Blocker); a clean call A is queued behind it; the armed call B is queued behind A and refused
    part-way, so B unwinds — its blocks go back to the pool — while its own earlier launches, A and the blocker are still pending.  B returns
    STARK_ERR_OOM while the blocker still runs (require_busy's condition at that moment); A's output, downloaded afterwards, is the oracle's, and so
    is the blocker's own digest."""
    queue, want, refused, at, options = busy_cases(oracle)[name]
    with own_context(**options) as c:
        qc.Blocker(c, oracle, 16).start(); c.sync()                          # the blocker's tag frame
        assert equal(queue(c)(), want)                                       # warm: plans, frames, parameter sets, the pool
        c.diag_alloc_refusal(1, 0); rc, handles, free = refused(c); total = c.diag_alloc_refusal(0)[0]
        assert rc == 0, last_error(c)
        for h in handles:
            free(vp(h))
        c.sync()
        n = at if at is not None else max(2, total // 2)
        assert 1 < n <= total, (n, total)
        blocker = qc.Blocker(c, oracle).start()
        finish = queue(c)
        c.diag_alloc_refusal(1, n)
        rc, handles, _ = refused(c)
        busy = blocker.still_busy()
        st = c.diag_alloc_refusal(0)
        assert rc == OOM and st[1] == 1, (rc, st, last_error(c))
        assert all(not h for h in handles), name
        assert busy, "%s: the refused call (request %d of %d) returned only after the blocker (%.1f ms) had finished: it waited for the stream" % (name, n, total, blocker.ms())
        assert equal(finish(), want), "%s: the clean call queued before the refused one differs from the oracle" % name
        blocker.check()
        assert equal(queue(c)(), want)
        assert c.diag_alloc_refusal(-1)[2] == 0
