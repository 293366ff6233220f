"""Host sources of the plain-named entry points: a call returns, with ANY status, only after the device has finished reading the caller's arrays.

Each case prepares its arguments, starts a Blocker (queued_cases.py: one long serial sponge and an event behind it), asserts that the stream is still
busy immediately before the call — so the call's upload really queues behind work — makes the call, asserts its status and that the blocker's event is
complete on return (the call fenced its uploads), overwrites every host argument, checks the blocker's own digest, and then makes one successful
stark_fri_build on the same context whose roots must be the oracle's (the context is still usable).  Cases 2 - 5 are ordinary argument refusals that
the library raises AFTER it has enqueued the upload of the caller's memory; case 1 is the success path of stark_fri_build, whose commit phase only
enqueues.  A sixth case, a sum-check prove that the batch driver refuses behind the entry check, does not exist: both refuse exactly k > 40.
Every case runs on the session's default-stream context and on a context created on a torch stream, as test_gpu_queued_calls.py does.  Needs an
MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import queued_cases as qc
from test_gpu_guard_bands import hp
from test_gpu_queued_calls import CONTEXTS, on, stream_ctx  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
vp = C.c_void_p
OK, INVALID_ARG = 0, -1
N8 = qc.N8
SCHEDULE = [4, 2]
BLOCKER_K = 1 << 14                        # a quarter of queued_cases.BLOCKER_K: tens of milliseconds in front of one call; still_busy() is asserted, not assumed
_ref = {}


def column(oracle, c, n=N8):
    return oracle.synth_column(0x4057, c, 0, n)


def fri_roots_ref(oracle):
    """the roots of fri_build(column 4, [4, 2]) on the oracle, computed once"""
    if "roots" not in _ref:
        p = oracle.deep_fri_prove(None, None, None, None, N8, SCHEDULE, 1, qc.SEED_Z, f0=column(oracle, 4))
        try:
            _ref["roots"] = np.stack([p.root(l) for l in range(len(SCHEDULE) + 1)])
        finally:
            p.free()
    return _ref["roots"]


def state_roots(ctx, state, L):
    out = np.zeros((L + 1, 4), np.uint64)
    for l in range(L + 1):
        ctx._chk(ctx.lib.stark_fri_layer_root(state, l, hp(out[l])))
    return out


def build_and_check(ctx, oracle, what):
    """one successful stark_fri_build of column 4 under [4, 2]: its roots are the oracle's"""
    f0 = column(oracle, 4); sch = np.array(SCHEDULE, np.uint64); state = vp()
    ctx._chk(ctx.lib.stark_fri_build(ctx.h, hp(f0), N8, hp(sch), len(SCHEDULE), qc.SEED_Z, C.byref(state)))
    try:
        got = state_roots(ctx, state, len(SCHEDULE))
    finally:
        ctx.lib.stark_fri_state_free(state)
    assert (got == fri_roots_ref(oracle)).all(), "%s: the roots of a stark_fri_build on this context differ from the oracle's" % what


def fenced(on, oracle, context, prepare, want_rc, what, after=None):
    """The steps around one call.  prepare(ctx) -> (fn, host): fn() makes the call and returns its status, host are its host arguments.
    after(ctx): checks of the call's own results, run once the host arguments are overwritten."""
    import torch
    ctx, stream = on(context)
    torch.cuda.synchronize()
    with qc.on_stream(stream):
        build_and_check(ctx, oracle, what + ", before")                                    # warm: plans, parameter sets and tag frames exist, so the call has no other reason to wait
        warm = qc.Blocker(ctx, oracle, 16).start(); ctx.sync(); warm.check()               # ... and the blocker's tag frame
        fn, host = prepare(ctx)
        b = qc.Blocker(ctx, oracle, BLOCKER_K).start()
        assert b.still_busy(), "%s: the blocker had finished before the call was made: its upload would not queue behind work" % what
        rc = fn()
        done = not b.still_busy()
        qc.clobber(*host)
        assert rc == want_rc, "%s: status %d, expected %d (%r)" % (what, rc, want_rc, ctx.lib.stark_last_error(ctx.h))
        assert done, "%s returned %d while the blocker in front of its upload still ran: the device may not have read the caller's arrays yet" % (what, rc)
        ctx.sync(); b.check()
        if after:
            after(ctx)
        build_and_check(ctx, oracle, what + ", afterwards")
    torch.cuda.synchronize()


def fri_build_case(oracle, schedule, got):
    def prepare(ctx):
        f0 = column(oracle, 4).copy(); sch = np.array(schedule, np.uint64); got["state"] = vp()
        return (lambda: ctx.lib.stark_fri_build(ctx.h, hp(f0), N8, hp(sch), len(schedule), qc.SEED_Z, C.byref(got["state"]))), (f0, sch)
    return prepare


@pytest.mark.parametrize("context", CONTEXTS)
def test_fri_build_success_reads_f0_before_return(on, oracle, context):
    """case 1: stark_fri_build, schedule [4, 2], n0 = 2^8: STARK_OK, and the roots are the oracle's although f0 was overwritten on return"""
    got = {}

    def after(ctx):
        roots = state_roots(ctx, got["state"], len(SCHEDULE))
        assert (roots == fri_roots_ref(oracle)).all(), "stark_fri_build: the roots differ from the oracle's after f0 was overwritten on return"

    ctx, _ = on(context)
    try:
        fenced(on, oracle, context, fri_build_case(oracle, SCHEDULE, got), OK, "stark_fri_build [4, 2]", after)
    finally:
        if got.get("state"):
            ctx.lib.stark_fri_state_free(got["state"])


@pytest.mark.parametrize("context", CONTEXTS)
def test_fri_build_refused_schedule(on, oracle, context):
    """case 2: stark_fri_build, schedule [3] does not divide 2^8: refused after f0 was enqueued"""
    got = {}
    fenced(on, oracle, context, fri_build_case(oracle, [3], got), INVALID_ARG, "stark_fri_build [3]")
    assert not got["state"], "a refused stark_fri_build wrote a state handle"


@pytest.mark.parametrize("context", CONTEXTS)
def test_ali_merge_z_inside_h(on, oracle, context):
    """case 3: stark_ali_merge with z = 1 (inside H), n = 2^8: refused after the four columns were enqueued"""
    def prepare(ctx):
        cols = [column(oracle, c).copy() for c in range(4)]
        omega, z, f0 = np.array(oracle.domain_omega(N8)), np.array(oracle.from_u64(1)), np.zeros((N8, 4), np.uint64)
        return (lambda: ctx.lib.stark_ali_merge(ctx.h, hp(cols[0]), hp(cols[1]), hp(cols[2]), hp(cols[3]), None, None, hp(omega), hp(z), N8, hp(f0), None)), cols + [omega, z, f0]
    fenced(on, oracle, context, prepare, INVALID_ARG, "stark_ali_merge, z = 1")


@pytest.mark.parametrize("context", CONTEXTS)
def test_deep_fri_prove_f0_not_power_of_two(on, oracle, context):
    """case 4: stark_deep_fri_prove with a host f0 of n0 = 24 rows: refused after f0 was enqueued, *out untouched"""
    out = vp(0x5A5A5A5A)

    def prepare(ctx):
        f0 = column(oracle, 4, 24).copy(); sch = np.array([2], np.uint64)
        return (lambda: ctx.lib.stark_deep_fri_prove(ctx.h, None, None, None, None, hp(f0), 24, hp(sch), 1, 1, qc.SEED_Z, C.byref(out))), (f0, sch)
    fenced(on, oracle, context, prepare, INVALID_ARG, "stark_deep_fri_prove, n0 = 24")
    assert out.value == 0x5A5A5A5A, "a refused stark_deep_fri_prove wrote *out"


@pytest.mark.parametrize("context", CONTEXTS)
def test_merkle_build_arity_incompatible(on, oracle, context):
    """case 5: stark_merkle_build of 2^8 leaves with the t = 9 parameter set and arity 16: refused after the leaves were enqueued"""
    tree = vp()

    def prepare(ctx):
        p9 = ctx.poseidon_params_for_arity(8)                                              # made (and synchronised) before the blocker starts
        leaves = column(oracle, 0).copy()
        return (lambda: ctx.lib.stark_merkle_build(ctx.h, p9.h, 16, 7, hp(leaves), N8, 0, None, C.byref(tree))), (leaves,)
    fenced(on, oracle, context, prepare, INVALID_ARG, "stark_merkle_build, t = 9 with arity 16")
    assert not tree, "a refused stark_merkle_build wrote a tree handle"
