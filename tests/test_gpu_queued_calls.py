"""The no-synchronisation promises of include/stark_mlwe.h under a busy stream (the harness and the cases: queued_cases.py).

Every pipeline runs (a) with each call bracketed by a synchronisation, (b) queued back to back behind a blocker — one long serial sponge that is
provably still running when the last call of the section returns — with every host argument (pointer tables, points, challenges, labels, tags)
overwritten the moment each call returns and ONE download of all outputs at the end, and (c) on the CPU oracle: (a) == (c) and (b) == (c), byte for
byte, guard bands clean, inputs intact, the blocker's own digest the oracle's.  For every entry point that promises "no host synchronisation" the
blocker must still be busy right after the call returns (a call that drained the stream fails with its name); for the entry points that are only
stream-ordered (Q4) the observation is recorded, not asserted.  Q1 - Q3 run on the session's default-stream context and on a context created on a
torch stream, as bench.py's is.  No time is asserted.  Needs an MI355X (`pytest -m gpu`); the helpers and the references are tested on the CPU in
test_queued_cases_host.py."""
import ctypes as C

import numpy as np
import pytest

import queued_cases as qc
from test_gpu_guard_bands import Band
from test_gpu_lagrange_eval import options

pytestmark = pytest.mark.gpu
CONTEXTS = ("default stream", "torch stream")


@pytest.fixture(scope="module")
def stream_ctx():
    """a context on a torch stream of its own (bench.py's arrangement), closed at the end of the module"""
    import torch
    from stark_mlwe_amd.api import Context
    s = torch.cuda.Stream()
    c = Context(0, C.c_void_p(s.cuda_stream))
    yield c, s
    c.close()


@pytest.fixture
def on(request, gpu_ctx):
    """context name -> (context, torch stream or None)"""
    def pick(name):
        return (gpu_ctx, None) if name == "default stream" else request.getfixturevalue("stream_ctx")
    return pick


def run(on, oracle, name, pipeline, ref, what, **kw):
    import torch
    ctx, stream = on(name)
    torch.cuda.synchronize()
    with qc.on_stream(stream):
        r = qc.three_runs(ctx, oracle, pipeline, ref, what, name, **kw)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("context", CONTEXTS)
@pytest.mark.parametrize("commit", [False, True], ids=["merkle_build_batch", "commitment_commit_batch"])
def test_q1_extend_commit_hash_free_rebuild(on, oracle, context, commit):
    """stark_lde_batch_dev (3 columns 2^8 -> 2^11 on a coset) -> stark_merkle_build_batch_dev / stark_commitment_commit_batch_dev over its outputs ->
    stark_tr_hash_many_dev over the roots in place, an empty item and 200 elements of output 0 -> stark_merkle_free of all three trees while that hash
    is queued -> a second build of the same shape, which must take the released level blocks (stark_ctx_cached_bytes returns to the same value) ->
    the hash of the new roots.  A reuse not ordered behind the reader would hash the second batch's roots in the first hash."""
    run(on, oracle, context, qc.q1, qc.q1_refs(oracle, commit)["results"], "Q1, commit = %s" % commit, commit=commit)


@pytest.mark.parametrize("context", CONTEXTS)
@pytest.mark.parametrize("small", [False, True], ids=["default options", "small passes"])
def test_q2_open_and_evaluate(on, oracle, context, small):
    """Lagrange evaluation (batch: 3 points, one inside H; single), MLE evaluation (batch at k = 11; single), stark_ntt_batch_dev in place (inverse,
    then forward on a coset), stark_ntt_dev and stark_lde_dev, all queued on three resident 2^11 columns; with the default options and with
    mle_log_tile = 4 (three launches on pooled ping-pong blocks), lagrange_max_partials = 1 (one point per pass) and ntt_batch_max_elems = 2^11 (one
    column per pass).  Setting an option synchronises, so the options are set before the blocker."""
    ctx, _ = on(context)
    if not small:
        run(on, oracle, context, qc.q2, qc.q2_refs(oracle), "Q2, default options")
        return
    try:
        with options(ctx, mle_log_tile=4, lagrange_max_partials=1):
            ctx.set_option("ntt_batch_max_elems", qc.N11)
            run(on, oracle, context, qc.q2, qc.q2_refs(oracle), "Q2, small passes")
    finally:
        ctx.set_option("ntt_batch_max_elems", 1 << 24)                   # this option takes no -1: its default by value


@pytest.mark.parametrize("context", CONTEXTS)
def test_q3_many_staged_uploads_in_flight(on, oracle, context):
    """300 stark_tr_hash_many_dev calls of two items behind one blocker: hundreds of staged host copies are alive at once and later calls reap
    finished ones while others are in flight; all 600 digests are the oracle's.  Afterwards a synchronised call is still correct."""
    import torch
    ctx, stream = on(context)
    run(on, oracle, context, qc.q3, qc.q3_refs(oracle), "Q3")
    with qc.on_stream(stream):
        pool = Band([qc.q3_pool(oracle)]); out = Band([2])
        r = qc.Run(ctx, oracle, "sync")
        qc.hash_many(r, [(qc.TAGS[2], pool.ptr(0).value + 32 * 5, 33), (qc.TAGS[0], None, 0)], out.ptr(0).value)
        host = out.host(); out.check("the synchronised call after Q3", host)
        want = np.stack([qc.digest(oracle, qc.TAGS[2], qc.q3_pool(oracle)[5:38]), qc.digest(oracle, qc.TAGS[0], [])])
        assert (out.payload(0, host) == want).all(), "a synchronised stark_tr_hash_many_dev after Q3 differs from the oracle"
    torch.cuda.synchronize()


def test_q3_destroy_with_uploads_outstanding(oracle):
    """stark_ctx_destroy of a private context whose staged uploads are still queued behind a blocker returns STARK_OK (it synchronises first), and
    what was queued is correct"""
    import torch
    from stark_mlwe_amd.api import Context
    c = Context(0)
    try:
        pool = Band([qc.q3_pool(oracle)]); out = Band([2 * 8])
        warm = qc.Run(c, oracle, "sync"); warm.begin()
        qc.hash_many(warm, [(t, None, 0) for t in qc.TAGS], out.ptr(0).value)                  # the tag frames
        r = qc.Run(c, oracle, "queued", k=1 << 13); r.begin()
        for j in range(8):
            qc.hash_many(r, [(tag, pool.ptr(0).value + 32 * off if k else None, k) for tag, off, k in qc.q3_items(j)], out.ptr(0).value + 64 * j)
        r.end()
        busy = r.busy_at_end
        rc = c.lib.stark_ctx_destroy(c.h); c.h = None
        assert rc == 0, "stark_ctx_destroy with %d staged uploads outstanding returned %d" % (8, rc)
        assert busy, "the uploads were not outstanding: the blocker had finished before stark_ctx_destroy was called"
        torch.cuda.synchronize()
        host = out.host(); out.check("Q3 on a private context", host); r.blocker.check()
        assert (out.payload(0, host) == qc.q3_refs(oracle)[0][1][:16]).all(), "the digests queued before stark_ctx_destroy differ from the oracle"
    finally:
        if c.h:
            c.close()


def test_q4_stream_ordered_calls_consume_queued_producers(gpu_ctx, oracle):
    """Behind a blocker: stark_lde_batch_dev of four columns -> stark_ali_merge_dev on the outputs -> stark_fri_build_dev on that f0 (forks the side
    stream) -> the state freed and at once a stark_merkle_build_batch_dev that recycles blocks the side stream touched -> stark_fri_fold_dev,
    stark_leaf_pair_hash_dev, stark_poseidon_hash_ds_batch_dev and stark_tr_hash_fields_tagged_dev, each fed by the call queued before it.  The header
    promises stream order for these, not an early return: the results are asserted, whether a call returned while the blocker ran is recorded."""
    import torch
    torch.cuda.synchronize()
    r = qc.three_runs(gpu_ctx, oracle, qc.q4, qc.q4_refs(oracle), "Q4", "default stream")
    assert set(r.table) >= {"stark_ali_merge_dev", "stark_fri_build_dev", "stark_fri_fold_dev", "stark_leaf_pair_hash_dev", "stark_poseidon_hash_ds_batch_dev",
                            "stark_tr_hash_fields_tagged_dev"}
