"""Refused allocations in the shared drivers, on the CPU.  HostArena (csrc/hostcheck.cpp) is the twin of the device executors' DevArena; armed with
hc_set_alloc_refuse_at(N) its N-th allocation request fails with STARK_ERR_OOM once, as the device allocator's does under stark_diag_alloc_refusal
(tests/test_gpu_alloc_refusal.py).  Every shared driver that has an hc_* export is swept: N = 1, 2, ... until a run ends with no refusal fired.
Each refused run must return -4 (not the -1 of a refused shape), and the unarmed repeat right after it must give the oracle's result byte for byte,
as the first, unarmed run does.  A sweep that stops early would hide sites: it must have fired as many refusals as the unarmed run counted
requests.  Exports whose driver takes nothing from the arena (the verify plans, the MLE pass loop, the transcript stream) count 0 requests; they
are swept all the same, so that a request added to them later is refused here the day it appears.  The same sweep runs under AddressSanitizer,
UBSan and the leak checker in tools/alloc_refusal_check.cpp (tools/alloc_refusal_sanitize.sh).  The shapes are those of the drivers' own host tests."""
import numpy as np
import pytest

import lagrange_cases as lc
import lagrange_shard_cases as ls
import merkle_batch_cases as mc
import mixed_batch_cases as xc
import mle_cases as mle
import test_fri_batch_host as fb
import test_merkle_batch_host as mb
import test_mixed_batch_host as xb
import test_sumcheck_batch_host as sb
import test_sumcheck_verify_batch_host as sv
import test_verify_batch_host as vb

OOM = -4
hc_params = mb.hc_params


@pytest.fixture(scope="module")
def tparams(hostcheck):
    h = hostcheck.params(1)
    yield h
    hostcheck.params_free(h)


@pytest.fixture(scope="module")
def cparams(hostcheck):
    h = hostcheck.params(2, 17, b"POSEIDON-T17-X5-SEED")
    yield h
    hostcheck.params_free(h)


def sweep(hostcheck, run, check, expect_requests=None):
    """run() -> (status: 0 on success, result); check(result) asserts the oracle's bytes.  -> the requests an unarmed run makes"""
    try:
        hostcheck.set_alloc_refuse_at(0)
        rc, res = run(); total, fired = hostcheck.alloc_refusal_stats()
        assert rc == 0 and fired == 0; check(res)
        n_fired = 0
        for n in range(1, total + 2):
            hostcheck.set_alloc_refuse_at(n)
            rc, res = run(); seen, fired = hostcheck.alloc_refusal_stats()
            hostcheck.set_alloc_refuse_at(0)
            if not fired:
                assert rc == 0, "request %d: nothing was refused, status %d" % (n, rc)
                check(res); break
            assert fired == 1 and seen == n, (n, seen, fired)                # the refused request is the driver's last: it stops there
            assert rc == OOM, "request %d of %d was refused and the export returned %d" % (n, total, rc)
            rc, res = run()
            assert rc == 0, "the unarmed repeat after refusal %d returned %d" % (n, rc)
            check(res); n_fired += 1
        else:
            pytest.fail("the sweep did not end after %d requests" % total)
        assert n_fired >= total and n_fired == total, (n_fired, total)
        if expect_requests is not None:
            assert (total > 0) == expect_requests, total
        return total
    finally:
        hostcheck.set_alloc_refuse_at(0)


def test_the_countdown_refuses_exactly_one_request(hostcheck, oracle, hc_params):
    """the helper can fail: unarmed nothing is refused; armed past the last request nothing is refused and the count is the unarmed one"""
    arity, n, B = 16, 17, 2
    labels, cols, cps, want = mb.batch_inputs(oracle, arity, n, False, B)
    run = lambda: mb.hc_build_rc(hostcheck, hc_params(arity), arity, labels, cols, n, cps)[0]
    levels = want[0].num_levels()
    hostcheck.set_alloc_refuse_at(0); assert run() == levels; total, fired = hostcheck.alloc_refusal_stats(); assert total > 0 and fired == 0
    hostcheck.set_alloc_refuse_at(total + 1); assert run() == levels; assert hostcheck.alloc_refusal_stats() == (total, 0)
    hostcheck.set_alloc_refuse_at(total); assert run() == OOM; assert hostcheck.alloc_refusal_stats() == (total, 1)
    assert run() == levels and hostcheck.alloc_refusal_stats() == (2 * total, 1)      # it fired once and disarmed itself
    hostcheck.set_alloc_refuse_at(0)


@pytest.mark.parametrize("shape", [0, 1, 3])
def test_fri_commit_batch(hostcheck, tparams, oracle, shape):
    """FriBatchCommit::init and run: the layers, the roots, the labels, the z powers, every level block of the climbs.  (The [128] shape of
    test_fri_batch_host.py adds no allocation site, only the derivation of the t = 129 constants.)"""
    import test_pool_poison_host as pp
    k, sched, _ = fb.SHAPES[shape]; B = 1 if shape == 1 else 2            # the 2^10 shape costs a second per run on the host: one trace
    f0s, want = pp._fri_reference(oracle, shape)

    def check(roots):
        assert (roots == want[:B]).all()
    sweep(hostcheck, lambda: fb.commit_batch_rc(hostcheck, tparams, f0s[:B], 1 << k, sched, 0xDEEFBAAD + shape), check, True)


@pytest.mark.parametrize("arity,n,pairs", [(16, 257, False), (16, 257, True), (4, 64, True), (2, 5, False), (16, 1, False)])
def test_merkle_build_batch(hostcheck, hc_params, oracle, arity, n, pairs):
    B = 3
    labels, cols, cps, want = mb.batch_inputs(oracle, arity, n, pairs, B)

    def run():
        nl, built = mb.hc_build_rc(hostcheck, hc_params(arity), arity, labels, cols, n, cps)
        return (0 if nl >= 0 else nl), built

    def check(built):
        lens, trees = built
        for b in range(B):
            assert len(trees[b]) == want[b].num_levels()
            assert all((trees[b][v] == want[b].level(v)).all() for v in range(len(lens))), b
    sweep(hostcheck, run, check, True)


@pytest.mark.parametrize("arity,pairs", [(8, False), (8, True), (16, False), (32, False)])
def test_merkle_build_mixed_batch(hostcheck, hc_params, oracle, arity, pairs):
    """the pair form adds one site (the leaf block and the cp table), which the arity-8 set crosses at a quarter of the hashes of the other two"""
    ns = xc.SETS[arity]; labels, cols, cps = xb.mixed_inputs(oracle, arity, ns, pairs)
    want = [xc.oracle_tree(oracle, arity, b, n, pairs, labels[b]) for b, n in enumerate(ns)]

    def run():
        depth, trees = xb.hc_build_mixed_rc(hostcheck, hc_params(arity), arity, labels, cols, cps)
        return (0 if depth >= 0 else depth), trees

    def check(trees):
        for b in range(len(ns)):
            assert len(trees[b]) == want[b].num_levels()
            assert all((trees[b][v] == want[b].level(v)).all() for v in range(want[b].num_levels())), b
    sweep(hostcheck, run, check, True)


def test_merkle_verify_batch(hostcheck, hc_params, oracle):
    arity, n, B = 16, 257, 3
    labels, cols, cps, want = mb.batch_inputs(oracle, arity, n, False, B)
    items, expect = [], []
    for b in range(B):
        ix = mc.index_lists(n, b); vals = want[b].level(0)[ix]; root = want[b].level(want[b].num_levels() - 1)[0]
        for name, lab, rt, i, v, pr in mc.tamperings(labels[b], root, ix, vals, want[b].open_bytes(ix), n):
            items.append((lab, rt, i, v, pr)); expect.append(mc.oracle_verify(arity, lab, rt, i, v, pr))
    assert 1 in expect and 0 in expect

    def check(got):
        assert got == expect
    for slots in (0, 1):
        sweep(hostcheck, lambda: (0, mb.hc_verify(hostcheck, arity, items, max_slots=slots)), check)


def test_deep_fri_verify_batch(hostcheck, tparams, oracle):
    n0, sched, r = 64, [8, 8], 4
    proof = vb.make_proof(oracle, n0, sched, r, 77 + n0)
    bad = bytearray(proof); bad[len(proof) // 3] ^= 4
    batch = [proof, vb.make_proof(oracle, 2 * n0, sched, r, 91 + n0), b"", proof[:-1], bytes(bad)]
    want = [1 if oracle.deep_fri_verify(p, sched, r, vb.SEED_Z) == 1 else 0 for p in batch]
    assert want[:2] == [1, 1] and 0 in want

    def check(got):
        assert got == want
    sweep(hostcheck, lambda: (0, vb.verify_batch(hostcheck, tparams, batch, sched, r)), check)


@pytest.mark.parametrize("mf", [0, 1])
def test_sumcheck_verify_batch(hostcheck, tparams, cparams, oracle, mf):
    items, want = sv.cases.mixed_batch(oracle, mf)
    proofs = [it[0] for it in items]; labels = [it[2] for it in items]

    def check(got):
        assert got == want
    sweep(hostcheck, lambda: (0, sv.verify_batch(hostcheck, tparams, cparams, mf, proofs, labels if mf else None)), check)


def test_mle_evaluate_batch(hostcheck, oracle):
    for k in (0, 1, 4, 7):
        tabs, pts = mle.tables_and_points(oracle, k, 3); want = mle.reference(oracle, tabs, k, pts)

        def check(got):
            assert (got == want).all(), k
        sweep(hostcheck, lambda: (0, mle.hc_evaluate(hostcheck, tabs, k, pts, 3)[0]), check)


@pytest.mark.parametrize("n", [1, 256, 1 << 12])
def test_lagrange_eval_batch(hostcheck, oracle, n):
    """points outside H and inside it (the gather path), one pass and one pass per point"""
    cols = lc.columns(oracle, n, 3); ref = lc.matrix_reference(oracle, n)[:2, :3]
    inside = lc.inside_points(oracle, n)[:2]
    zs = np.concatenate([lc.points(oracle, n, 2)] + [z.reshape(1, 4) for z, _ in inside])
    want = np.concatenate([ref] + [np.stack([v[j] for v in cols]).reshape(1, 3, 4) for _, j in inside])

    def check(got):
        assert (got == want).all()
    for mp in (0, 1):
        sweep(hostcheck, lambda: lc.hc_eval_rc(hostcheck, cols, n, zs, max_partials=mp)[:2], check, True)


@pytest.mark.parametrize("part", [1, 5], ids=[ls.PARTITION_IDS[1], ls.PARTITION_IDS[5]])
def test_lagrange_eval_shard_and_from_partials(hostcheck, oracle, part):
    n, blocks = ls.PARTITIONS[part]
    cols = lc.columns(oracle, n, 3); zs, _ = ls.mixed_points(oracle, n, blocks); want = ls.reference(oracle, n, blocks)
    clean = [ls.hc_shard(hostcheck, ls.block_rows(cols, j0, nl), nl, j0, n, zs)[0] for j0, nl in blocks]
    for q, (j0, nl) in enumerate(blocks):
        rows = ls.block_rows(cols, j0, nl)

        def check(got):
            assert (got == clean[q]).all(), q
        sweep(hostcheck, lambda: ls.hc_shard_rc(hostcheck, rows, nl, j0, n, zs)[:2], check, True)
    shares = np.stack(clean)

    def check_sum(got):
        assert (got == want).all()                                          # the shares (each equal to its unarmed run) sum to the oracle's values
    sweep(hostcheck, lambda: ls.hc_from_partials_rc(hostcheck, shares, 3, n, zs), check_sum, True)


def test_tr_batch(hostcheck, tparams):
    """one launch of the transcript stream of test_sumcheck_batch_host.py: four instances from Transcript::new, two ragged segments each"""
    import random
    import pyref
    rng = random.Random(5); p = pyref.P_PALLAS
    v0 = [rng.randrange(p) for _ in range(60)]; v1 = [rng.randrange(p) for _ in range(20)]
    pool0 = np.array([pyref.to_limbs(x) for x in v0], np.uint64); pool1 = np.array([pyref.to_limbs(x) for x in v1], np.uint64)
    K1 = 0x80000000; val = lambda i: v1[i & ~K1] if i & K1 else v0[i]
    segs = [[[rng.randrange(60) for _ in range([3, 16, 17, 37][b])] + [K1 | rng.randrange(20) for _ in range(b)], [rng.randrange(60) for _ in range([0, 5, 16, 2][b])]] for b in range(4)]
    want = []
    for b in range(4):
        m = sb.Model(); row = []
        for s in range(2):
            m.absorb([val(i) for i in segs[b][s]]); row.append(m.finish())
        want.append(row)

    def run():
        state = np.zeros((17 * 4, 4), np.uint64); pos = np.zeros(4, np.uint32)
        return 0, sb.tr_launch(hostcheck, tparams, state, pos, segs, pool0, pool1, reset=1)

    def check(got):
        assert got == want
    sweep(hostcheck, run, check)
