"""What the shared drivers read from their own temporaries, on the CPU.  The host executors of csrc/hostcheck.cpp hand out zeroed blocks by default, so a
driver (sumcheck_batch.hpp, sumcheck_verify_batch.hpp, fri_verify_batch.hpp, merkle_batch.hpp, fri_batch.hpp, the pass loop of mle_dev.hpp) that reads a
pool slot before anything fills it reads 0 here and whatever the recycled block held on the device.  hc_set_alloc_fill makes every such block hold a
byte of the test's choice: each case below runs under 0x5A (the byte of the project's SENTINEL; as limbs a non-zero stored element above the Pallas
modulus) and under 0x00, and every result must be the oracle's, byte for byte, under both.  The device allocator has the same knob (context option
"pool_poison", tests/test_gpu_pool_poison.py)."""
import contextlib

import numpy as np
import pytest

import merkle_batch_cases as mc
import mle_cases as mle
import test_fri_batch_host as fb
import test_merkle_batch_host as mb
import test_sumcheck_batch_host as sb
import test_sumcheck_verify_batch_host as sv
import test_verify_batch_host as vb

FILLS = [0x5A, 0x00]
SEED_Z = vb.SEED_Z


@contextlib.contextmanager
def alloc_fill(hostcheck, byte):
    hostcheck.set_alloc_fill(byte)
    try:
        yield
    finally:
        hostcheck.set_alloc_fill(0)


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


hc_params = mb.hc_params


def test_the_fill_reaches_the_blocks(hostcheck):
    """the helper can fail: a probe block holds the byte that was set, and zeros again once 0 is restored"""
    for nbytes in (1, 32, 4096 + 5):
        with alloc_fill(hostcheck, 0x5A):
            assert hostcheck.alloc_probe(nbytes) == b"\x5a" * nbytes
        assert hostcheck.alloc_probe(nbytes) == bytes(nbytes)
    assert hostcheck.l.hc_set_alloc_fill(256) == -1 and hostcheck.l.hc_set_alloc_fill(-1) == -1
    assert hostcheck.alloc_probe(8) == bytes(8)


# ---- batched sum-check prove ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sumcheck_witnesses(oracle):
    """k -> five witnesses of 2^k elements and their labels (shared by the plain and mf cases and left unchanged)"""
    return {k: (oracle.rand_fr_columns(0x900 + k, 1 << k, 5), [2025, 7, 2025, 11, 6060]) for k in (0, 1, 5)}


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("k", [0, 1, 5])
def test_sumcheck_prove_plain(hostcheck, tparams, cparams, oracle, sumcheck_witnesses, k, B):
    ws, labels = sumcheck_witnesses[k]
    want = [oracle.sumcheck_prove(0, k, labels[b], ws[b]) for b in range(B)]
    for fill in FILLS:
        with alloc_fill(hostcheck, fill):
            got = sb.prove_batch(hostcheck, tparams, cparams, 0, k, labels[:B], ws[:B])
        assert got == want, "fill 0x%02X: proofs %s differ from the oracle's" % (fill, [b for b in range(B) if got[b] != want[b]])


@pytest.mark.parametrize("q", [2, 8])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("k", [0, 1, 5])
def test_sumcheck_prove_mf(hostcheck, tparams, cparams, oracle, sumcheck_witnesses, k, B, q):
    ws, labels = sumcheck_witnesses[k]
    want = [oracle.sumcheck_prove(1, k, labels[b], ws[b], q=q) for b in range(B)]
    for fill in FILLS:
        with alloc_fill(hostcheck, fill):
            got = sb.prove_batch(hostcheck, tparams, cparams, 1, k, labels[:B], ws[:B], q)
        assert got == want, "fill 0x%02X: proofs %s differ from the oracle's" % (fill, [b for b in range(B) if got[b] != want[b]])


# ---- batched sum-check verify -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mf", [0, 1])
def test_sumcheck_verify(hostcheck, tparams, cparams, oracle, mf):
    """the mixed batch of sumcheck_verify_cases: honest proofs of every shape, truncations and one flipped bit in each of 57 bytes"""
    items, want = sv.cases.mixed_batch(oracle, mf)
    proofs = [it[0] for it in items]; labels = [it[2] for it in items]
    assert any(want) and not all(want)
    for fill in FILLS:
        with alloc_fill(hostcheck, fill):
            got = sv.verify_batch(hostcheck, tparams, cparams, mf, proofs, labels if mf else None)
            one = [sv.verify_batch(hostcheck, tparams, cparams, mf, [proofs[i]], [labels[i]])[0] for i in (0, 1, 10)]
        assert got == want, "fill 0x%02X: decisions %s differ from the oracle's" % (fill, [i for i in range(len(want)) if got[i] != want[i]])
        assert one == [want[i] for i in (0, 1, 10)], "fill 0x%02X: batches of one" % fill


# ---- DEEP-FRI verify, batched and single ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,sched,r", [(2, [2], 1), (1 << 9, [8, 4, 2], 5), (64, [8, 8], 4)])
def test_deep_fri_verify(hostcheck, tparams, oracle, n0, sched, r):
    proof = vb.make_proof(oracle, n0, sched, r, 77 + n0)
    batch = [proof, vb.make_proof(oracle, 2 * n0, sched, r, 91 + n0), b"", proof[:-1], proof[: len(proof) // 2]]
    for pos in (0, 8, 8 + 31, len(proof) // 3, len(proof) // 2, len(proof) - 41, len(proof) - 33, len(proof) - 1):
        bad = bytearray(proof); bad[pos] ^= 1 << (pos % 8); batch.append(bytes(bad))
    want = [1 if oracle.deep_fri_verify(p, sched, r, SEED_Z) == 1 else 0 for p in batch]
    assert want[:2] == [1, 1] and 0 in want
    for fill in FILLS:
        with alloc_fill(hostcheck, fill):
            got = vb.verify_batch(hostcheck, tparams, batch, sched, r)
            single = [hostcheck.deep_fri_verify(tparams, p, sched, r) for p in batch]
        assert got == want, "fill 0x%02X, batch: %s" % (fill, [i for i in range(len(want)) if got[i] != want[i]])
        assert single == want, "fill 0x%02X, single: %s" % (fill, [i for i in range(len(want)) if single[i] != want[i]])


# ---- batched Merkle build, open and verify ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("arity,n", [(16, 257), (4, 64), (2, 5), (16, 17)])
def test_merkle_build_open_verify(hostcheck, hc_params, oracle, arity, n, pairs):
    """B = 3 and a batch of one.  The build executor's level blocks never hold zeros: under fill 0x00 they keep the stale pattern they have always had
    (0xA5), so for them the two fills are two different non-zero patterns; the verify pools and the tables follow the fill exactly."""
    B = 3
    labels, cols, cps, want = mb.batch_inputs(oracle, arity, n, pairs, B)
    ixs = [mc.index_lists(n, b) for b in range(B)]
    want_proofs = [want[b].open_bytes(ixs[b]) for b in range(B)]
    zeros = np.zeros((n, 4), np.uint64)
    for fill in FILLS:
        with alloc_fill(hostcheck, fill):
            lens, trees = mb.hc_build(hostcheck, hc_params(arity), arity, labels, cols, n, cps)
            proofs = mb.hc_open(hostcheck, [arity] * B, trees, ixs)
            one = mb.hc_build(hostcheck, hc_params(arity), arity, labels[:1], cols[:1], n, None if cps is None else cps[:1])[1][0]
        for b in range(B):
            assert len(trees[b]) == want[b].num_levels()
            for v in range(len(lens)):
                assert (trees[b][v] == want[b].level(v)).all(), "fill 0x%02X: tree %d, level %d" % (fill, b, v)
        assert all((one[v] == want[0].level(v)).all() for v in range(len(lens))), "fill 0x%02X: a batch of one" % fill
        assert proofs == want_proofs, "fill 0x%02X: openings" % fill
        # verify: the opened values of level 0 under verify_many_ds (the batch entry point and the single one); a pair tree's (f, cp) under verify_pairs_ds
        items, expect = [], []
        for b in range(B):
            vals = trees[b][0][ixs[b]]; root = trees[b][-1][0]
            for name, lab, rt, ix, v, pr in mc.tamperings(labels[b], root, ixs[b], vals, proofs[b], n):
                items.append((lab, rt, ix, v, pr)); expect.append(mc.oracle_verify(arity, lab, rt, ix, v, pr))
        assert 1 in expect and 0 in expect
        with alloc_fill(hostcheck, fill):
            got = mb.hc_verify(hostcheck, arity, items)
            cut = mb.hc_verify(hostcheck, arity, items, max_slots=1)
            single = [hostcheck.merkle_verify(None, False, arity, lab, rt, ix, v, None, pr) for lab, rt, ix, v, pr in items[:7]]
        assert got == expect and cut == expect, "fill 0x%02X: verify_many_ds batch" % fill
        assert single == expect[:7], "fill 0x%02X: verify_many_ds single" % fill
        if pairs:
            for b in range(B):
                f = cols[b][ixs[b]]; cp = (zeros if cps[b] is None else cps[b])[ixs[b]]; root = trees[b][-1][0]
                bad = mc.flip_bit(cp, 4 * (len(ixs[b]) - 1) + 2, 3)
                for c in (cp, bad):
                    w = mc.oracle_verify_pairs(arity, labels[b], root, ixs[b], f, c, proofs[b])
                    with alloc_fill(hostcheck, fill):
                        g = hostcheck.merkle_verify(None, True, arity, labels[b], root, ixs[b], f, c, proofs[b])
                    assert g == w, "fill 0x%02X: verify_pairs_ds, tree %d" % (fill, b)
                assert mc.oracle_verify_pairs(arity, labels[b], root, ixs[b], f, cp, proofs[b]) == 1


# ---- batched FRI commit -----------------------------------------------------------------------------------------------------------------------
_fri_refs = {}


def _fri_reference(oracle, shape):
    """the inputs and oracle roots of tests/test_fri_batch_host.py's `references`, one shape at a time, computed once"""
    if shape not in _fri_refs:
        k, sched, r = fb.SHAPES[shape]; n0 = 1 << k
        f0s = oracle.rand_fr_columns(0xF0 + shape, n0, 5)
        want = np.zeros((5, len(sched) + 1, 4), np.uint64)
        for b in range(5):
            pr = oracle.deep_fri_prove(None, None, None, None, n0, sched, r, 0xDEEFBAAD + shape, f0=f0s[b])
            for l in range(len(sched) + 1):
                want[b, l] = pr.root(l)
            pr.free()
        _fri_refs[shape] = (f0s, want)
    return _fri_refs[shape]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("shape", range(len(fb.SHAPES)))
def test_fri_commit(hostcheck, tparams, oracle, shape, B):
    """FriBatchCommit is the commit phase of the batched commit, f0 and prove entry points alike; the host check runs it through hc_fri_commit_batch.
    The [128] shape derives the t = 129 constants once per process (minutes on the host), as tests/test_fri_batch_host.py does."""
    k, sched, _ = fb.SHAPES[shape]
    f0s, want = _fri_reference(oracle, shape)
    for fill in FILLS:
        with alloc_fill(hostcheck, fill):
            got = fb.commit_batch(hostcheck, tparams, f0s[:B], 1 << k, sched, 0xDEEFBAAD + shape)
        for b in range(B):
            assert (got[b] == want[b]).all(), "fill 0x%02X: trace %d" % (fill, b)


# ---- batched MLE (the pooled intermediate layers of the pass loop) and the pass cutting of the batched LDE -------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_mle_passes(hostcheck, oracle, B):
    for k in mle.K_MATRIX:
        tabs, pts = mle.tables_and_points(oracle, k, B); want = mle.reference(oracle, tabs, k, pts)
        for fill in FILLS:
            with alloc_fill(hostcheck, fill):
                got, _ = mle.hc_evaluate(hostcheck, tabs, k, pts, 3)
                dflt, _ = mle.hc_evaluate(hostcheck, tabs, k, pts)
            assert (got == want).all() and (dflt == want).all(), "fill 0x%02X: k = %d" % (fill, k)


def test_lde_pass_cutting_allocates_nothing(hostcheck):
    """the host part of the batched NTT / LDE is the pass cutting and the launch plan (ntt_mixed_plan.hpp), neither of which takes a pooled block: the same passes under both fills; the scratch vector it
    sizes is the device's (ctx_scratch), filled there by "pool_poison\""""
    import test_lde_batch_host as lb
    for fill in FILLS:
        with alloc_fill(hostcheck, fill):
            assert lb.passes_lib(hostcheck.l, 5, 11, 2 << 11) == lb.passes_ref(5, 11, 2 << 11) == [2, 2, 1]
            assert lb.passes_lib(hostcheck.l, 3, 3, 1 << 24) == [3]
