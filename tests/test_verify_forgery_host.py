"""Forged proofs that break exactly one check each (tests/verify_forgery_cases.py) through the host-check build of the batched verifiers: the
sum-check plan (hc_sumcheck_verify_batch), the DEEP-FRI and Merkle plans (hc_deep_fri_verify_batch, hc_merkle_verify_batch) and the single entries
(hc_deep_fri_verify, hc_merkle_verify).  Before any verifier under test is asked, each forgery's premise is established on the CPU: a census of the
verifier's relations in Python integers lists exactly the one item the forgery aims at, and the oracle rejects the bytes.  Every decision must then
equal the oracle's, alone, among honest proofs, and at the first / 256th / 257th / last place of a batch of 300.  The GPU build of the same plans
is tested in tests/test_gpu_verify_forgery.py."""
import ctypes as C

import numpy as np
import pytest

import pyref
import verify_forgery_cases as vf
from test_merkle_batch_host import hc_verify
from test_sumcheck_verify_batch_host import verify_batch as sc_verify_batch
from test_verify_batch_host import verify_batch as fri_verify_batch

vp = C.c_void_p


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


def sc_verify_batch_slots(hostcheck, tparams, cparams, mf, proofs, labels, max_slots):
    """the batch cut into plans of at most max_slots pool slots, as the device driver cuts it"""
    n = len(proofs)
    bufs = [(C.c_uint8 * max(1, len(p))).from_buffer_copy(p or b"\0") for p in proofs]
    ptrs = (vp * n)(*[C.cast(b, vp) for b in bufs]); lens = (C.c_size_t * n)(*[len(p) for p in proofs])
    lab = np.ascontiguousarray(labels, dtype=np.uint64); acc = (C.c_int32 * n)(*([7] * n))
    assert hostcheck.l.hc_sumcheck_verify_batch_slots(tparams, cparams, mf, C.c_size_t(n), ptrs, lens, lab.ctypes.data_as(vp), C.c_size_t(max_slots), acc) == 0
    return [acc[i] == 1 for i in range(n)]


# ---- helpers: codec, channel, provers ---------------------------------------------------------------------------------------------------------
def test_codec_and_python_provers_reproduce_the_oracles_bytes(oracle):
    """parse -> encode is the identity on the oracle's honest proofs; the Python provers, with no deviation, give the oracle's bytes: prove_mf with the
    query indices derived from its own channel and with the indices parsed out of the oracle's proof, prove_plain through its channel"""
    for k, label, q in vf.MF_SHAPES:
        w = vf.witness(oracle, 300 + k, k); p = oracle.sumcheck_prove(1, k, label, vf.rows(w), q=q)
        P = pyref.parse_proof_mf(p)
        assert pyref.encode_proof_mf(P) == p and len(P["rounds"]) == k
        assert vf.prove_mf(oracle, k, label, q, w, [Rn["next_indices"] for Rn in P["rounds"]]) == p, k
        assert vf.prove_mf(oracle, k, label, q, w) == p, k
        for Rn in P["rounds"]:                                                               # both encodings of a Merkle proof round-trip
            for pr in (Rn["cur_proof"], Rn["next_proof"]):
                back = pyref.mproof_parse_canonical(pyref.mproof_canonical(pr)); del back["sib_off"]
                assert back == pr
    for k, label in vf.PLAIN_SHAPES:
        w = vf.witness(oracle, 400 + k, k); p = oracle.sumcheck_prove(0, k, label, vf.rows(w))
        assert pyref.encode_proof_plain(pyref.parse_proof_plain(p)) == p
        assert vf.prove_plain(oracle, k, label, w) == p, k


def test_deep_fri_decoder_locates_roots_and_siblings(oracle):
    """the decoded roots are the prover's, and the bytes at every recorded offset are the element the decoder returned"""
    for n0, sched, r in vf.DEEP_FRI_SHAPES:
        cols = oracle.rand_fr_columns(600 + n0, n0, 4)
        ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, sched, r, vf.SEED_Z); p = ref.bytes()
        P = pyref.parse_deep_fri_proof(p)
        assert len(P["roots"]) == ref.num_layers() == len(sched) + 1 and P["n0"] == n0 and len(P["queries"]) == r
        for l, off in enumerate(P["root_off"]):
            assert P["roots"][l] == pyref.from_limbs(ref.root(l)) == int.from_bytes(p[off:off + 32], "little")
        for pr in [P["final_proof"]] + [lb[n] for lb in P["layers"] for n in ("child_proof", "parent_proof")]:
            assert pyref.mproof_canonical(pr) == p[pr["span"][0]:pr["span"][1]]
            for lv, offs in enumerate(pr["sib_off"]):
                assert [int.from_bytes(p[o:o + 32], "little") for o in offs] == pr["siblings"][lv]
        ref.free()


# ---- the sum-check catalogue ------------------------------------------------------------------------------------------------------------------
def test_sumcheck_catalogue_conditions(oracle):
    cases = vf.checked_sumcheck_catalogue(oracle)
    accepted = sorted(c.name for c in cases if c.accept and not c.name.endswith("honest"))
    assert accepted == ["mf k=0 F8", "mf k=1 F7", "plain k=1 P5"]
    f8 = [c for c in cases if c.name == "mf k=0 F8"][0]; honest = [c for c in cases if c.name == "mf k=0 honest"][0]
    assert pyref.parse_proof_mf(f8.proof)["final_eval"] != pyref.parse_proof_mf(honest.proof)["final_eval"] and not pyref.parse_proof_mf(f8.proof)["rounds"]


@pytest.mark.parametrize("mf", [0, 1])
def test_sumcheck_forgeries_alone_and_among_honest_proofs(hostcheck, tparams, cparams, oracle, mf):
    cases = [c for c in vf.checked_sumcheck_catalogue(oracle) if c.mf == mf]
    want = [c.accept for c in cases]
    assert sum(want) == (6 if mf else 4) and len(cases) >= 30                                          # the honest proof of every shape, F7 / P5 (and F8)
    for c in cases:
        assert sc_verify_batch(hostcheck, tparams, cparams, mf, [c.proof], [c.label]) == [c.accept], c.name
    honest = [c for c in cases if c.name.endswith("honest")]
    batch = []
    for i, c in enumerate(cases):                                                             # every forgery between honest proofs of the shapes
        batch += [honest[i % len(honest)], c]
    batch.append(honest[0])
    got = sc_verify_batch(hostcheck, tparams, cparams, mf, [c.proof for c in batch], [c.label for c in batch])
    assert got == [c.accept for c in batch], [c.name for c, g in zip(batch, got) if g != c.accept]
    got = sc_verify_batch(hostcheck, tparams, cparams, mf, [c.proof for c in batch[::-1]], [c.label for c in batch[::-1]])
    assert got == [c.accept for c in batch[::-1]]


@pytest.mark.parametrize("pos", vf.POSITIONS)
@pytest.mark.parametrize("name", vf.POSITION_FORGERIES_PLAIN + vf.POSITION_FORGERIES_MF[:2])
def test_sumcheck_forgery_at_each_place_of_a_batch_of_300(hostcheck, tparams, cparams, oracle, name, pos):
    """one forgery among 300 honest k = 2 proofs at index 0, 255, 256 and 299, forward and reversed, in one plan and with a plan boundary directly
    before and after every item (max_slots = 1: one proof per plan)"""
    mf = int(name.startswith("mf"))
    honest, forged, label, q = vf.sumcheck_position_set(oracle, mf); c = forged[name]
    assert all(oracle.sumcheck_verify(mf, 2, label, p, q=q or 2) == 1 for p in honest)
    assert vf.census_of(c) == c.census and len(c.census) == 1 and not vf.oracle_decision(oracle, c) and c.label == label
    items = vf.position_batch(honest, c.proof, pos); want = [i != pos for i in range(300)]; labels = [label] * 300
    assert len(items) == 300
    assert sc_verify_batch(hostcheck, tparams, cparams, mf, items, labels) == want
    assert sc_verify_batch(hostcheck, tparams, cparams, mf, items[::-1], labels) == want[::-1]
    assert sc_verify_batch_slots(hostcheck, tparams, cparams, mf, items, labels, 1) == want


def test_sumcheck_plan_cut_matches_one_plan_on_the_catalogue(hostcheck, tparams, cparams, oracle):
    """the whole catalogue in plans of a few proofs each and of one proof each"""
    for mf in (0, 1):
        cases = [c for c in vf.sumcheck_catalogue(oracle) if c.mf == mf]
        for slots in (1, 64, 1000):
            got = sc_verify_batch_slots(hostcheck, tparams, cparams, mf, [c.proof for c in cases], [c.label for c in cases], slots)
            assert got == [c.accept for c in cases], (mf, slots)


# ---- DEEP-FRI ---------------------------------------------------------------------------------------------------------------------------------
def test_deep_fri_catalogue_conditions(oracle):
    """D1(l) fails exactly the openings against roots[l], D2 exactly the opening whose sibling changed; the oracle rejects both kinds"""
    vf.checked_deep_fri_catalogue(oracle)


@pytest.mark.parametrize("n0,sched,r", vf.DEEP_FRI_SHAPES)
def test_deep_fri_forgeries(oracle, hostcheck, tparams, n0, sched, r):
    cases = vf.checked_deep_fri_catalogue(oracle)[(n0, tuple(sched), r)]
    want = [int(name == "honest") for name, _, _ in cases]
    assert [hostcheck.deep_fri_verify(tparams, p, sched, r) for _, p, _ in cases] == want
    honest = cases[0][1]; batch = []; bwant = []
    for (_, p, _), w in zip(cases, want):
        batch += [honest, p]; bwant += [1, w]
    assert fri_verify_batch(hostcheck, tparams, batch, sched, r) == bwant
    assert fri_verify_batch(hostcheck, tparams, batch[::-1], sched, r) == bwant[::-1]


@pytest.mark.parametrize("name", vf.DEEP_FRI_POSITION_FORGERIES)
def test_deep_fri_forgery_at_each_place_of_a_batch_of_300(oracle, hostcheck, tparams, name):
    n0, sched, r = vf.DEEP_FRI_SHAPES[2]
    honest, forged = vf.deep_fri_position_set(oracle)
    for pos in vf.POSITIONS:
        items = vf.position_batch(honest, forged[name], pos); want = [int(i != pos) for i in range(300)]
        assert fri_verify_batch(hostcheck, tparams, items, sched, r) == want, pos
        assert fri_verify_batch(hostcheck, tparams, items[::-1], sched, r) == want[::-1], pos


# ---- Merkle -----------------------------------------------------------------------------------------------------------------------------------
def test_merkle_forgeries(oracle, hostcheck):
    cases = vf.merkle_catalogue(oracle)
    want = [int(vf.merkle_oracle_decision(c)) for c in cases]
    assert want == [int(c.name.endswith("honest")) for c in cases] and sum(want) == 3 and len(cases) == 3 + (3 + 2 + 2) + 3 * 8
    single = [hostcheck.merkle_verify(None, c.cp is not None, c.arity, c.label, c.root, c.idx, c.values, c.cp, c.proof) for c in cases]
    assert single == want, [c.name for c, s, w in zip(cases, single, want) if s != w]
    for arity in (16, 8):                                                                     # verify_many_ds of every item of one cfg_arity in one plan, and one plan per item
        sub = [(c, w) for c, w in zip(cases, want) if c.arity == arity and c.cp is None]
        items = [(c.label, c.root, c.idx, c.values, c.proof) for c, _ in sub]
        assert len(items) >= 11
        assert hc_verify(hostcheck, arity, items) == [w for _, w in sub]
        assert hc_verify(hostcheck, arity, items[::-1]) == [w for _, w in sub][::-1]
        assert hc_verify(hostcheck, arity, items, max_slots=1) == [w for _, w in sub]


def test_commitment_openings_taken_out_of_the_sumcheck_proofs(oracle):
    """the openings the GPU test puts to stark_commitment_verify: taken out of their ProofMF, re-encoded in the canonical form, the oracle's
    verify_many_ds under MerkleCommitment's parameters accepts the four honest ones and rejects every F5 sibling and every root word"""
    opens = vf.commitment_openings(oracle)
    assert sum(it[-1] for it in opens) == 4 and len(opens) == 16 and len({it[0] for it in opens}) == 16


@pytest.mark.parametrize("name", vf.MERKLE_POSITION_FORGERIES)
def test_merkle_forgery_at_each_place_of_a_batch_of_300(oracle, hostcheck, name):
    honest, forged = vf.merkle_position_set(oracle); bad = forged[name]
    for pos in vf.POSITIONS:
        items = vf.position_batch(honest, bad, pos); want = [int(i != pos) for i in range(300)]
        assert hc_verify(hostcheck, 2, items) == want, pos
        assert hc_verify(hostcheck, 2, items[::-1]) == want[::-1], pos
