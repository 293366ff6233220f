"""Forged proofs that break exactly one check each (tests/verify_forgery_cases.py) through the C-ABI on the GPU: the batch entries
(stark_sumcheck_verify_plain_batch / _mf_batch, stark_deep_fri_verify_batch, stark_merkle_verify_many_ds_batch) and the single ones, which plan a batch
of one (stark_sumcheck_verify_plain / _mf, stark_deep_fri_verify, stark_merkle_verify_many_ds / _pairs_ds, stark_commitment_verify).  Each forgery's
premise is asserted on the CPU first (the census lists exactly the aimed relation, the oracle rejects); every decision must then equal the oracle's:
alone, among honest proofs, under the forced kernel forms, and at index 0 / 255 / 256 / 299 of a batch of 300 (the check kernels run one lane per
record or item in blocks of 256).  The host-check build of the same plans is tested in tests/test_verify_forgery_host.py.  Needs an MI355X: `pytest -m gpu`."""
import pytest

pytestmark = pytest.mark.gpu

import verify_forgery_cases as vf
from stark_mlwe_amd.api import Context, DeepFriParams


def sc_batch(ctx, mf, cases):
    proofs = [c.proof for c in cases]
    if mf:
        return ctx.verify_mf_batch(cases[0].k, [c.label for c in cases], cases[0].q, proofs)      # verify_mf reads neither k nor q
    return ctx.verify_plain_batch(cases[0].k, None, proofs)


def sc_single(ctx, c):
    return ctx.verify_mf(c.k, c.label, c.q, c.proof) if c.mf else ctx.verify_plain(c.k, c.label, c.proof)


def among_honest(cases):
    """every case between honest proofs of the shapes"""
    honest = [c for c in cases if c.name.endswith("honest")]; batch = []
    for i, c in enumerate(cases):
        batch += [honest[i % len(honest)], c]
    return batch + [honest[0]]


def merkle_batch(ctx, arity, items):
    return ctx.merkle_verify_single_batch(arity, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items], [it[3] for it in items], [it[4] for it in items])


@pytest.fixture(scope="module")
def one_proof_per_plan():
    """a context whose sum-check verify plans hold one proof each: a plan boundary directly before and directly after every item"""
    c = Context(0)
    c.set_option("sumcheck_verify_batch_max_slots", 1)
    yield c
    c.close()


# ---- sum-check --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mf", [0, 1])
def test_gpu_sumcheck_forgeries_alone_and_among_honest_proofs(gpu_ctx, oracle, mf):
    cases = [c for c in vf.checked_sumcheck_catalogue(oracle) if c.mf == mf]
    assert sum(c.accept for c in cases) == (6 if mf else 4) and len(cases) >= 30               # the honest proof of every shape, F7 / P5 (and F8)
    got = [sc_single(gpu_ctx, c) for c in cases]
    assert got == [c.accept for c in cases], [c.name for c, g in zip(cases, got) if g != c.accept]
    got = sc_batch(gpu_ctx, mf, cases)
    assert got == [c.accept for c in cases], [c.name for c, g in zip(cases, got) if g != c.accept]
    batch = among_honest(cases)
    got = sc_batch(gpu_ctx, mf, batch)
    assert got == [c.accept for c in batch], [c.name for c, g in zip(batch, got) if g != c.accept]
    assert sc_batch(gpu_ctx, mf, batch[::-1]) == [c.accept for c in batch[::-1]]


@pytest.mark.parametrize("name", vf.POSITION_FORGERIES_PLAIN + vf.POSITION_FORGERIES_MF)
def test_gpu_sumcheck_forgery_at_each_place_of_a_batch_of_300(gpu_ctx, one_proof_per_plan, oracle, name):
    mf = int(name.startswith("mf"))
    honest, forged, label, q = vf.sumcheck_position_set(oracle, mf); c = forged[name]
    assert all(oracle.sumcheck_verify(mf, 2, label, p, q=q or 2) == 1 for p in honest)
    assert vf.census_of(c) == c.census and len(c.census) == 1 and not vf.oracle_decision(oracle, c) and c.label == label

    def call(ctx, items):
        return ctx.verify_mf_batch(2, [label] * len(items), q, items) if mf else ctx.verify_plain_batch(2, None, items)
    for pos in vf.POSITIONS:
        items = vf.position_batch(honest, c.proof, pos); want = [i != pos for i in range(300)]
        assert len(items) == 300
        assert call(gpu_ctx, items) == want, pos
        assert call(gpu_ctx, items[::-1]) == want[::-1], pos
        assert call(one_proof_per_plan, items) == want, pos


# ---- DEEP-FRI ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,sched,r", vf.DEEP_FRI_SHAPES)
def test_gpu_deep_fri_forgeries(gpu_ctx, oracle, n0, sched, r):
    cases = vf.checked_deep_fri_catalogue(oracle)[(n0, tuple(sched), r)]; prm = DeepFriParams(sched, r, vf.SEED_Z)
    want = [name == "honest" for name, _, _ in cases]
    got = [gpu_ctx.deep_fri_verify(prm, p) for _, p, _ in cases]
    assert got == want, [c[0] for c, g, w in zip(cases, got, want) if g != w]
    honest = cases[0][1]; batch = []; bwant = []
    for (_, p, _), w in zip(cases, want):
        batch += [honest, p]; bwant += [True, w]
    assert gpu_ctx.deep_fri_verify_batch(prm, batch) == bwant
    assert gpu_ctx.deep_fri_verify_batch(prm, batch[::-1]) == bwant[::-1]


@pytest.mark.parametrize("name", vf.DEEP_FRI_POSITION_FORGERIES)
def test_gpu_deep_fri_forgery_at_each_place_of_a_batch_of_300(gpu_ctx, oracle, name):
    n0, sched, r = vf.DEEP_FRI_SHAPES[2]; prm = DeepFriParams(sched, r, vf.SEED_Z)
    honest, forged = vf.deep_fri_position_set(oracle)
    for pos in vf.POSITIONS:
        items = vf.position_batch(honest, forged[name], pos); want = [i != pos for i in range(300)]
        assert gpu_ctx.deep_fri_verify_batch(prm, items) == want, pos
        assert gpu_ctx.deep_fri_verify_batch(prm, items[::-1]) == want[::-1], pos


# ---- Merkle -----------------------------------------------------------------------------------------------------------------------------------
def merkle_single(ctx, c):
    cfg = ctx.merkle_cfg(c.arity).with_tree_label(c.label)
    if c.cp is None:
        return ctx.merkle_verify_single(cfg, c.root, c.idx, c.values, c.proof)
    return ctx.merkle_verify_pairs(cfg, c.root, c.idx, c.values, c.cp, c.proof)


def test_gpu_merkle_forgeries(gpu_ctx, oracle):
    """M1-M3 through stark_merkle_verify_many_ds, _pairs_ds and _many_ds_batch; the openings of the sum-check proofs through stark_commitment_verify"""
    cases = vf.merkle_catalogue(oracle)
    want = [vf.merkle_oracle_decision(c) for c in cases]
    assert want == [c.name.endswith("honest") for c in cases] and sum(want) == 3 and any(c.cp is not None for c in cases)
    got = [merkle_single(gpu_ctx, c) for c in cases]
    assert got == want, [c.name for c, g, w in zip(cases, got, want) if g != w]
    for arity in (16, 8):
        sub = [(c, w) for c, w in zip(cases, want) if c.arity == arity and c.cp is None]
        items = [(c.label, c.root, c.idx, c.values, c.proof) for c, _ in sub]
        assert len(items) >= 11
        assert merkle_batch(gpu_ctx, arity, items) == [w for _, w in sub]
        assert merkle_batch(gpu_ctx, arity, items[::-1]) == [w for _, w in sub][::-1]
    opens = vf.commitment_openings(oracle)
    assert sum(it[-1] for it in opens) == 4 and len(opens) == 16
    got = [gpu_ctx.commitment_verify(label, root, idx, vals, proof) for _, label, root, idx, vals, proof, _ in opens]
    assert got == [it[-1] for it in opens], [it[0] for it, g in zip(opens, got) if g != it[-1]]


@pytest.mark.parametrize("name", vf.MERKLE_POSITION_FORGERIES)
def test_gpu_merkle_forgery_at_each_place_of_a_batch_of_300(gpu_ctx, oracle, name):
    honest, forged = vf.merkle_position_set(oracle)
    for pos in vf.POSITIONS:
        items = vf.position_batch(honest, forged[name], pos); want = [i != pos for i in range(300)]
        assert merkle_batch(gpu_ctx, 2, items) == want, pos
        assert merkle_batch(gpu_ctx, 2, items[::-1]) == want[::-1], pos


# ---- the forced kernel forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", ["poseidon_lane_only", "sponge_one_wave"])
def test_gpu_catalogue_batches_under_forced_forms(oracle, option):
    sc = vf.checked_sumcheck_catalogue(oracle); fri = vf.checked_deep_fri_catalogue(oracle); merkle = vf.merkle_catalogue(oracle)
    mwant = [vf.merkle_oracle_decision(c) for c in merkle]
    c = Context(0)                                                            # a fresh context: the session's options stay as they are
    try:
        c.set_option(option, 1)
        for mf in (0, 1):
            batch = among_honest([x for x in sc if x.mf == mf])
            got = sc_batch(c, mf, batch)
            assert got == [x.accept for x in batch], [x.name for x, g in zip(batch, got) if g != x.accept]
        for (n0, sched, r), cases in fri.items():
            assert c.deep_fri_verify_batch(DeepFriParams(list(sched), r, vf.SEED_Z), [p for _, p, _ in cases]) == [name == "honest" for name, _, _ in cases], n0
        for arity in (16, 8):
            sub = [(x, w) for x, w in zip(merkle, mwant) if x.arity == arity and x.cp is None]
            assert merkle_batch(c, arity, [(x.label, x.root, x.idx, x.values, x.proof) for x, _ in sub]) == [w for _, w in sub]
    finally:
        c.close()
