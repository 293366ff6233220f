"""queued_cases.py on the CPU: the helpers of the queued-call tests can fail, and the references of Q1 - Q4 are consistent with a second derivation
that does not go through the code that built them — so a wrong case file cannot pass for a library bug on the GPU (test_gpu_queued_calls.py)."""
import ctypes as C

import numpy as np
import pytest

import lagrange_cases as lc
import pyref
import queued_cases as qc


# ---- the helpers can fail -----------------------------------------------------------------------------------------------------------------------
def test_clobber_changes_every_kind_of_argument():
    a = np.arange(12, dtype=np.uint64).reshape(3, 4); z = np.zeros(4, np.uint64); lab = np.array([7, 8, 9], np.uint64)
    tab = qc.table([0x1000, qc.vp(0x2000), None]); ks = (C.c_size_t * 3)(0, 1, 17)
    tag = C.create_string_buffer(b"FRI/index"); tags = qc.table([C.addressof(tag)]); cp = (C.c_char_p * 2)(b"a", b"b")
    assert [tab[i] for i in range(3)] == [0x1000, 0x2000, None] and tags[0] == C.addressof(tag)
    qc.clobber(a, z, lab, None, tab, ks, tag, tags, cp)
    for x in (a, z, lab):
        assert (x == 0xFFFFFFFFFFFFFFFF).all()
    assert [tab[i] for i in range(3)] == [None] * 3 and tags[0] is None and cp[0] is None and cp[1] is None
    assert [ks[i] for i in range(3)] == [2 ** 64 - 1] * 3
    assert tag.value == b"?" and tag.raw == b"?" + b"\0" * 9
    view = np.arange(16, dtype=np.uint64).reshape(4, 4)
    qc.clobber(view[1:3])                                                  # a contiguous slice: only its rows change
    assert (view[1:3] == 0xFFFFFFFFFFFFFFFF).all() and (view[0] == np.arange(4)).all() and (view[3] == np.arange(12, 16)).all()
    for bad in (b"bytes", [1, 2], 5):
        with pytest.raises(TypeError):
            qc.clobber(bad)
    with pytest.raises(AssertionError):
        qc.clobber(view[:, 1])                                             # not contiguous: it cannot have been a C argument


def test_three_way_names_the_first_differing_call_and_row():
    ref = [("first call", np.arange(40, dtype=np.uint64).reshape(10, 4)), ("second call", np.arange(8, dtype=np.uint64).reshape(2, 4))]
    copy = lambda: [(c, np.array(r)) for c, r in ref]
    qc.three_way(copy(), copy(), ref, "case")
    assert qc.first_difference(copy(), ref) is None
    bad = copy(); bad[1][1][1, 3] ^= 1; bad[1][1][0, 0] ^= 1
    assert qc.first_difference(bad, ref) == ("second call", 0)
    with pytest.raises(AssertionError) as e:
        qc.three_way(copy(), bad, ref, "case")
    assert "case, the queued run differs from the reference: second call, 2 of 2 rows differ, first at row 0" in str(e.value), str(e.value)
    bad = copy(); bad[0][1][7, 2] = 0; bad[1][1][0, 0] ^= 1                 # the first call in issue order is named, not the later one
    with pytest.raises(AssertionError) as e:
        qc.three_way(bad, copy(), ref, "case")
    assert "the synchronised run differs from the reference: first call, 1 of 10 rows differ, first at row 7" in str(e.value), str(e.value)
    short = copy(); short[0] = ("first call", short[0][1][:9])
    assert qc.first_difference(short, ref) == ("first call", None)
    with pytest.raises(AssertionError) as e:
        qc.three_way(copy(), short, ref, "case")
    assert "first call, another shape" in str(e.value)
    assert qc.first_difference(copy()[:1], ref) == ("the list of calls", None)


class StubEvent:
    def __init__(self, *answers): self.answers = list(answers)
    def query(self): return self.answers.pop(0) if len(self.answers) > 1 else self.answers[0]


class StubBlocker(qc.Blocker):
    def __init__(self, *answers): super().__init__(None, None); self.event = StubEvent(*answers)
    def ms(self): return 100.0


class StubCtx:
    def __init__(self): self.syncs, self.checked = 0, []
    def sync(self): self.syncs += 1
    def _chk(self, rc): self.checked.append(rc)


def test_still_busy_and_the_busy_condition_with_a_stub_event():
    assert StubBlocker(False).still_busy() and not StubBlocker(True).still_busy()
    # a sync run brackets every call and notes nothing
    c = StubCtx(); r = qc.Run(c, None, "sync"); z = np.ones(4, np.uint64)
    r.t0 = 0.0; r.call("stark_ntt_dev", lambda: 0, z)
    assert c.syncs == 2 and c.checked == [0] and (z == 0xFFFFFFFFFFFFFFFF).all() and r.table == {} and r.waited is None
    r.end(); r.require_busy("sync")                                        # nothing to require
    # a queued run: the event completes during the third call; a call that is not promised does not count as having waited
    r = qc.Run(StubCtx(), None, "queued"); r.blocker = StubBlocker(False, False, True, True); r.t0 = 0.0
    r.call("stark_lde_batch_dev", lambda: 0)
    r.call("stark_ali_merge_dev", lambda: 0)
    r.call("stark_fri_build_dev", lambda: 0)
    assert r.waited is None and r.table == {"stark_lde_batch_dev": True, "stark_ali_merge_dev": True, "stark_fri_build_dev": False}
    r.call("stark_merkle_free", lambda: 0); r.call("stark_lde_batch_dev", lambda: 0); r.end()
    assert r.waited[:2] == ("stark_merkle_free", 4) and r.table["stark_lde_batch_dev"] is False and r.ctx.syncs == 0 and r.busy_at_end is False
    with pytest.raises(AssertionError) as e:
        r.require_busy("case")
    assert "case: stark_merkle_free (call 4 of the section) returned only after the stream had drained" in str(e.value), str(e.value)
    # busy throughout, but not at the end: the blocker was too short
    r = qc.Run(StubCtx(), None, "queued"); r.blocker = StubBlocker(False, True); r.t0 = 0.0
    r.call("stark_ntt_dev", lambda: 0); r.end()
    with pytest.raises(AssertionError) as e:
        r.require_busy("case")
    assert "the blocker (100.0 ms) had finished before the last queued call returned" in str(e.value)
    r = qc.Run(StubCtx(), None, "queued"); r.blocker = StubBlocker(False); r.t0 = 0.0
    r.call("stark_ntt_dev", lambda: 0); r.end(); r.require_busy("case")
    n = len(qc.RECORDS); r.record("case", "stub")
    assert len(qc.RECORDS) == n + 1
    assert qc.RECORDS.pop() == dict(pipeline="case", context="stub", K=qc.BLOCKER_K, calls=1, enqueue_ms=round(r.enqueue_ms, 3), blocker_ms=100.0, busy_at_end=True,
                                    first_promised_call_that_waited=None, returns_while_busy={"stark_ntt_dev": True})


def test_every_promised_entry_point_is_exercised_by_a_pipeline_that_asserts_it():
    import inspect
    src = "".join(inspect.getsource(f) for f in (qc.q1, qc.q2, qc.q3, qc.hash_many, qc.free_trees))
    for name in qc.PROMISED:
        assert 'run.call("%s"' % name in src, name


# ---- the references are self-consistent ---------------------------------------------------------------------------------------------------------
def ints(a):
    return [pyref.from_limbs(r) for r in qc.rows(a)]


def test_q3_digests_against_pyref(oracle):
    pool = qc.q3_pool(oracle); want = qc.q3_refs(oracle)[0][1]
    assert want.shape == (2 * qc.Q3_CALLS, 4)
    items = [it for j in range(qc.Q3_CALLS) for it in qc.q3_items(j)]
    assert {k for _, _, k in items} == set(qc.Q3_KS) and {t for t, _, _ in items} == set(qc.TAGS) and all(off + k <= pool.shape[0] for _, off, k in items)
    for k in qc.Q3_KS:                                                     # one item of every length through the Python sponge
        i = next(i for i, it in enumerate(items) if it[2] == k); tag, off, _ = items[i]
        assert pyref.from_limbs(want[i]) == pyref.tr_hash_fields_tagged(tag, ints(pool[off:off + k])), (i, items[i])
    f, d = qc.blocker_input(oracle, 16)
    assert pyref.from_limbs(d) == pyref.tr_hash_fields_tagged(qc.BLOCKER_TAG, ints(f))


def test_q1_roots_are_the_trees_over_the_extension_by_definition(oracle):
    I = qc.q1_inputs(oracle); g = I["coset"]
    for c, want in zip(I["cols"], I["lde"]):                                # LDE = coefficients, zero-padded, evaluated on the coset of the large domain
        coeff = np.zeros((qc.N11, 4), np.uint64); coeff[:qc.N8] = oracle.ntt(0, c, inverse=True)
        assert (oracle.ntt(0, coeff, coset=g) == want).all()
    plain, commit = qc.q1_refs(oracle, False), qc.q1_refs(oracle, True)
    for labels, leaves, key in ((qc.Q1_LABELS, I["lde"], "roots"), (qc.Q1_LABELS2, I["other"], "roots2")):
        for i in range(3):
            t = oracle.merkle_build(16, labels[i], leaves[i])
            try:
                assert t.num_levels() == 4 and (t.level(0) == leaves[i]).all() and (t.level(3)[0] == plain[key][i]).all() and (t.root() == plain[key][i]).all()
            finally:
                t.free()
            assert (commit[key][i] == oracle.commitment_root(labels[i], leaves[i])).all() and (commit[key][i] != plain[key][i]).any()
    roots = np.stack(plain["roots"] + plain["roots2"])
    assert len({r.tobytes() for r in roots}) == 6                          # a hash of the wrong batch's roots cannot pass for the right one
    first, second = plain["results"][3][1], plain["results"][4][1]
    assert first.shape == (5, 4) and second.shape == (3, 4) and (first[:3] != second).any(axis=1).all()
    assert pyref.from_limbs(first[0]) == pyref.tr_hash_fields_tagged(qc.TAGS[0], ints(plain["roots"][0]))
    assert pyref.from_limbs(first[3]) == pyref.tr_hash_fields_tagged(qc.TAGS[0], [])


def test_q2_points_and_references(oracle):
    I = qc.q2_inputs(oracle); cols, zs = I["cols"], I["zs"]; one = oracle.from_u64(1)
    inside = [p for p in range(zs.shape[0]) if (oracle.pow(zs[p], qc.N11) == one).all()]
    p, j = I["inside"]
    assert inside == [p] and (zs[p] == oracle.pow(oracle.domain_omega(qc.N11), j)).all()
    ref = dict(qc.q2_refs(oracle))
    lag = ref["stark_lagrange_eval_on_h_batch_dev"].reshape(3, 3, 4)
    for c in range(3):
        assert (lag[p, c] == cols[c][j]).all()                             # R3: inside H the value is the column's element
    assert (lag[[0, 2], :2] == lc.r1(oracle, cols[:2], zs[[0, 2]])).all()    # R1 outside H
    assert (ref["stark_lagrange_eval_on_h_dev"] == lag[2, 1]).all()
    r = I["r"]; P = pyref.P_PALLAS                                          # MLE by the definition on one table: fold the low variable first (channel/src/lib.rs:279-295)
    t = ints(cols[2]); rr = ints(r[0])
    for x in rr:
        t = [(t[2 * i] + x * (t[2 * i + 1] - t[2 * i])) % P for i in range(len(t) // 2)]
    assert t == ints(ref["stark_mle_evaluate_dev"])
    assert (ref["stark_mle_evaluate_batch_dev"][0] == oracle.mle_evaluate(cols[0], r[0])).all()
    g = I["coset"]                                                         # inverse then forward on the coset = the 1x extension onto the coset; the single inverse undoes a coset transform
    assert (ref["stark_ntt_batch_dev inverse, then forward on the coset, column 1"] == oracle.lde(0, cols[1], 0, g)).all()
    assert (oracle.ntt(0, ref["stark_ntt_dev"], coset=g) == cols[0]).all()
    assert (ref["stark_lde_dev"][::2] == oracle.lde(0, cols[1], 0, g)).all()


def test_q4_references_chain(oracle):
    I = qc.q4_inputs(oracle); ref = dict(qc.q4_refs(oracle)); L = len(qc.FRI_SCHEDULE)
    lde = [ref["stark_lde_batch_dev, output %d" % i] for i in range(4)]
    assert qc.N11 % int(np.prod(qc.FRI_SCHEDULE)) == 0 and ref["stark_fri_build_dev, the roots"].shape == (L + 1, 4)
    a, s, e, t, f0 = [ints(x[:3]) for x in lde + [ref["stark_ali_merge_dev"]]]    # f0[j] = (a s + e - t - c* (z^n - 1)) / (w^j - z), so (w^j - z) f0[j] - phi[j] is one constant
    P = pyref.P_PALLAS; w, z = ints(I["omega"])[0], ints(I["z"])[0]
    consts = {((pow(w, j, P) - z) * f0[j] - (a[j] * s[j] + e[j] - t[j])) % P for j in range(3)}
    assert len(consts) == 1
    p = oracle.deep_fri_prove(None, None, None, None, qc.N11, qc.FRI_SCHEDULE, 1, qc.SEED_Z, f0=ref["stark_ali_merge_dev"])
    try:
        assert (p.layer_f(1) == oracle.fri_fold_layer(ref["stark_ali_merge_dev"], oracle.fri_sample_z_ell(qc.SEED_Z, 0, qc.N11), qc.FRI_SCHEDULE[0])).all()
    finally:
        p.free()
    assert ref["stark_fri_fold_dev"].shape == (qc.N11 // 8, 4) and ref["stark_poseidon_hash_ds_batch_dev"].shape == (128, 4)
    assert pyref.from_limbs(ref["stark_leaf_pair_hash_dev"][9]) == pyref.hash_leaf_pair(ints(lde[1][9:10])[0], ints(ref["stark_fri_fold_dev"][1:2])[0])
    assert pyref.from_limbs(ref["stark_tr_hash_fields_tagged_dev"][7]) == pyref.tr_hash_fields_tagged(qc.TAGS[0], ints(ref["stark_poseidon_hash_ds_batch_dev"][112:128]))
