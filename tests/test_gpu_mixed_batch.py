"""Mixed-size batches on the GPU: stark_merkle_build_mixed_batch_dev and stark_commitment_commit_mixed_batch_dev (every DS kernel form over the ragged
stream, csrc/poseidon_streams.hpp DsRaggedStream) against stark_merkle_build_dev tree by tree and byte for byte, and against the CPU oracle;
stark_sumcheck_prove_plain_mixed_batch_dev / stark_sumcheck_prove_mf_mixed_batch_dev against the single prove of each witness and the oracle.
Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import merkle_batch_cases as mc
import mixed_batch_cases as xc
import queued_cases as qc
from test_gpu_merkle_batch import Single, dev, hp, tab

pytestmark = pytest.mark.gpu
vp = C.c_void_p
_singles = {}
_inputs = {}


def inputs(oracle, arity, ns, pairs):
    """host and device columns of one mixed call (uploaded once per session and never written)"""
    key = (arity, tuple(ns), pairs)
    if key not in _inputs:
        fs = [xc.leaves_of(oracle, b, n) for b, n in enumerate(ns)]
        cps = xc.cps_of(oracle, ns) if pairs else None
        _inputs[key] = (fs, cps, [dev(f) for f in fs], None if cps is None else [None if c is None else dev(c) for c in cps])
    return _inputs[key]


def single(ctx, oracle, arity, b, n, pairs, label):
    """stark_merkle_build_dev of column b alone under the default options (built once)"""
    key = (arity, b, n, pairs, label)
    if key not in _singles:
        f = xc.leaves_of(oracle, b, n)
        cp = None if not pairs else (np.zeros((n, 4), np.uint64) if xc.cp_is_null(b) else mc.leaves_of(oracle, xc.SEED, b + 100, n))
        _singles[key] = Single(ctx, arity, label, f, cp)
    return _singles[key]


def build_mixed(ctx, arity, labels, fd, ns, cd=None):
    return ctx.merkle_build_mixed_batch_dev([t.data_ptr() for t in fd], ns, arity, labels, ctx.poseidon_params_for_arity(arity),
                                            None if cd is None else [None if t is None else t.data_ptr() for t in cd])


def check_mixed(ctx, ref_ctx, oracle, arity, ns, pairs, with_oracle=False, opens=False):
    B = len(ns); labels = xc.labels_of(B)
    fs, cps, fd, cd = inputs(oracle, arity, ns, pairs)
    trees = build_mixed(ctx, arity, labels, fd, ns, cd)
    refs = [single(ref_ctx, oracle, arity, b, n, pairs, labels[b]) for b, n in enumerate(ns)]
    for b, (t, r) in enumerate(zip(trees, refs)):
        assert t.num_levels == len(r.levels), (b, ns[b])
        for v, want in enumerate(r.levels):
            assert (t.level(v) == want).all(), "tree %d (n = %d) level %d" % (b, ns[b], v)
    if with_oracle:
        roots = ctx.merkle_roots_batch(trees)
        for b, n in enumerate(ns):
            assert (roots[b] == xc.oracle_tree(oracle, arity, b, n, pairs, labels[b]).root()).all(), (b, n)
    if opens:
        ixs = [mc.index_lists(n, b) for b, n in enumerate(ns)]
        opened = ctx.merkle_open_batch(trees, ixs)
        assert opened == [r.open(ix) for r, ix in zip(refs, ixs)]
        ok = ctx.merkle_verify_single_batch(arity, labels, [r.root for r in refs], ixs, [fs[b][ixs[b]] for b in range(B)], opened)
        assert ok == [True] * B
    for t in trees:
        t.free()


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("arity", sorted(xc.SETS))
def test_mixed_build_equals_single_builds(gpu_ctx, oracle, arity, pairs):
    """every level of every tree of one mixed call equals stark_merkle_build_dev on that column alone; the roots (stark_merkle_roots_batch) are the
    oracle's; the openings of the plain trees (stark_merkle_open_batch) are the single trees' and pass stark_merkle_verify_many_ds_batch"""
    check_mixed(gpu_ctx, gpu_ctx, oracle, arity, xc.SETS[arity], pairs, with_oracle=True, opens=not pairs)


def test_every_kernel_form_runs_the_ragged_stream(gpu_ctx, oracle):
    """one arity-16 call whose first node level has 4654 hashes (the wave pair), the next 293 (one wave per node) and the rest at most 20 (five
    waves per node): the form is chosen for the launch's total number of hashes"""
    ns = xc.THRESHOLDS; lens = [level_lens(n, 16) for n in ns]
    hashes = [sum(l[v] for l in lens if len(l) > v) for v in range(1, max(len(l) for l in lens))]
    assert hashes[0] > 4096 and 256 < hashes[1] <= 4096 and all(x <= 256 for x in hashes[2:]), hashes
    check_mixed(gpu_ctx, gpu_ctx, oracle, 16, ns, False, with_oracle=True)


def level_lens(n, arity):
    lens = [n]
    while lens[-1] > 1:
        lens.append((lens[-1] + arity - 1) // arity)
    return lens


@pytest.mark.parametrize("option", ["merkle_wave_pair", "poseidon_lane_only", "sponge_one_wave"])
def test_mixed_build_under_forced_kernel_forms(gpu_ctx, oracle, option):
    """the arity-16 set, plain and as pairs, with every level on the wave pair, on one lane per sponge, and with the small levels on one wave"""
    from stark_mlwe_amd.api import Context
    c = Context(0)
    try:
        c.set_option(option, 1)
        for pairs in (False, True):
            check_mixed(c, gpu_ctx, oracle, 16, xc.SETS[16], pairs)
        c.sync()
    finally:
        c.close()


def test_commit_mixed_equals_single_commits(gpu_ctx, oracle):
    """stark_commitment_commit_mixed_batch_dev equals stark_commitment_commit vector by vector, and the oracle's roots"""
    ns = [1, 17, 273, 2]; tags = [11, 12, 13, 14]
    cols = [xc.leaves_of(oracle, 40 + b, n) for b, n in enumerate(ns)]; cd = [dev(x) for x in cols]
    trees = gpu_ctx.commitment_commit_mixed_batch_dev(tags, [t.data_ptr() for t in cd], ns)
    for b in range(len(ns)):
        root, ref = gpu_ctx.commitment_commit(tags[b], cols[b])
        assert trees[b].num_levels == ref.num_levels and all((trees[b].level(v) == ref.level(v)).all() for v in range(ref.num_levels)), b
        assert (root == oracle.commitment_root(tags[b], cols[b])).all()
        ref.free(); trees[b].free()


def test_refusals_and_ownership(gpu_ctx, oracle):
    """the refused-argument list of include/stark_mlwe.h: the stated code, every out[i] NULL and stark_ctx_cached_bytes unchanged (n[i] = 0 in the
    last slot); handles freed in a scrambled order bring the pool back to where one build-and-free cycle left it; the leaves are intact"""
    from stark_mlwe_amd.api import Context
    c = Context(0)
    try:
        lib, h = c.lib, c.h
        arity, ns = 16, xc.SETS[16][:8]; B = len(ns); labels = xc.labels_of(B)
        fs, _, fd, _ = inputs(oracle, arity, xc.SETS[16], False); fd = fd[:B]
        p17, p9 = c.poseidon_params_for_arity(16).h, c.poseidon_params_for_arity(8).h
        for t in build_mixed(c, arity, labels, fd, ns):                    # the warm-up cycle: the pool now holds every block of this call
            t.free()
        base = lib.stark_ctx_cached_bytes(h)
        lab = np.array(labels, np.uint64); leaves = tab([t.data_ptr() for t in fd]); nn = (C.c_size_t * B)(*ns)

        def build(ctx=h, p=p17, arity_=16, batch=B, labels_=lab, lv=leaves, n_=nn, pairs=0, cp=None, null_out=False):
            out = (vp * B)(*[vp(0xDEAD)] * B)
            rc = lib.stark_merkle_build_mixed_batch_dev(ctx, p, arity_, batch, hp(labels_), lv, n_, pairs, cp, None if null_out else out)
            return rc, [out[b] for b in range(B)]
        assert build(batch=0)[0] == 0
        zero_last = (C.c_size_t * B)(*(ns[:-1] + [0])); too_many = (C.c_size_t * B)(*([1 << 30] * 2 + ns[2:]))
        for kw in (dict(ctx=None), dict(p=None), dict(labels_=None), dict(lv=None), dict(n_=None), dict(lv=tab([t.data_ptr() for t in fd[:-1]] + [None])), dict(pairs=1),
                   dict(n_=zero_last), dict(arity_=8), dict(arity_=0), dict(p=p9), dict(n_=too_many)):
            rc, out = build(**kw)
            assert rc == -1 and out == [None] * B, kw
            assert lib.stark_ctx_cached_bytes(h) == base, kw
        assert build(null_out=True)[0] == -1
        rc, out = build(p=p9, arity_=1)
        assert rc == -5 and out == [None] * B                              # arity 1 with some n > 1: STARK_ERR_UNSUPPORTED, as the single build
        ones = (C.c_size_t * B)(*[1] * B)
        rc, out = build(p=p9, arity_=1, n_=ones)                           # arity 1, one leaf each: the roots are the leaves
        assert rc == 0 and all(out)
        for o in out:
            lib.stark_merkle_free(vp(o))
        base = lib.stark_ctx_cached_bytes(h)                               # that call succeeded: its one block of B leaves is in the pool now
        out = (vp * B)(*[vp(0xDEAD)] * B)
        assert lib.stark_commitment_commit_mixed_batch_dev(h, B, hp(lab), leaves, None, out) == -1 and [out[b] for b in range(B)] == [None] * B
        assert lib.stark_commitment_commit_mixed_batch_dev(h, B, hp(lab), leaves, zero_last, out) == -1
        assert lib.stark_ctx_cached_bytes(h) == base
        trees = build_mixed(c, arity, labels, fd, ns)
        held = lib.stark_ctx_cached_bytes(h)
        assert held < base                                                 # the level blocks came out of the pool
        for b in (5, 0, 7, 2, 6, 1, 3):
            trees[b].free()
        assert lib.stark_ctx_cached_bytes(h) == held                       # the shared blocks stay out while one handle lives
        want = single(gpu_ctx, oracle, arity, 4, ns[4], False, labels[4])
        assert all((trees[4].level(v) == w).all() for v, w in enumerate(want.levels))
        trees[4].free()
        assert lib.stark_ctx_cached_bytes(h) == base                       # and go back once, with the last one
        c.sync()
        for b in range(B):
            assert (fd[b].cpu().numpy().view(np.uint64) == fs[b]).all(), b
    finally:
        c.close()


def test_mixed_build_returns_while_the_stream_is_busy(gpu_ctx, oracle):
    """stark_merkle_build_mixed_batch_dev queued behind the blocker of tests/queued_cases.py, its n, label and pointer tables destroyed the moment it
    returns: the blocker's event is still incomplete then, and the trees are byte-equal to the synchronised run's"""
    lib, h = gpu_ctx.lib, gpu_ctx.h
    arity, ns = 16, xc.SETS[16]; B = len(ns); labels = xc.labels_of(B)
    _, _, fd, cd = inputs(oracle, arity, ns, True)
    p = gpu_ctx.poseidon_params_for_arity(arity)

    def levels_of(handles):
        from stark_mlwe_amd.api import MerkleTree
        trees = [MerkleTree(gpu_ctx, vp(x), None) for x in handles]
        got = [t.levels for t in trees]
        for t in trees:
            t.free()
        return got

    def call():
        lab = np.array(labels, np.uint64); lv = qc.table([t.data_ptr() for t in fd]); cv = qc.table([None if t is None else t.data_ptr() for t in cd])
        nn = (C.c_size_t * B)(*ns); out = (vp * B)()
        rc = lib.stark_merkle_build_mixed_batch_dev(h, p.h, arity, B, hp(lab), lv, nn, 1, cv, out)
        return rc, out, (lab, lv, cv, nn)

    qc.Blocker(gpu_ctx, oracle, 16).start(); gpu_ctx.sync()                 # the blocker's tag frame, and (below) the pool blocks of the call: warm
    rc, out, _ = call(); gpu_ctx._chk(rc); gpu_ctx.sync()
    want = levels_of([out[b] for b in range(B)])
    blocker = qc.Blocker(gpu_ctx, oracle).start()
    rc, out, host = call()
    busy = blocker.still_busy()
    qc.clobber(*host)
    gpu_ctx._chk(rc)
    gpu_ctx.sync(); blocker.check()
    got = levels_of([out[b] for b in range(B)])
    assert busy, "stark_merkle_build_mixed_batch_dev returned only after the stream had drained (blocker: %.1f ms)" % blocker.ms()
    for b in range(B):
        assert len(got[b]) == len(want[b]) and all((g == w).all() for g, w in zip(got[b], want[b])), b
        ref = single(gpu_ctx, oracle, arity, b, ns[b], True, labels[b])
        assert all((g == w).all() for g, w in zip(got[b], ref.levels)), b


def test_mixed_build_does_not_read_what_its_blocks_held(gpu_ctx, oracle):
    """the arity-16 set, plain and as pairs, under pool_poison 0x5A and 0x00 (twice each: the second run takes the first one's blocks): the levels are
    the default run's and the roots the oracle's"""
    from stark_mlwe_amd.api import Context
    c = Context(0)
    try:
        for fill in (0x5A, 0x00):
            c.set_option("pool_poison", fill)
            for rep in (1, 2):
                for pairs in (False, True):
                    check_mixed(c, gpu_ctx, oracle, 16, xc.SETS[16], pairs, with_oracle=True)
        c.sync()
    finally:
        c.close()


# ---- mixed-size sum-check prove: stark_sumcheck_prove_plain_mixed_batch_dev / stark_sumcheck_prove_mf_mixed_batch_dev -------------------------
from test_gpu_sumcheck_batch import LABELS, single as sc_single, upload

SC_K = [0, 1, 5, 12, 3, 12, 0, 7]
_witnesses = {}


def sc_inputs(oracle, ks, seed):
    """host witnesses, labels and device tensors of one mixed call (uploaded once per session, never written)"""
    key = (tuple(ks), seed)
    if key not in _witnesses:
        ws = xc.witnesses_of(oracle, ks, seed)
        _witnesses[key] = (ws, [LABELS[b % len(LABELS)] for b in range(len(ks))], upload(ws))
    return _witnesses[key]


def prove_mixed(ctx, mf, ks, labels, ts, q):
    ptrs = [t.data_ptr() for t in ts]
    return ctx.prove_mf_mixed_batch_dev(ks, labels, q, ptrs) if mf else ctx.prove_plain_mixed_batch_dev(ks, labels, ptrs)


def check_sumcheck(ctx, oracle, mf, ks, q, seed, oracle_at=(), verify=False):
    ws, labels, ts = sc_inputs(oracle, ks, seed); B = len(ks)
    got = prove_mixed(ctx, mf, ks, labels, ts, q)
    assert len(got) == B
    for b in range(B):
        assert got[b] == sc_single(ctx, mf, ks[b], labels[b], q, ts[b]), (b, ks[b])
    for b in oracle_at:
        assert got[b] == oracle.sumcheck_prove(mf, ks[b], labels[b], ws[b], q=q if mf else 2), (b, ks[b])
    if verify:
        ok = ctx.verify_mf_batch(max(ks), labels, q, got) if mf else ctx.verify_plain_batch(max(ks), labels, got)
        assert ok == [bool(mf or k > 0) for k in ks]                        # verify_plain rejects a proof without rounds (:1100-1102)
    return got


@pytest.mark.parametrize("mf,q", [(0, 0), (1, 2)])
def test_mixed_sumcheck_equals_single_proofs(gpu_ctx, oracle, mf, q):
    """k = 0, 1, 5, 12, 3, 12, 0, 7 in one call: every proof is the single entry point's on that witness alone, three of them the oracle's, and
    the batch verifiers (which take proofs of any round counts) accept all but the plain proofs without a round"""
    check_sumcheck(gpu_ctx, oracle, mf, SC_K, q, 0x5C, oracle_at=(0, 3, 7), verify=True)


def test_mixed_sumcheck_redraws(gpu_ctx, oracle):
    """k = 3, 2, 1, 3 with q = 8: q >= half at every step, so duplicate draws are redrawn for some instances and the fill-in rule runs"""
    check_sumcheck(gpu_ctx, oracle, 1, [3, 2, 1, 3], 8, 0x6D, oracle_at=(0, 1, 2, 3), verify=True)


@pytest.mark.parametrize("mf,q", [(0, 0), (1, 2)])
def test_mixed_sumcheck_more_instances_than_cus(gpu_ctx, oracle, mf, q):
    """300 instances, k cycling 0 .. 4"""
    check_sumcheck(gpu_ctx, oracle, mf, [b % 5 for b in range(300)], q, 0x7E, oracle_at=(0, 4, 299))


@pytest.mark.parametrize("mf,q", [(0, 0), (1, 2)])
def test_mixed_sumcheck_in_another_order(gpu_ctx, oracle, mf, q):
    """the caller's order shuffled: the same proof per witness"""
    ws, labels, ts = sc_inputs(oracle, SC_K, 0x5C)
    got = prove_mixed(gpu_ctx, mf, SC_K, labels, ts, q)
    sh = [5, 2, 7, 0, 3, 6, 1, 4]
    got2 = prove_mixed(gpu_ctx, mf, [SC_K[i] for i in sh], [labels[i] for i in sh], [ts[i] for i in sh], q)
    assert got2 == [got[i] for i in sh]


def test_mixed_sumcheck_one_wave_transcripts_and_pool_poison(gpu_ctx, oracle):
    """the first case on a context with sponge_one_wave (the one-wave transcript kernel), and under pool_poison 0x5A and 0x00: the bytes of the
    default run, and the oracle's"""
    from stark_mlwe_amd.api import Context
    ws, labels, ts = sc_inputs(oracle, SC_K, 0x5C)
    want = {(mf, q): prove_mixed(gpu_ctx, mf, SC_K, labels, ts, q) for mf, q in ((0, 0), (1, 2))}
    for option, values in (("sponge_one_wave", (1,)), ("pool_poison", (0x5A, 0x00))):
        c = Context(0)
        try:
            for v in values:
                c.set_option(option, v)
                for (mf, q), w in want.items():
                    for rep in (1, 2):
                        assert prove_mixed(c, mf, SC_K, labels, ts, q) == w, (option, v, mf, rep)
            c.sync()
        finally:
            c.close()
    for b in (0, 3, 7):
        assert want[(0, 0)][b] == oracle.sumcheck_prove(0, SC_K[b], labels[b], ws[b], q=2) and want[(1, 2)][b] == oracle.sumcheck_prove(1, SC_K[b], labels[b], ws[b], q=2)


def test_mixed_sumcheck_argument_errors(gpu_ctx, oracle):
    """a null k, a k above 40, a null witness: INVALID_ARG and every out[i] NULL; batch == 0 is OK"""
    lib, h = gpu_ctx.lib, gpu_ctx.h
    _, _, ts = sc_inputs(oracle, [3, 2, 1, 3], 0x6D)
    w = (vp * 2)(ts[0].data_ptr(), ts[1].data_ptr()); lab = np.array([1, 2], np.uint64); ks = (C.c_size_t * 2)(3, 2)
    assert lib.stark_sumcheck_prove_plain_mixed_batch_dev(h, 0, None, None, None, None) == 0
    assert lib.stark_sumcheck_prove_mf_mixed_batch_dev(h, 0, None, None, None, 2, None) == 0
    for kw in (dict(k=None), dict(k=(C.c_size_t * 2)(3, 41)), dict(w=(vp * 2)(ts[0].data_ptr(), None)), dict(lab=None), dict(ctx=None)):
        a = dict(ctx=h, w=w, k=ks, lab=hp(lab)); a.update(kw)
        for mf in (0, 1):
            out = (vp * 2)(1, 1)
            rc = lib.stark_sumcheck_prove_mf_mixed_batch_dev(a["ctx"], 2, a["w"], a["k"], a["lab"], 2, out) if mf else lib.stark_sumcheck_prove_plain_mixed_batch_dev(a["ctx"], 2, a["w"], a["k"], a["lab"], out)
            assert rc == -1 and out[0] is None and out[1] is None, (kw, mf)
