"""Forged proofs that break exactly one check of a verifier each (tests/test_verify_forgery_host.py on the CPU, tests/test_gpu_verify_forgery.py on
the GPU): Python provers of prove_plain / prove_mf (channel/src/lib.rs:1045-1076, :1130-1172) that take a deviation hook, a census of the verifiers'
relations in Python integers that says WHICH relation of a proof fails, and the catalogues built from both.  The expected decision of every case is
the oracle's on the same bytes; the census is the premise ("exactly this one check fails"), established without the code under test.  Not a test module."""
import collections
import copy
import functools
import random

import numpy as np

import merkle_batch_cases as mc
import pyref

R = pyref.P_PALLAS
SEED_Z = 0xDEEFBAAD
MF_SHAPES = [(5, 7105, 3), (2, 7102, 1), (1, 7101, 1), (0, 7100, 1)]          # (k, label, q)
PLAIN_SHAPES = [(5, 8105), (2, 8102), (1, 8101)]                              # (k, label)
DEEP_FRI_SHAPES = [(1 << 9, [8, 4, 2], 5), (1 << 10, [16, 8], 8), (2, [2], 1)]  # from SHAPES of tests/test_gpu_verify_batch.py
POSITIONS = (0, 255, 256, 299)
B_POS = 300
# The forgeries put at each place of a batch: the first and the last relation of the proof (chain(1) and final).  verify_mf's plan also holds fold
# records in front of the first chain record and the root comparisons behind every other record: the first fold and the last comparison are the first
# and the last record the plan holds for the proof (the GPU test runs them too).
POSITION_FORGERIES_PLAIN = ["plain k=2 P3(1)", "plain k=2 P1"]
POSITION_FORGERIES_MF = ["mf k=2 F2(1)", "mf k=2 F3", "mf k=2 F4(0,0)", "mf k=2 F5 next_root"]

Case = collections.namedtuple("Case", "name mf k label q proof census accept")     # census: the items census_* must list, in its order


def limbs(x):
    return np.array(pyref.to_limbs(x % R), np.uint64)


def rows(xs):
    return np.array([pyref.to_limbs(x % R) for x in xs], np.uint64).reshape(-1, 4)


def ints(a):
    return [pyref.from_limbs(row) for row in np.asarray(a, np.uint64).reshape(-1, 4)]


def witness(oracle, seed, k):
    return ints(oracle.rand_fr_columns(seed, 1 << k, 1)[0])


# ---- the Python provers ------------------------------------------------------------------------------------------------------------
class Tree:
    """MerkleCommitment's tree of a layer of integers (the oracle's: arity 16, "POSEIDON-T17-X5-SEED")"""

    def __init__(self, oracle, label, layer):
        self.t = oracle.merkle_build(16, label, rows(layer), params_kind=2); self.root = pyref.from_limbs(self.t.root())

    def open(self, idx):
        p = pyref.mproof_parse_canonical(self.t.open_bytes(idx)); del p["sib_off"]; return p

    def free(self):
        self.t.free()


def round_coeffs(layer):                                                       # channel/src/lib.rs:406-416
    return [sum(layer[0::2]) % R, sum(b - a for a, b in zip(layer[0::2], layer[1::2])) % R]


def fold(layer, r):                                                            # :456-462 / :640-647
    return [((1 - r) * a + r * b) % R for a, b in zip(layer[0::2], layer[1::2])]


def _no_hook(event, i, value):
    return value


def prove_plain(oracle, k, label, wit, hook=None):
    """prove_plain over Python integers -> ProofPlain bytes.  hook(event, i, value) -> value may deviate at
    "layer" (the layer round i starts from), "coeffs" ([c0, c1] as sent in round i) and "final" (final_eval)."""
    hook = hook or _no_hook
    layer = [x % R for x in wit]; assert len(layer) == 1 << k
    ch = pyref.Channel(b"E2E/PLAIN")
    t = Tree(oracle, label, layer); root = t.root; t.free()
    ch.send_digest(b"commit/root", root)
    ch.bytes(b"SUMCHECK/CLAIM"); ch.tr.absorb_field(sum(layer) % R)
    rounds = []
    for i in range(k):
        layer = hook("layer", i, layer)
        c0, c1 = hook("coeffs", i, round_coeffs(layer))
        ch.bytes(b"SUMCHECK/ROUND"); ch.bytes(pyref.le64(i)); ch.bytes(b"COEFF/c0"); ch.tr.absorb_field(c0); ch.bytes(b"COEFF/c1"); ch.tr.absorb_field(c1)
        layer = fold(layer, ch.challenge_scalar(b"sumcheck/r" + pyref.le64(i)))
        rounds.append([c0, c1])
    return pyref.encode_proof_plain(dict(root=root, rounds=rounds, final_eval=hook("final", k, layer[0])))


def prove_mf(oracle, k, label, q, wit, queries=None, hook=None):
    """prove_mf over Python integers -> ProofMF bytes.  queries[i]: the indices opened in the next layer of round i (the verifier never derives
    them, so they are the prover's to choose); None derives them from the channel as the reference does (:656-690).
    hook(event, i, value) -> value may deviate at "coeffs" ([c0, c1] as sent), "next" (the layer committed in round i, from which the prover
    continues) and "final" (final_eval)."""
    hook = hook or _no_hook
    cur = [x % R for x in wit]; assert len(cur) == 1 << k
    ch = pyref.Channel(b"E2E/MF") if queries is None else None
    cur_tree = Tree(oracle, label, cur)
    P = dict(initial_root=cur_tree.root, rounds=[])
    if ch:
        ch.send_digest(b"sumcheck-mf/root/0", cur_tree.root); ch.bytes(b"SUMCHECK/MF/CLAIM"); ch.tr.absorb_field(sum(cur) % R)
    for i in range(k):
        c0, c1 = hook("coeffs", i, round_coeffs(cur))
        if ch:
            ch.bytes(b"SUMCHECK/MF/ROUND"); ch.bytes(pyref.le64(i)); ch.bytes(b"COEFF/c0"); ch.tr.absorb_field(c0); ch.bytes(b"COEFF/c1"); ch.tr.absorb_field(c1)
        r = pyref.mf_round_challenge_from_root(i, cur_tree.root)
        half = len(cur) // 2
        nxt = hook("next", i, fold(cur, r))
        next_tree = Tree(oracle, label, nxt)
        if ch:
            ch.send_digest(b"sumcheck-mf/root/next", next_tree.root)
            q_target = min(max(q, 1), half); qs = set(); j = 0
            while len(qs) < q_target and j < max(16 * q_target, 16):
                qs.add(pyref.mf_query_index(ch.challenge_scalar(b"sumcheck-mf/q" + pyref.le64(i) + pyref.le64(j)), half)); j += 1
            for ix in range(half):
                if len(qs) < q_target:
                    qs.add(ix)
        else:
            qs = set(queries[i])
        qs = sorted(qs)
        Rn = dict(c0=c0, c1=c1, next_root=next_tree.root)
        Rn["cur_indices"] = [2 * j + b for j in qs for b in (0, 1)]; Rn["cur_values"] = [cur[ix] for ix in Rn["cur_indices"]]; Rn["cur_proof"] = cur_tree.open(Rn["cur_indices"])
        Rn["next_indices"] = qs; Rn["next_values"] = [nxt[ix] for ix in qs]; Rn["next_proof"] = next_tree.open(qs)
        if ch:
            ch.send_opening(Rn["cur_indices"], Rn["cur_values"], Rn["cur_proof"]); ch.send_opening(Rn["next_indices"], Rn["next_values"], Rn["next_proof"])
        P["rounds"].append(Rn)
        cur_tree.free(); cur, cur_tree = nxt, next_tree
    cur_tree.free()
    P["final_eval"] = hook("final", k, cur[0])
    return pyref.encode_proof_mf(P)


# ---- the census: which relations of a proof fail, in Python integers mod r ---------------------------------------------------------------
def census_plain(proof):
    """the failed items of verify_plain (:1080-1128) as (kind, round, position): decode (a value >= r), chain, final"""
    P = pyref.parse_proof_plain(proof); bad = []
    for rnd, pos, v in [(None, "root", P["root"])] + [(i, n, c) for i, cc in enumerate(P["rounds"]) for n, c in zip(("c0", "c1"), cc)] + [(None, "final_eval", P["final_eval"])]:
        if v >= R:
            bad.append(("decode", rnd, pos))
    if not P["rounds"]:
        return bad + [("shape", None, None)]
    ch = pyref.Channel(b"E2E/PLAIN"); ch.send_digest(b"commit/root", P["root"] % R)
    running = (2 * P["rounds"][0][0] + P["rounds"][0][1]) % R
    ch.bytes(b"SUMCHECK/CLAIM"); ch.tr.absorb_field(running)
    for i, (c0, c1) in enumerate(P["rounds"]):
        c0 %= R; c1 %= R
        ch.bytes(b"SUMCHECK/ROUND"); ch.bytes(pyref.le64(i)); ch.bytes(b"COEFF/c0"); ch.tr.absorb_field(c0); ch.bytes(b"COEFF/c1"); ch.tr.absorb_field(c1)
        if (2 * c0 + c1) % R != running:
            bad.append(("chain", i, None))
        running = (c0 + c1 * ch.challenge_scalar(b"sumcheck/r" + pyref.le64(i))) % R
    if P["final_eval"] % R != running:
        bad.append(("final", None, None))
    return bad


@functools.lru_cache(maxsize=None)
def _mf_challenge(i, root):
    return pyref.mf_round_challenge_from_root(i, root)


def _opening_holds(label, root, idx, values, proof):
    p = dict(proof, siblings=[[s % R for s in l] for l in proof["siblings"]])
    return mc.oracle_verify(16, label, limbs(root), idx, rows(values), pyref.mproof_canonical(p), commitment=True) == 1


def census_mf(proof, label):
    """the failed items of verify_mf (:1176-1240) as (kind, round, query / position): decode, chain, final, fold, eq-cur, eq-next; the eq-*
    entries are the oracle's verify_many_ds on that opening alone"""
    P = pyref.parse_proof_mf(proof); bad = []

    def rng(rnd, pos, v):
        if v >= R:
            bad.append(("decode", rnd, pos))
    rng(None, "initial_root", P["initial_root"])
    for i, Rn in enumerate(P["rounds"]):
        for n in ("c0", "c1", "next_root"):
            rng(i, n, Rn[n])
        for n in ("cur", "next"):
            for t, v in enumerate(Rn[n + "_values"]):
                rng(i, (n + "_value", t), v)
            for lv, l in enumerate(Rn[n + "_proof"]["siblings"]):
                for j, v in enumerate(l):
                    rng(i, (n + "_sibling", lv, j), v)
    rng(None, "final_eval", P["final_eval"])
    prev_root = P["initial_root"] % R; running = None
    for i, Rn in enumerate(P["rounds"]):
        c0, c1, next_root = Rn["c0"] % R, Rn["c1"] % R, Rn["next_root"] % R
        if running is not None and (2 * c0 + c1) % R != running:
            bad.append(("chain", i, None))
        r = _mf_challenge(i, prev_root)
        if not _opening_holds(label, prev_root, Rn["cur_indices"], Rn["cur_values"], Rn["cur_proof"]):
            bad.append(("eq-cur", i, None))
        if not _opening_holds(label, next_root, Rn["next_indices"], Rn["next_values"], Rn["next_proof"]):
            bad.append(("eq-next", i, None))
        if len(Rn["cur_indices"]) != len(Rn["cur_values"]) or len(Rn["next_indices"]) != len(Rn["next_values"]):
            bad.append(("shape", i, None)); break
        pairs = {}
        for ix, v in zip(Rn["cur_indices"], Rn["cur_values"]):
            pairs.setdefault(ix // 2, {})[ix % 2] = v % R
        for t, (j, v) in enumerate(zip(Rn["next_indices"], Rn["next_values"])):
            e = pairs.get(j, {})
            if 0 not in e or 1 not in e or ((1 - r) * e[0] + r * e[1] - v) % R:
                bad.append(("fold", i, t))
        running = (c0 + c1 * r) % R; prev_root = next_root
    if running is not None and P["final_eval"] % R != running:
        bad.append(("final", None, None))
    return bad


# ---- the sum-check catalogue ----------------------------------------------------------------------------------------------------------------
def _flip_sibling(proof):
    """one bit of one sibling of a proof dict (a middle sibling of its first level that has any); False: no sibling"""
    for l in proof["siblings"]:
        if l:
            l[len(l) // 2] ^= 1 << 9; return True
    return False


def _mf_cases(oracle, rng, k, label, q):
    """every forgery kind of the issue on one honest proof of the shape, and the honest proof itself"""
    tag = "mf k=%d " % k
    wit = witness(oracle, 300 + k, k)
    base = oracle.sumcheck_prove(1, k, label, rows(wit), q=q); B = pyref.parse_proof_mf(base)
    out = [Case(tag + "honest", 1, k, label, q, base, [], True)]
    d, b = rng.randrange(1, R), rng.randrange(1, R)

    def edit(name, census, fn, accept=False):
        P = copy.deepcopy(B); fn(P); out.append(Case(tag + name, 1, k, label, q, pyref.encode_proof_mf(P), census, accept))

    def coeffs(i, d0, d1):
        def fn(P):
            P["rounds"][i]["c0"] = (P["rounds"][i]["c0"] + d0) % R; P["rounds"][i]["c1"] = (P["rounds"][i]["c1"] + d1) % R
        return fn

    def final(P):
        P["final_eval"] = (P["final_eval"] + d) % R
    if k == 0:
        edit("F8", [], final, accept=True)                                                       # no round: any final_eval is accepted (:1237-1238)
        return out
    for i in range(k):
        edit("F1(%d)" % i, [("chain", i + 1, None)] if i + 1 < k else [("final", None, None)], coeffs(i, d, -2 * d))
    for i in range(1, k):
        r_i = pyref.mf_round_challenge_from_root(i, B["rounds"][i - 1]["next_root"])
        edit("F2(%d)" % i, [("chain", i, None)], coeffs(i, -b * r_i, b))
    edit("F3", [("final", None, None)], final)
    for i in range(k - 1):                                                                       # F4(i, t): next[j] += d at the queried j, -= d at an unqueried one
        queries = [Rn["next_indices"] for Rn in B["rounds"]]; n_next = 1 << (k - i - 1)
        if len(queries[i]) == n_next:
            queries[i] = queries[i][:-1]                                                         # leave one index unqueried
        spare = [j for j in range(n_next) if j not in queries[i]][0]
        for t, j in enumerate(queries[i]):
            def hook(ev, rnd, v, i=i, j=j, spare=spare):
                if ev == "next" and rnd == i:
                    v = list(v); v[j] = (v[j] + d) % R; v[spare] = (v[spare] - d) % R
                return v
            out.append(Case(tag + "F4(%d,%d)" % (i, t), 1, k, label, q, prove_mf(oracle, k, label, q, wit, queries, hook), [("fold", i, t)], False))

    def hook_last(ev, rnd, v):                                                                   # F4(k-1): the last layer committed as v + d, final_eval the running value
        if ev == "next" and rnd == k - 1:
            return [(v[0] + d) % R]
        return (v - d) % R if ev == "final" else v
    out.append(Case(tag + "F4(%d)" % (k - 1), 1, k, label, q, prove_mf(oracle, k, label, q, wit, [Rn["next_indices"] for Rn in B["rounds"]], hook_last), [("fold", k - 1, 0)], False))
    for i in range(k):
        for n in ("cur", "next"):
            if any(B["rounds"][i][n + "_proof"]["siblings"]):
                edit("F5 %s(%d)" % (n, i), [("eq-" + n, i, None)], lambda P, i=i, n=n: _flip_sibling(P["rounds"][i][n + "_proof"]))

    def next_root(P):
        P["rounds"][k - 1]["next_root"] ^= 1 << 70
    edit("F5 next_root", [("eq-next", k - 1, None)], next_root)
    # F6: the zero witness, one element encoded as r: every relation holds mod r
    zero = oracle.sumcheck_prove(1, k, label, rows([0] * (1 << k)), q=q); Z = pyref.parse_proof_mf(zero)
    assert census_mf(zero, label) == [] and Z["final_eval"] == 0 and all(Rn["c0"] == Rn["c1"] == 0 and not any(Rn["cur_values"] + Rn["next_values"]) for Rn in Z["rounds"])
    spots = [(0, "c0"), (0, "c1")] + ([(k - 1, "c0"), (k - 1, "c1")] if k > 1 else []) + [(k // 2, ("cur_value", 1)), (k // 2, ("next_value", 0)), (None, "final_eval")]
    for rnd, pos in spots:
        P = copy.deepcopy(Z)
        if pos == "final_eval":
            P["final_eval"] = R
        elif isinstance(pos, tuple):
            P["rounds"][rnd][pos[0] + "s"][pos[1]] = R
        else:
            P["rounds"][rnd][pos] = R
        out.append(Case(tag + "F6 %s" % (pos if rnd is None else "%s of round %d" % (pos, rnd),), 1, k, label, q, pyref.encode_proof_mf(P), [("decode", rnd, pos)], False))
    return out


def _boundary_cases(oracle, mf, label, rng):
    """k = 1 proofs whose c0 of round 0 is a chosen residue: encoded as r - 1 (honest, accepted: F7 / P5), as r + 1 and as 2^256 - 1 (the same residue
    as the honest 1 and 2^256 - 1 mod r, so only the range check rejects)"""
    out = []; tag = "mf k=1 " if mf else "plain k=1 "
    parse, enc = (pyref.parse_proof_mf, pyref.encode_proof_mf) if mf else (pyref.parse_proof_plain, pyref.encode_proof_plain)
    for name, c0, coded in (("F7" if mf else "P5", R - 1, R - 1), ("F6 c0 = r + 1" if mf else "P4 c0 = r + 1", 1, R + 1), ("F6 c0 = 2^256 - 1" if mf else "P4 c0 = 2^256 - 1", (2**256 - 1) % R, 2**256 - 1)):
        p = oracle.sumcheck_prove(mf, 1, label, rows([c0, rng.randrange(1, R)]), q=1); P = parse(p)
        c = P["rounds"][0]["c0"] if mf else P["rounds"][0][0]
        assert c == c0
        if mf:
            P["rounds"][0]["c0"] = coded
        else:
            P["rounds"][0][0] = coded
        out.append(Case(tag + name, mf, 1, label, 1, enc(P), [] if coded < R else [("decode", 0, "c0")], coded < R))
    return out


def _plain_cases(oracle, rng, k, label):
    tag = "plain k=%d " % k
    wit = witness(oracle, 400 + k, k)
    base = oracle.sumcheck_prove(0, k, label, rows(wit)); B = pyref.parse_proof_plain(base)
    out = [Case(tag + "honest", 0, k, label, 0, base, [], True)]
    d = rng.randrange(1, R)
    P = copy.deepcopy(B); P["final_eval"] = (P["final_eval"] + d) % R
    out.append(Case(tag + "P1", 0, k, label, 0, pyref.encode_proof_plain(P), [("final", None, None)], False))
    P = copy.deepcopy(B); P["rounds"][-1] = [(P["rounds"][-1][0] + d) % R, (P["rounds"][-1][1] - 2 * d) % R]
    out.append(Case(tag + "P2", 0, k, label, 0, pyref.encode_proof_plain(P), [("final", None, None)], False))
    for i in range(1, k):                                                                        # P3(i): from round i on, the layer with one entry changed by d
        def hook(ev, rnd, v, i=i):
            if ev == "layer" and rnd == i:
                v = list(v); v[len(v) // 2] = (v[len(v) // 2] + d) % R
            return v
        out.append(Case(tag + "P3(%d)" % i, 0, k, label, 0, prove_plain(oracle, k, label, wit, hook), [("chain", i, None)], False))
    zero = oracle.sumcheck_prove(0, k, label, rows([0] * (1 << k))); Z = pyref.parse_proof_plain(zero)
    assert census_plain(zero) == [] and Z["final_eval"] == 0 and not any(c for cc in Z["rounds"] for c in cc)
    # c0 and c1 of round 0 are each decoded twice by the plan (their own entries and the two halves of the claim entry), so either range check rejects them
    for rnd, pos in [(0, "c0"), (0, "c1")] + ([(k - 1, "c0"), (k - 1, "c1")] if k > 1 else []) + [(None, "final_eval")]:
        P = copy.deepcopy(Z)
        if rnd is None:
            P["final_eval"] = R
        else:
            P["rounds"][rnd][0 if pos == "c0" else 1] = R
        out.append(Case(tag + "P4 %s" % (pos if rnd is None else "%s of round %d" % (pos, rnd),), 0, k, label, 0, pyref.encode_proof_plain(P), [("decode", rnd, pos)], False))
    return out


_cache = {}


def sumcheck_catalogue(oracle):
    """every sum-check case of the issue (§2), built once per process and left unchanged"""
    if "sc" not in _cache:
        rng = random.Random(0xF026); cases = []
        for k, label, q in MF_SHAPES:
            cases += _mf_cases(oracle, rng, k, label, q)
        cases += _boundary_cases(oracle, 1, MF_SHAPES[2][1], rng)
        for k, label in PLAIN_SHAPES:
            cases += _plain_cases(oracle, rng, k, label)
        cases += _boundary_cases(oracle, 0, PLAIN_SHAPES[2][1], rng)
        assert len({c.name for c in cases}) == len(cases) and len({c.proof for c in cases}) == len(cases)
        _cache["sc"] = cases
    return _cache["sc"]


def assert_catalogue_complete(cases):
    """every round of every kind at k = 5, at least one case of every kind at k = 1 and k = 2, the zero-round case"""
    names = {c.name for c in cases}
    want = ["mf k=5 F1(%d)" % i for i in range(5)] + ["mf k=5 F2(%d)" % i for i in range(1, 5)] + ["mf k=5 F3", "mf k=5 F4(4)", "mf k=5 F5 next_root"]
    want += ["mf k=5 F4(%d,%d)" % (i, t) for i in range(3) for t in range(3)] + ["mf k=5 F4(3,0)"]          # queried index first, in the middle, last of q = 3
    want += ["mf k=5 F5 cur(%d)" % i for i in range(3)] + ["mf k=5 F5 next(%d)" % i for i in range(3)]      # rounds 3 and 4 open every leaf of both layers (q = 3): no sibling
    want += ["mf k=5 F6 " + s for s in ("c0 of round 0", "c1 of round 0", "c0 of round 4", "c1 of round 4", "('cur_value', 1) of round 2", "('next_value', 0) of round 2", "final_eval")]
    want += ["mf k=1 F6 c0 = r + 1", "mf k=1 F6 c0 = 2^256 - 1", "mf k=1 F7", "mf k=0 F8"]
    want += ["mf k=2 " + s for s in ("F1(0)", "F1(1)", "F2(1)", "F3", "F4(0,0)", "F4(1)", "F5 cur(0)", "F5 next(0)", "F5 next_root", "F6 c0 of round 0", "F6 final_eval")]
    want += ["mf k=1 " + s for s in ("F1(0)", "F3", "F4(0)", "F5 next_root", "F6 c0 of round 0", "F6 c1 of round 0", "F6 ('cur_value', 1) of round 0", "F6 ('next_value', 0) of round 0", "F6 final_eval")]
    want += ["plain k=5 P1", "plain k=5 P2"] + ["plain k=5 P3(%d)" % i for i in range(1, 5)] + ["plain k=5 P4 " + s for s in ("c0 of round 0", "c1 of round 0", "c0 of round 4", "c1 of round 4", "final_eval")]
    want += ["plain k=2 " + s for s in ("P1", "P2", "P3(1)", "P4 c0 of round 0", "P4 final_eval")]
    want += ["plain k=1 " + s for s in ("P1", "P2", "P4 c0 of round 0", "P4 c1 of round 0", "P4 final_eval", "P4 c0 = r + 1", "P4 c0 = 2^256 - 1", "P5")]
    missing = [w for w in want if w not in names]
    assert not missing, missing
    # the census of every rejecting case names one item, of every accepted one none
    assert all(len(c.census) == (0 if c.accept else 1) for c in cases)
    kinds = {(c.mf, c.census[0][0]) for c in cases if c.census}
    assert kinds == {(1, "decode"), (1, "chain"), (1, "final"), (1, "fold"), (1, "eq-cur"), (1, "eq-next"), (0, "decode"), (0, "chain"), (0, "final")}, kinds


def oracle_decision(oracle, c):
    return oracle.sumcheck_verify(c.mf, c.k, c.label, c.proof, q=c.q or 2) == 1


def census_of(c):
    return census_mf(c.proof, c.label) if c.mf else census_plain(c.proof)


# ---- DEEP-FRI -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _leaf_pair(f, s):
    return pyref.hash_leaf_pair(f, s)


def census_deep_fri(oracle, proof, sched, r):
    """Every Merkle opening of deep_fri_verify (fri.rs:643-762) verified on its own by the oracle's verify_many_ds / verify_pairs_ds, and the local
    checks: the failed items as ("child" | "parent", layer), ("final", L), ("local", query, layer), ("decode", ...), ("shape",)"""
    P = pyref.parse_deep_fri_proof(proof); L = len(sched); bad = []
    els = P["roots"] + [P["omega0"]] + [v for Q in P["queries"] for py in Q["pays"] for v in py.values()] + [v for Q in P["queries"] for v in (Q["final_f"], Q["final_s"])]
    els += [s for pr in [P["final_proof"]] + [lb[n] for lb in P["layers"] for n in ("child_proof", "parent_proof")] for l in pr["siblings"] for s in l]
    if any(v >= R for v in els):
        bad.append(("decode",))
    if len(P["roots"]) != L + 1 or len(P["layers"]) != L or len(P["queries"]) != r or r == 0 or any(len(Q["refs"]) != L or len(Q["pays"]) != L for Q in P["queries"]):
        return bad + [("shape",)]
    sizes = [P["n0"]]
    for m in sched:
        if sizes[-1] % m:
            return bad + [("shape",)]
        sizes.append(sizes[-1] // m)
    cmap, pmap = [{} for _ in range(L)], [{} for _ in range(L)]
    for Q in P["queries"]:
        for l in range(L):                                                                       # the FIRST payload of an index wins (:663-664)
            cmap[l].setdefault(Q["refs"][l]["i"], (Q["pays"][l]["f_i"], Q["pays"][l]["s_i"]))
            pmap[l].setdefault(Q["refs"][l]["parent_index"], (Q["pays"][l]["f_parent_b"], Q["pays"][l]["s_parent_b"]))

    def opening_holds(layer, m_req, idx, vals, pr):
        ar = oracle.pick_arity_for_layer(sizes[layer], m_req)
        if any(i not in vals for i in idx):
            return False
        f = [vals[i][0] % R for i in idx]; s = [vals[i][1] % R for i in idx]; root = limbs(P["roots"][layer]); pb = proof[pr["span"][0]:pr["span"][1]]
        if ar in (128, 64, 32, 16, 8):                                                           # hashed leaves (fri.rs:275): verify_single over hash_leaf_pair(f, s)
            return mc.oracle_verify(ar, layer, root, idx, rows([_leaf_pair(a, b) for a, b in zip(f, s)]), pb) == 1
        return mc.oracle_verify_pairs(ar, layer, root, idx, rows(f), rows(s), pb) == 1
    for l, lb in enumerate(P["layers"]):
        if not opening_holds(l, sched[l], lb["child_indices"], cmap[l], lb["child_proof"]):
            bad.append(("child", l))
        if not opening_holds(l + 1, sched[l + 1] if l + 1 < L else 1, lb["parent_indices"], pmap[l], lb["parent_proof"]):
            bad.append(("parent", l))
    for qi, Q in enumerate(P["queries"]):
        for l in range(L):
            if Q["refs"][l]["i"] // sched[l] >= sizes[l] // sched[l] or Q["pays"][l]["s_i"] % R != Q["pays"][l]["f_parent_b"] % R:
                bad.append(("local", qi, l))
    Q0 = P["queries"][0]
    if Q0["final_index"] != 0 or not opening_holds(L, 1, [0], {0: (Q0["final_f"], Q0["final_s"])}, P["final_proof"]):
        bad.append(("final", L))
    return bad


def deep_fri_proof(oracle, n0, sched, r, seed):
    cols = oracle.rand_fr_columns(seed, n0, 4)
    ref = oracle.deep_fri_prove(cols[0], cols[1], cols[2], cols[3], n0, sched, r, SEED_Z)
    b = ref.bytes(); ref.free(); return b


def _flip(b, off, bit=1):
    out = bytearray(b); out[off] ^= bit; return bytes(out)


def deep_fri_catalogue(oracle):
    """-> {(n0, tuple(sched), r): [(name, proof, census)]}: the honest proof, D1(l) for every root, D2 for every opening that has siblings"""
    if "fri" not in _cache:
        cat = {}
        for n0, sched, r in DEEP_FRI_SHAPES:
            honest = deep_fri_proof(oracle, n0, sched, r, 600 + n0); P = pyref.parse_deep_fri_proof(honest); L = len(sched)
            cases = [("honest", honest, [])]
            for l in range(L + 1):
                want = ([("parent", l - 1)] if l else []) + ([("child", l)] if l < L else []) + ([("final", L)] if l == L else [])      # the openings against roots[l]
                cases.append(("D1(%d)" % l, _flip(honest, P["root_off"][l] + 5, 1 << (l % 8)), want))
            openings = [(("child", l), lb["child_proof"]) for l, lb in enumerate(P["layers"])] + [(("parent", l), lb["parent_proof"]) for l, lb in enumerate(P["layers"])] + [(("final", L), P["final_proof"])]
            for item, pr in openings:
                levels = [lv for lv in pr["sib_off"] if lv]
                if levels:
                    lv = levels[len(levels) // 2]
                    cases.append(("D2 %s(%d)" % item, _flip(honest, lv[len(lv) // 2] + 3, 0x10), [item]))
            cat[(n0, tuple(sched), r)] = cases
        _cache["fri"] = cat
    return _cache["fri"]


# ---- Merkle -------------------------------------------------------------------------------------------------------------------------------
MerkleCase = collections.namedtuple("MerkleCase", "name arity label root idx values cp proof")    # cp None: verify_many_ds; else verify_pairs_ds over (values, cp)
MERKLE_SHAPES = [(16, 4096, False, [4095, 17, 2048, 17]), (8, 19, False, [18, 0, 1, 18]), (8, 19, True, [18, 3])]


def merkle_oracle_decision(c):
    if c.cp is None:
        return mc.oracle_verify(c.arity, c.label, c.root, c.idx, c.values, c.proof) == 1
    return mc.oracle_verify_pairs(c.arity, c.label, c.root, c.idx, c.values, c.cp, c.proof) == 1


def merkle_catalogue(oracle):
    """M1-M3: per shape the honest opening, one sibling flipped at each level of the proof in turn, one bit of the claimed root (stored form) flipped
    in each of its eight 32-bit words in turn"""
    if "merkle" not in _cache:
        cases = []
        for si, (arity, n, pairs, idx) in enumerate(MERKLE_SHAPES):
            f = mc.leaves_of(oracle, 0xF02C, si, n); cp = mc.leaves_of(oracle, 0xF02C, si + 100, n) if pairs else None; label = 0x1234 + si
            t = oracle.merkle_build(arity, label, f, cp); root = t.root(); proof = t.open_bytes(idx); levels = t.num_levels(); t.free()
            tag = "(%d, %d%s) " % (arity, n, ", pairs" if pairs else ""); vals = f[idx]; cpv = None if cp is None else cp[idx]
            P = pyref.mproof_parse_canonical(proof)
            assert len(P["siblings"]) == levels - 1 and all(P["siblings"]) and levels == (4 if n == 4096 else 3)      # three hash levels over 4096 leaves; a ragged (8, 19)
            cases.append(MerkleCase(tag + "honest", arity, label, root, idx, vals, cpv, proof))
            for lv, offs in enumerate(P["sib_off"]):
                cases.append(MerkleCase(tag + "M2 level %d" % lv, arity, label, root, idx, vals, cpv, _flip(proof, offs[len(offs) // 2] + 7, 0x20)))
            for w in range(8):
                cases.append(MerkleCase(tag + "M3 word %d" % w, arity, label, mc.flip_bit(root, w // 2, 32 * (w % 2) + 3 + w), idx, vals, cpv, proof))
        _cache["merkle"] = cases
    return _cache["merkle"]


# ---- where the forgery sits in a batch ------------------------------------------------------------------------------------------------------
def position_batch(honest, forged, pos, B=B_POS):
    """`honest` cycled to B items with `forged` at index pos"""
    items = [honest[i % len(honest)] for i in range(B)]; items[pos] = forged
    return items


def sumcheck_position_set(oracle, mf):
    """-> (four honest k = 2 proofs of distinct witnesses, {name: forged case}, label, q)"""
    key = ("pos", mf)
    if key not in _cache:
        k, label, q = (MF_SHAPES[1] if mf else PLAIN_SHAPES[1] + (0,))
        honest = [oracle.sumcheck_prove(mf, k, label, oracle.rand_fr_columns(700 + i + 10 * mf, 1 << k, 1)[0], q=q or 2) for i in range(4)]
        assert len(set(honest)) == 4
        by = {c.name: c for c in sumcheck_catalogue(oracle)}
        _cache[key] = (honest, {n: by[n] for n in (POSITION_FORGERIES_MF if mf else POSITION_FORGERIES_PLAIN)}, label, q)
    return _cache[key]


def merkle_position_set(oracle):
    """four honest openings of (2, 8) trees under distinct labels, and forgeries of the first (with the oracle's rejection asserted): a sibling of
    each level, the claimed root -> (honest, {name: item}); an item is (label, root, idx, values, proof)"""
    if "mpos" not in _cache:
        honest = []
        for b in range(4):
            f = mc.leaves_of(oracle, 0xF02D, b, 8); t = oracle.merkle_build(2, 50 + b, f); idx = [5] if b == 0 else [5, b]
            honest.append((50 + b, t.root(), idx, f[idx], t.open_bytes(idx))); t.free()
        lab, root, idx, vals, proof = honest[0]; P = pyref.mproof_parse_canonical(proof)
        assert len(P["sib_off"]) == 3 and all(P["sib_off"])
        forged = {"level %d" % lv: (lab, root, idx, vals, _flip(proof, offs[-1] + 1, 2)) for lv, offs in enumerate(P["sib_off"])}
        forged["root"] = (lab, mc.flip_bit(root, 3, 40), idx, vals, proof)
        assert all(mc.oracle_verify(2, *it) == 1 for it in honest) and all(mc.oracle_verify(2, *it) == 0 for it in forged.values())
        _cache["mpos"] = (honest, forged)
    return _cache["mpos"]


MERKLE_POSITION_FORGERIES = ["level 0", "level 1", "level 2", "root"]


def commitment_openings(oracle):
    """openings under MerkleCommitment's parameters (CommitmentScheme::verify, commitment/src/lib.rs:96-113) taken out of the k = 5 ProofMF cases: the
    honest cur / next openings of rounds 0 and 1, the same with the sibling F5 flipped, and the round-0 cur opening against its root with one bit
    flipped in each 32-bit word -> [(name, label, root, idx, values, canonical proof bytes, the oracle's decision)]"""
    if "copen" not in _cache:
        by = {c.name: c for c in sumcheck_catalogue(oracle)}; label = MF_SHAPES[0][1]; out = []

        def opening(case, rnd, which):
            P = pyref.parse_proof_mf(case.proof); Rn = P["rounds"][rnd]
            root = (P["rounds"][rnd - 1]["next_root"] if rnd else P["initial_root"]) if which == "cur" else Rn["next_root"]
            return [label, limbs(root), Rn[which + "_indices"], rows(Rn[which + "_values"]), pyref.mproof_canonical(Rn[which + "_proof"])]
        for rnd in (0, 1):
            for which in ("cur", "next"):
                out.append(["honest %s(%d)" % (which, rnd)] + opening(by["mf k=5 honest"], rnd, which))
                out.append(["F5 %s(%d)" % (which, rnd)] + opening(by["mf k=5 F5 %s(%d)" % (which, rnd)], rnd, which))
        for w in range(8):
            it = opening(by["mf k=5 honest"], 0, "cur"); it[1] = mc.flip_bit(it[1], w // 2, 32 * (w % 2) + 11)
            out.append(["root word %d" % w] + it)
        out = [tuple(it) + (mc.oracle_verify(16, *it[1:], commitment=True) == 1,) for it in out]
        assert [it[-1] for it in out] == [it[0].startswith("honest") for it in out]
        _cache["copen"] = out
    return _cache["copen"]


# ---- the catalogues with their conditions asserted on the CPU, before any verifier under test is asked ---------------------------------------
_checked = set()


def checked_sumcheck_catalogue(oracle):
    """complete; the census lists exactly the aimed item (none for the accepted cases); the oracle rejects (accepts F7 / P5 / F8 and the honest proofs).
    Asserted once per process: the catalogue does not change, and no case is skipped or rebuilt."""
    cases = sumcheck_catalogue(oracle)
    if "sc" not in _checked:
        assert_catalogue_complete(cases)
        for c in cases:
            assert census_of(c) == c.census, c.name
            assert oracle_decision(oracle, c) == c.accept, c.name
        _checked.add("sc")
    return cases


def checked_deep_fri_catalogue(oracle):
    """D1(l) fails exactly the openings against roots[l], D2 exactly the opening whose sibling changed; the oracle rejects both kinds"""
    cat = deep_fri_catalogue(oracle)
    if "fri" in _checked:
        return cat
    assert set(cat) == {(n0, tuple(s), r) for n0, s, r in DEEP_FRI_SHAPES}
    for (n0, sched, r), cases in cat.items():
        names = [c[0] for c in cases]
        assert all("D1(%d)" % l in names for l in range(len(sched) + 1)) and names[0] == "honest"
        for name, proof, census in cases:
            assert census_deep_fri(oracle, proof, list(sched), r) == census, (n0, name)
            assert (oracle.deep_fri_verify(proof, list(sched), r, SEED_Z) == 1) == (name == "honest"), (n0, name)
            assert (name == "honest") == (not census) and (not name.startswith("D2") or len(census) == 1)
    names = [c[0] for c in cat[(1 << 9, (8, 4, 2), 5)]]
    assert [n for n in names if n.startswith("D2")] == ["D2 child(0)", "D2 child(1)", "D2 child(2)", "D2 parent(0)", "D2 parent(1)", "D2 parent(2)", "D2 final(3)"]
    assert [c[0] for c in cat[(2, (2,), 1)]] == ["honest", "D1(0)", "D1(1)", "D2 child(0)"]    # the one-leaf parent and final layers have no sibling
    _checked.add("fri")
    return cat


def deep_fri_position_set(oracle):
    """four honest (2, [2], 1) proofs and the forgeries of the catalogue's: the first root comparison of the item, its last ones, a sibling"""
    if "fpos" not in _cache:
        n0, sched, r = DEEP_FRI_SHAPES[2]
        honest = [deep_fri_proof(oracle, n0, sched, r, 800 + i) for i in range(4)]
        assert len(set(honest)) == 4 and all(oracle.deep_fri_verify(p, sched, r, SEED_Z) == 1 for p in honest)
        _cache["fpos"] = (honest, {c[0]: c[1] for c in checked_deep_fri_catalogue(oracle)[(n0, tuple(sched), r)] if c[0] != "honest"})
    return _cache["fpos"]


DEEP_FRI_POSITION_FORGERIES = ["D1(0)", "D1(1)", "D2 child(0)"]
