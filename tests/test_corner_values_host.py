"""Stored-limb corner values through the host build of the product's inline code (libstark_mlwe_hostcheck.so), against Python big integers
and the oracle.  The inputs are corners of the four u64 limbs AS STORED (Montgomery form) — tests/corner_values.py — not corners of the
logical value: logical r - 1 is stored as 4t ~ 2^127 for Pallas, a benign operand.  CPU only.

The steered tests put chosen stored words behind EVERY S-box of a permutation, not only round 0: the round constants are free (the S-box input
of every round is state + rc), so for one state they are chosen such that all 8 t full-round outputs and all rp partial-round outputs are stored
corners (corner_values.steered_params).

Still open: the partial-round S-box outputs are controlled now, but nothing here drives one lane of pair_lane_update to its 2.7 r bound (after 16
blocks of partial rounds), or the wave form's lanes to theirs: that would need a search over the x_q against the kernel-form w tables."""
import numpy as np
import pytest

import corner_values as cv
import pyref

R = pyref.R
FIELDS = [(0, pyref.P_PALLAS), (1, pyref.P_BLS)]
P = pyref.P_PALLAS
# (hostcheck kind, seed, oracle kind, pyref parameters) of the t = 17 parameter sets
SETS17 = {"merkle": (0, b"", 0, lambda: pyref.params_for_width(17)),
          "transcript": (1, b"", 1, lambda: pyref.derive_params(b"POSEIDON-T17-X5-TRANSCRIPT", 17, 8, 64)),
          "bench": (2, b"POSEIDON-T17-X5", 3, lambda: pyref.derive_params(b"POSEIDON-T17-X5", 17, 8, 64))}


def test_corner_family_contents():
    for _, p in FIELDS:
        c = cv.stored_corners(p)
        assert len(set(c)) == len(c) >= 38 and all(0 <= v < p for v in c)
        for v in (0, 1, 2, p - 1, p - 2, (1 << 254) - 1, 1 << 254, (1 << 254) + 1, R % p, p - R % p, (p - 1) // 2):
            assert v in c
        for v in cv.carry_chains():
            assert v in c
        b = c[c.index(cv.carry_chains()[0])].to_bytes(32, "little")
        assert b[0] == 0x80 and set(b[1:31]) == {0x7f} and b[31] == 0
        assert (cv.raw_to_int(cv.raw(p - 1)) == p - 1) and cv.raw(1 << 64).tolist() == [0, 1, 0, 0]
    assert any(1 << 254 <= v < P for v in cv.stored_corners(P))          # the band no synthetic column reaches


# ---- the construction itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_crafted_inputs_put_the_targets_behind_the_first_sbox(oracle, hostcheck, name):
    """ARK + S-box of a crafted node's first state, recomputed with Python integers and through the host copy of fr_add / fr_pow5_r29 / fr_mul:
    elements 4..15 carry the twelve targets limb for limb (and all seventeen for a crafted state).  The round constants Python derives are the ones the
    libraries hold.  Without this the device tests could silently stop testing anything if a constant's layout changed."""
    kind, seed, okind, mk = SETS17[name]
    params = mk()
    _, _, _, rcf, _ = oracle.poseidon_params(okind, 17)
    h = hostcheck.params(kind, 17, seed)
    _, rcf_h, _ = hostcheck.params_export(h, 17, 8, 64); hostcheck.params_free(h)
    for i in range(17):
        assert cv.raw_to_int(rcf[i]) == cv.stored_rc(params, 0, i) == cv.raw_to_int(rcf_h[i])
    corners = cv.stored_corners(P); L = len(corners)
    inv20 = cv.raw(pow(1 << 20, -1, P) * R % P)
    for rot in range(0, L, 5):
        targets = [corners[(rot + j) % L] for j in range(12)]
        kids = cv.crafted_children(params, targets)
        assert len(kids) == 16 and all(0 <= x < P for x in kids)
        ds = [16, 3, 1000 + rot, 42]
        state = [d * R % P for d in ds] + kids[:12] + [0]                  # stored first state of hash_with_ds_dynamic
        # Python: x2 = s^2 / 2^261, x4 = x2^2 / 2^261, x5 = s x4 / 2^261 on the stored s = x + rc
        for j in range(12):
            s = (state[4 + j] + cv.stored_rc(params, 0, 4 + j)) % P
            assert pow(s, 5, P) * pow(1 << 261, -4, P) % P == targets[j], (name, rot, j)
        # the host copy of the field code: add, then fr_pow5_r29 itself, and the square-square-multiply chain of fr_mul followed by 2^-20
        for j in range(12):
            s = hostcheck.fr_op(0, 0, cv.raw(state[4 + j]), rcf[4 + j])
            assert (hostcheck.fr_op(0, 8, s) == cv.raw(targets[j])).all(), (name, rot, j)
            s2 = hostcheck.fr_op(0, 2, s, s); s4 = hostcheck.fr_op(0, 2, s2, s2); s5 = hostcheck.fr_op(0, 2, s4, s)
            assert (hostcheck.fr_op(0, 2, s5, inv20) == cv.raw(targets[j])).all(), (name, rot, j, cv.hex_limbs(s5))
    targets = [corners[(3 + 2 * j) % L] for j in range(17)]
    st = cv.crafted_state(params, targets)
    for i in range(17):
        assert (hostcheck.fr_op(0, 8, hostcheck.fr_op(0, 0, cv.raw(st[i]), rcf[i])) == cv.raw(targets[i])).all(), i
    # the level builder is the same construction, vectorised
    ch, slot_idx = cv.crafted_level(params, L + 3)
    for n in (0, 1, L - 1, L + 2):
        want = cv.crafted_children(params, [corners[k] for k in slot_idx[n]], tail=[corners[(n + 12 + j) % L] for j in range(4)])
        assert (ch[16 * n:16 * n + 16] == cv.raw_array(want)).all()
    assert sorted(set(slot_idx[:L, 0].tolist())) == list(range(L)) and sorted(set(slot_idx[:L, 11].tolist())) == list(range(L))


# ---- fr.hpp -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,p", FIELDS)
def test_fr_hpp_on_all_pairs_of_stored_corners(oracle, hostcheck, field, p):
    """add / sub / mul on every ordered pair of stored corners, inverse / square / pow on every non-zero one: the host build of fr.hpp against
    Python (a Montgomery product is x * y * R^-1 on the stored values) and against the oracle."""
    c = cv.stored_corners(p); limbs = [cv.raw(v) for v in c]
    Ri = pow(R, -1, p)
    for x, a in zip(c, limbs):
        for y, b in zip(c, limbs):
            for op, want in ((0, (x + y) % p), (1, (x - y) % p), (2, x * y * Ri % p)):
                got = hostcheck.fr_op(field, op, a, b)
                assert cv.raw_to_int(got) == want, (field, op, hex(x), hex(y), cv.hex_limbs(got))
                assert (got == oracle.fr_op(field, op, a, b)).all(), (field, op, hex(x), hex(y))
    e = 0xFFFFFFFF00000003
    for x, a in zip(c, limbs):
        if x == 0:
            continue
        inv = hostcheck.fr_op(field, 3, a)
        assert cv.raw_to_int(inv) == pow(x, -1, p) * R * R % p and (inv == oracle.inv(a, field)).all(), hex(x)
        assert cv.raw_to_int(hostcheck.fr_op(field, 2, a)) == x * x * Ri % p                                   # b = NULL: the square
        pw = hostcheck.fr_op(field, 7, a, np.array([e, 0, 0, 0], np.uint64))
        assert cv.raw_to_int(pw) == pow(x * Ri % p, e, p) * R % p and (pw == oracle.pow(a, e, field)).all(), hex(x)
        assert cv.raw_to_int(hostcheck.fr_op(field, 5, a)) == x * Ri % p


# ---- wide dots ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 6, 7, 12, 13, 17, 24, 25, 27, 48, 59, 60, 61, 120, 129])
def test_wide_dots_on_stored_extremes(hostcheck, n):
    """sum a_i * b_i with every operand one stored extreme — p - 1 (every limb near its maximum: the true worst case of the column sums),
    2^254 - 1, 2^254, the two alternating-29-bit-limb values — in every combination of a and b, across the carry pass every 6 terms, the chunk
    of 60 and the <= 24-term radix-2^32 accumulator, against Python."""
    Ri = pow(R, -1, P)
    ext = [P - 1, (1 << 254) - 1, 1 << 254, cv.alt29(0), cv.alt29(1)]
    for x in ext:
        for y in ext:
            a, b = np.tile(cv.raw(x), (n, 1)), np.tile(cv.raw(y), (n, 1))
            want = n * x * y * Ri % P
            got = hostcheck.wide_dot(a, b)
            assert cv.raw_to_int(got) == want, (n, hex(x), hex(y), cv.hex_limbs(got))
            if n <= 24:
                assert cv.raw_to_int(hostcheck.wide_dot32(a, b)) == want, (n, hex(x), hex(y))
    c = cv.pattern_d(P, 2 * n)
    a, b = c[:n], c[n:][::-1]
    want = sum(cv.raw_to_int(a[i]) * cv.raw_to_int(b[i]) for i in range(n)) * Ri % P
    assert cv.raw_to_int(hostcheck.wide_dot(a, b)) == want
    if n <= 24:
        assert cv.raw_to_int(hostcheck.wide_dot32(a, b)) == want


# ---- ntt29 and partial_reduce -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,p", FIELDS)
def test_lazy_nine_limb_ntt_on_stored_extremes(oracle, hostcheck, field, p):
    """The NTT kernels' arithmetic on the host (hc_ntt29) for every sub-NTT size a pass can take, forward and inverse, on whole vectors of
    stored p - 1, stored 2^254 - 1, two alternating patterns, the corner list by index and a random draw from it: equal to the oracle, with the
    documented operand bounds (limbs <= 6 * 2^29, top limb < 2^29) asserted unchanged."""
    rng = np.random.default_rng(29 + field)
    corners = cv.raw_array(cv.stored_corners(p))
    seen_limb = seen_top = 0
    for log_b in list(range(1, 11)) + [12]:
        n = 1 << log_b
        pats = cv.patterns(p, n)
        pats["random corners"] = corners[rng.integers(0, corners.shape[0], n)]
        for name, x in pats.items():
            for inverse in (False, True):
                got, max_limb, max_top = hostcheck.ntt29(field, x, inverse)
                assert (got == oracle.ntt(field, x, inverse)).all(), (field, log_b, name, inverse)
                seen_limb, seen_top = max(seen_limb, max_limb), max(seen_top, max_top)
                assert max_limb <= 6 << 29 and max_top < 1 << 29, \
                    "field %d log_b %d %s inverse=%s: max limb %.3f * 2^29, max top limb %.3f * 2^29" % (field, log_b, name, inverse, max_limb / 2**29, max_top / 2**29)
    print("field %d: largest operand limb %.3f * 2^29, largest top limb %.3f * 2^29" % (field, seen_limb / 2**29, seen_top / 2**29))


@pytest.mark.parametrize("field,p", FIELDS)
def test_partial_reduce_on_stored_corners(hostcheck, field, p):
    """fr29_partial_reduce on the stored corners themselves, on corners plus small multiples of p (the quotient estimate sees the corner's
    limbs under another top limb) and on their lazy forms with weight pushed down into limbs of up to 7 * 2^29: same residue, limbs below
    2^29, result below 1.00002 p."""
    M = cv.M29
    cases = []
    for v in cv.stored_corners(p):
        for k in (0, 1, 2, 31, 63):
            w = v + k * p
            if w >= 1 << 261:
                continue
            l = [(w >> (29 * i)) & M for i in range(8)] + [w >> 232]
            cases.append(l)
            lz = l[:]
            for i in range(8):                                            # move as much weight as allowed one limb down
                m = min(lz[i + 1], 6)
                lz[i + 1] -= m; lz[i] += m << 29
            cases.append(lz)
    arr = np.array(cases, dtype=np.uint64).astype(np.uint32)
    assert (arr.astype(np.uint64) == np.array(cases, dtype=np.uint64)).all() and int(arr[:, :8].max()) < 7 << 29
    out = hostcheck.partial_reduce(field, arr)
    for lin, lout in zip(cases, out.tolist()):
        vin = sum(x << (29 * i) for i, x in enumerate(lin)); vout = sum(x << (29 * i) for i, x in enumerate(lout))
        assert vout % p == vin % p and all(x <= M for x in lout[:8]) and vout < p + (p >> 15), (lin, lout)


# ---- matrix-core emulation ----------------------------------------------------------------------------------------------------------
def corner_states17():
    """t = 17 states of stored corners: every corner in every element position (rotations), rows of 17 equal values, the carry-chain values and
    the all-0x7f value next to each other in every order of a rotation"""
    c = cv.stored_corners(P); L = len(c)
    rows = [[c[(i + j) % L] for j in range(17)] for i in range(L)]
    rows += [[v] * 17 for v in c]
    chain = cv.carry_chains() + [c[11]]
    assert c[11].to_bytes(32, "little")[:31] == b"\x7f" * 31
    rows += [[chain[(i + j) % len(chain)] for j in range(17)] for i in range(len(chain))]
    return rows


@pytest.mark.parametrize("name", ["merkle", "transcript"])
def test_matrix_core_emulation_on_stored_corners(hostcheck, name):
    """full_round_linear — the L*U rows of the VALU path (which = 0) and the emulated matrix-core path (which = 1: signed radix-256 recoding,
    fragment tables, fold, signed carry pass, Montgomery step) — for M and for B_1 * M on states of stored corners, against each other AND against
    a dense Python product 2^20 sum_j M[i][j] x_j computed from the exported constants (B_1 * M recomputed in Python from M; the 2^20 because
    the states are S-box outputs as fr_pow5_r29 delivers them, divided by 2^20)."""
    kind, seed, _, mk = SETS17[name]
    params = mk()
    h = hostcheck.params(kind, 17, seed)
    mds, _, _ = hostcheck.params_export(h, 17, 8, 64)
    Ri = pow(R, -1, P)
    M = [[cv.raw_to_int(mds[i * 17 + j]) * Ri % P for j in range(17)] for i in range(17)]
    assert M == params["mds"]
    mats = {False: M, True: cv.mds_pre_canonical(params)}
    rows = corner_states17()
    st = np.stack([cv.raw_array(r) for r in rows])
    for pre in (False, True):
        want = np.stack([cv.raw_array([(sum(mats[pre][i][j] * r[j] for j in range(17)) << cv.SBOX_SHIFT) % P for i in range(17)]) for r in rows])
        a = hostcheck.full_round_linear(h, 0, pre, st); b = hostcheck.full_round_linear(h, 1, pre, st)
        for k in np.nonzero((b != want).any(axis=(1, 2)))[0][:3]:
            raise AssertionError("matrix-core path, %s pre=%s, state %s" % (name, pre, cv.hex_limbs(st[k])))
        for k in np.nonzero((a != want).any(axis=(1, 2)))[0][:3]:
            raise AssertionError("L*U path, %s pre=%s, state %s" % (name, pre, cv.hex_limbs(st[k])))
        assert (a == b).all()
    hostcheck.params_free(h)


# ---- kernel bodies on the host ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,t,seed,okind", [(0, 9, b"", 0), (0, 17, b"", 0), (1, 17, b"", 1), (2, 17, b"POSEIDON-T17-X5", 3), (0, 33, b"", 0)])
def test_permutation_forms_on_corner_states(oracle, hostcheck, kind, t, seed, okind):
    corners = cv.stored_corners(P); L = len(corners)
    rows = [[corners[(i + j) % L] for j in range(t)] for i in range(0, L, 3 if t <= 17 else 12)] + [[corners[i]] * t for i in (3, 6, 11, 17)]
    if t == 17:
        params = {0: SETS17["merkle"], 1: SETS17["transcript"], 2: SETS17["bench"]}[kind][3]()
        rows += [cv.crafted_state(params, [corners[(i + 2 * j) % L] for j in range(17)]) for i in range(0, L, 7)]
    st = np.stack([cv.raw_array(r) for r in rows])
    want = oracle.permute(okind, t, st)
    h = hostcheck.params(kind, t, seed)
    assert (hostcheck.permute_dense(h, st, t) == want).all()
    assert (hostcheck.permute_kernel_form(h, st, t) == want).all()
    if t == 17:
        assert (hostcheck.permute_chain_model(h, st, t) == want).all()
        Ri = pow(R, -1, P)
        ref = pyref.permute([x * Ri % P for x in rows[-1]], params)                   # one crafted state through the big-integer permutation
        assert [cv.raw_to_int(x) for x in want[-1]] == [y * R % P for y in ref]
    hostcheck.params_free(h)


def test_sponge_bodies_on_corner_inputs(oracle, hostcheck):
    """leaf_pair, hash_ds_level (node and pair-leaf modes), tr_hash and hash_stream — the kernel bodies of the sponges — on corner inputs and on
    crafted nodes, against the oracle."""
    c = cv.pattern_d(P, 160)
    ht, h17, h9 = hostcheck.params(1), hostcheck.params(0, 17), hostcheck.params(0, 9)
    assert (hostcheck.leaf_pair(ht, c[:96], c[100:106], 16) == oracle.leaf_pair_hash(c[:96], c[100:106], 16)).all()
    assert (hostcheck.leaf_pair(ht, c[:50], None, 1) == oracle.leaf_pair_hash(c[:50], None, 1)).all()
    # node levels: crafted children (the recoding's corners behind round 0), a ragged last node; t = 17 and t = 9
    for h, params, arity, last in ((h17, pyref.params_for_width(17), 16, 5), (h9, pyref.params_for_width(9), 8, 3)):
        nodes = len(cv.stored_corners(P)) + 2
        for lc in (None, last):
            ch, _ = cv.crafted_level(params, nodes, last_children=lc)
            got = hostcheck.hash_ds_level(h, 0, arity, 2, 1000, 9, ch)
            full = nodes if lc is None else nodes - 1
            want = oracle.hash_with_ds_dynamic(0, arity + 1, cv.ds_words(oracle, arity, 2, 1000, 9, full), ch[:full * arity], arity, n=full)
            assert got.shape[0] == nodes and (got[:full] == want).all()
            if lc is not None:
                ds = cv.ds_words(oracle, arity, 2, 1000 + full, 9, 1)
                assert (got[full] == oracle.hash_with_ds_dynamic(0, arity + 1, ds, ch[full * arity:], lc)).all()
    # pair-leaf level against the oracle's pair tree
    f, cp = c[:64], c[64:128]
    tree = oracle.merkle_build(16, 5, f, cp)
    assert (hostcheck.hash_ds_level(h17, 1, 16, 0xFFFFFFFF, 0, 5, f, cp) == tree.level(0)).all()
    tree.free()
    for n in (1, 12, 13, 29, 45):
        assert (hostcheck.tr_hash(ht, b"ALI/A", c[:n]) == oracle.tr_hash_fields_tagged(b"ALI/A", c[:n])).all(), n
    got = hostcheck.tr_hash(ht, b"FRI/index", c[:150], n=50)
    for i in range(50):
        assert (got[i] == oracle.tr_hash_fields_tagged(b"FRI/index", c[3 * i:3 * i + 3])).all()
    ds = c[40:44]
    for cnt in (5, 12, 16, 28):
        assert (hostcheck.hash_stream(h17, 0, ds, 4, c[:cnt], cnt) == oracle.hash_with_ds_dynamic(0, 17, ds, c[:cnt], cnt)).all(), cnt
    hseed = hostcheck.params(2, 17, b"POSEIDON-T17-X5-SEED")
    for cnt in (1, 16, 17, 37):
        assert (hostcheck.hash_stream(hseed, 1, None, 0, c[:cnt], cnt, c[50]) == oracle.hash_with_ds(2, c[:cnt], c[50])).all(), cnt
    for h in (ht, h17, h9, hseed):
        hostcheck.params_free(h)


# ---- steered round constants: chosen stored words behind every S-box of all 72 rounds ----------------------------------------------------
_SCHEDULES = {}


def schedules(t):
    if t not in _SCHEDULES:
        _SCHEDULES[t] = cv.target_schedules(pyref.params_for_width(t))
    return _SCHEDULES[t]


def test_target_schedules_cover_every_round_half_and_block_position():
    """By computation, for every width: each uniform corner has a schedule of its own, and over the rotations every other stored corner is the S-box
    output of every full round in every element half (X and Y of the wave pair for t = 17) and x_q at every position q mod 4."""
    corners = cv.stored_corners(P)
    for t in (9, 17, 33, 65):
        sc = schedules(t)
        full, part, uni = cv.schedule_coverage(t, [(tf, tp) for _, tf, tp in sc])
        assert full.shape == (len(corners), 8, 2 if t == 17 else 1) and full.all() and part.all(), t
        assert uni == set(cv.uniform_corners(P)) and len(uni) == 9
        for c in (P - 1, (1 << 254) - 1, 1 << 254, cv.alt29(0), cv.alt29(1)):
            assert c in uni
        rot = [s for s in sc if s[0].startswith("rotation")]
        rest = len(corners) - 9
        assert len(rot) == max(-(-rest // (8 if t == 17 else t)), -(-rest // (pyref.RP_FOR_T[t] // 4))), (t, len(rot))      # no set more than the windows need


# (t, index into schedules(t)): every schedule for t = 9 and 17; for t = 33 (a pyref permutation takes 4 times as long, the table
# derivation 6 times) the uniform p - 1, the first carry chain and the first and last rotation
STEERED_HOST = [(t, i) for t in (9, 17) for i in range(14)] + [(33, i) for i in (0, 5, 9, 11)]


@pytest.mark.parametrize("t,i", STEERED_HOST)
def test_steered_constants_through_the_host_kernel_bodies(hostcheck, t, i):
    """One steered set per case.  The construction: pyref.permute under the steered set ends where the walk said, and every S-box output on the
    trajectory, re-stored as fr_pow5_r29 delivers it, is its target.  The code: the kernel-form permutation (L*U rows, sparse partial rounds in
    blocks of four with their carry-free radix-2^29 accumulations), the chain model of the five-wave form (t = 17) and the sponge body of a Merkle
    level agree with pyref on the steered state / node — chosen limbs in all 72 rounds — and on 16 others under the same set; for t = 17 the
    matrix-core emulation agrees with the L*U rows and with pyref's M x on the steered S-box outputs of each of the eight full rounds."""
    base = pyref.params_for_width(t); arity = t - 1
    name, tf, tp = schedules(t)[i]
    assert len(schedules(17)) == 14 and len(schedules(9)) == 14 and len(schedules(33)) == 12
    rng = np.random.default_rng(100 * t + i)
    # ONE set per case (deriving its kernel-form tables is the larger cost at t = 33): steered for a Merkle node — permutation 1 of a full
    # node, both permutations (which = 2), or the ragged last node — whose first state is the steered state of the permutation checks
    which, kstar, last = ((1, 5, None), (2, 5, None), (1, 16, 3))[i % 3]
    nd = cv.steered_set(base, (name, tf, tp), which, 1000 + i, 2, 9, count=last)
    sp, state = nd["params"], nd["state"]
    assert sp["mds"] == base["mds"]
    of, op, end = cv.sbox_outputs(sp, state)
    assert pyref.permute(state, sp) == end, (t, name)
    assert sum(a != b for a, b in zip(sum(nd["tf"], []), sum(tf, []))) == (1 if which == 2 else 0) and (which == 1 or nd["tf"][7][:t - 1] == tf[7][:t - 1])
    for r in range(8):
        assert of[r] == nd["tf"][r], "t = %d, %s: full round %d delivers %s" % (t, name, r, ["%x" % v for v in of[r]])
    assert op == tp, (t, name)
    plain, end2 = cv.steered_params(base, state, nd["tf"], tp)
    assert plain == sp and end2 == end                                      # the node variant is steered_params on the node's first state
    h = hostcheck.params_upload(*cv.params_arrays(sp))
    try:
        mds, rcf, rcp = hostcheck.params_export(h, t, 8, sp["rp"])
        assert (rcp == cv.to_stored(sp["rc_partial"])).all() and (rcf == cv.to_stored([x for r in sp["rc_full"] for x in r])).all()
        others = [[int.from_bytes(rng.bytes(40), "little") % P for _ in range(t)] for _ in range(14)] + [[0] * t, [P - 1] * t]
        sts = [state] + others
        want = np.stack([cv.to_stored(end)] + [cv.to_stored(pyref.permute(s, sp)) for s in others])
        arr = np.stack([cv.to_stored(s) for s in sts])
        forms = [("kernel form", hostcheck.permute_kernel_form), ("dense", hostcheck.permute_dense)] + ([("chain model", hostcheck.permute_chain_model)] if t == 17 else [])
        for fname, fn in forms:
            got = fn(h, arr, t)
            bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
            assert bad.size == 0, "%s, t = %d, set '%s': state %d (0 is the steered one) differs from pyref: got %s want %s" % (
                fname, t, name, bad[0], cv.hex_limbs(got[bad[0]])[:2], cv.hex_limbs(want[bad[0]])[:2])
        ch, pos0 = cv.steered_level(base, nd, 17, kstar, last_children=last)
        assert pos0 == 1000 + i - kstar
        got = hostcheck.hash_ds_level(h, 0, arity, 2, pos0, 9, ch)
        assert got.shape[0] == 17
        assert (cv.node_digest(sp, 2, nd["pos"], 9, nd["children"]) == nd["digest"]).all()
        for k in range(17):
            w = nd["digest"] if k == kstar else cv.node_digest(sp, 2, pos0 + k, 9, ch[k * arity:(k + 1) * arity])
            assert (got[k] == w).all(), "hash_ds_level, t = %d, set '%s', permutation %d steered in node %d: node %d differs from pyref" % (t, name, which, kstar, k)
        if t == 17:
            Mpre = cv.mds_pre_canonical(base)
            x = np.stack([cv.raw_array(row) for row in nd["tf"]])             # the eight steered S-box output vectors, stored as delivered
            for pre, M in ((False, base["mds"]), (True, Mpre)):
                w = np.stack([cv.raw_array([(sum(M[a][j] * row[j] for j in range(17)) << cv.SBOX_SHIFT) % P for a in range(17)]) for row in nd["tf"]])
                a, b = hostcheck.full_round_linear(h, 0, pre, x), hostcheck.full_round_linear(h, 1, pre, x)
                for r in range(8):
                    assert (b[r] == w[r]).all(), "matrix-core path, pre = %s, set '%s', S-box outputs of full round %d: %s" % (pre, name, r, cv.hex_limbs(x[r]))
                    assert (a[r] == w[r]).all(), "L*U path, pre = %s, set '%s', S-box outputs of full round %d: %s" % (pre, name, r, cv.hex_limbs(x[r]))
    finally:
        hostcheck.params_free(h)
