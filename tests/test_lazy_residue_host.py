"""The lazy chain of the 8-round partial blocks, host side (mfma_digits.hpp: the finish with the next round's constant in its columns, the mailbox slot of
nine limbs, the unreduced recode of an S-box output, the S-box on x5 + W' without a canonical value) against Python big integers, and the whole
permutation in the kernels' sequence (hc_permute_block8) against the reference's dense rounds.  CPU only."""
import ctypes as C
import random

import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref
import scaled_chain_lib as sc
from test_limb_handover_host import INV_POW5, LIM, M29, SETS17, W_HI, W_LO, limbs_of, limbs_value, split_digits, value
from test_partial_block8_host import states

P = pyref.P_PALLAS
R = pyref.R
vp = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(vp)


def finish_c(hostcheck, sums, consts):
    s = np.ascontiguousarray(sums, dtype=np.int32); c = np.ascontiguousarray([limbs_of(x) for x in consts], dtype=np.uint32)
    assert s.shape == (c.shape[0], 32)
    limbs = np.zeros((s.shape[0], 9), np.uint32); slots = np.zeros((s.shape[0], 8), np.uint32)
    assert hostcheck.l.hc_mfma_finish_limbs_c(ptr(s), ptr(c), C.c_size_t(s.shape[0]), ptr(limbs), ptr(slots)) == 0
    return limbs, slots


def add_slot(hostcheck, x5, slots):
    x5 = np.ascontiguousarray(x5, dtype=np.uint32); u = np.zeros_like(x5)
    hostcheck.l.hc_lazy29_add_slot(ptr(x5), ptr(np.ascontiguousarray(slots, dtype=np.uint32)), C.c_size_t(x5.shape[0]), ptr(u))
    return u


def check_finish_c(hostcheck, cases, consts):
    """W' == V + c (mod r), inside the range stated next to the finish, limbs in range; the slot's words return the same nine limbs"""
    limbs, slots = finish_c(hostcheck, cases, consts)
    back = add_slot(hostcheck, np.zeros_like(limbs), slots)
    for s, c, l, w, b in zip(cases, consts, limbs, slots, back):
        W = limbs_value(l)
        assert all(int(x) <= M29 for x in l[:8]) and int(l[8]) < 1 << 24, (s, l)
        assert W_LO < W < W_HI and W < 1 << 256, (s, hex(W))
        assert W % P == (value(s) + c) % P, (s, c)
        assert W == value(s) + c - (((value(s) + c) >> 254) - 1) * P            # q1 is taken after the constant is in
        assert [int(x) for x in b] == [int(x) for x in l]
        assert [int(x) & M29 for x in w] == [int(x) for x in l[:8]] and sum((int(x) >> 29) << (3 * k) for k, x in enumerate(w)) == int(l[8])


CONSTS = (0, 1, P - 1)


def test_finish_with_constant_extreme_patterns(hostcheck):
    """every digit-sum pattern with |S_c| = 2^24 - 1, and single sums at both ends, with the constants 0, 1 and r - 1"""
    pats = [[LIM] * 32, [-LIM] * 32, [LIM if c % 2 == 0 else -LIM for c in range(32)], [-LIM if c % 2 == 0 else LIM for c in range(32)], [0] * 32]
    for c in (0, 31):
        for v in (LIM, -LIM):
            s = [0] * 32; s[c] = v; pats.append(s)
    check_finish_c(hostcheck, [p for p in pats for _ in CONSTS], [c for _ in pats for c in CONSTS])


def test_finish_with_constant_crafted_multiples(hostcheck):
    """V = k r - 1, k r, k r + 1 and k 2^254 - 1, k 2^254, k 2^254 + 1 for k in {-2^17, -1, 0, 1, 2^17}: the constant carries V + c across each edge"""
    Vs = []
    for k in (-(1 << 17), -1, 0, 1, 1 << 17):
        Vs += [k * P - 1, k * P, k * P + 1, (k << 254) - 1, k << 254, (k << 254) + 1]
    cases = [split_digits(V) for V in Vs]
    assert all(value(s) == V for V, s in zip(Vs, cases))
    check_finish_c(hostcheck, [s for s in cases for _ in CONSTS], [c for _ in cases for c in CONSTS])


def test_finish_with_constant_random(hostcheck):
    rng = random.Random(0x1A2B)
    cases = [[rng.randint(-LIM, LIM) for _ in range(32)] for _ in range(20000)]
    check_finish_c(hostcheck, cases, [rng.choice((0, 1, P - 1, rng.randrange(P))) for _ in cases])


def test_finish_with_constant_rejects_inputs_outside_its_domain(hostcheck):
    s = np.zeros((1, 32), np.int32); c = np.zeros((1, 9), np.uint32); c[0, 8] = 1 << 23
    limbs = np.zeros((1, 9), np.uint32); slots = np.zeros((1, 8), np.uint32)
    assert hostcheck.l.hc_mfma_finish_limbs_c(ptr(s), ptr(c), C.c_size_t(1), ptr(limbs), ptr(slots)) == -1


def finish_recoded(hostcheck, sums):
    s = np.ascontiguousarray(sums, dtype=np.int32)
    limbs = np.zeros((s.shape[0], 9), np.uint32); digits = np.zeros((s.shape[0], 32), np.int8)
    assert hostcheck.l.hc_mfma_finish_recoded(ptr(s), C.c_size_t(s.shape[0]), ptr(limbs), ptr(digits)) == 0
    return limbs, digits


def check_finish_recoded(hostcheck, cases):
    """the lanes between two blocks: W = V - floor(V / 2^254) r inside (-2^145, 2^254 + 2^145), and 32 digits in [-128, 127] (int8 by construction) whose
    weighted sum is exactly W"""
    limbs, digits = finish_recoded(hostcheck, cases)
    t = P - (1 << 254)
    for s, l, d in zip(cases, limbs, digits):
        V = value(s); W = V - (V >> 254) * P
        assert W == (V & ((1 << 254) - 1)) - (V >> 254) * t and -(1 << 145) < W < (1 << 254) + (1 << 145)
        top = int(l[8]) - (1 << 32) if int(l[8]) >> 31 else int(l[8])
        assert all(int(x) <= M29 for x in l[:8]) and -1 <= top <= 1 << 22 and limbs_value(list(l[:8]) + [top]) == W, (s, l)
        assert sum(int(v) << (8 * c) for c, v in enumerate(d)) == W, (s, hex(W))


def test_floor_quotient_finish_and_signed_recode(hostcheck):
    """the extreme digit-sum patterns, V = k r + {-1, 0, 1} and k 2^254 + {-1, 0, 1} for k in {-2^17, -1, 0, 1, 2^17}, V chosen so that W is -1, 0 and
    2^254, and 20 000 random cases"""
    rng = random.Random(0xF100)
    t = P - (1 << 254)
    pats = [[LIM] * 32, [-LIM] * 32, [LIM if c % 2 == 0 else -LIM for c in range(32)], [-LIM if c % 2 == 0 else LIM for c in range(32)], [0] * 32]
    Vs = []
    for k in (-(1 << 17), -1, 0, 1, 1 << 17):
        Vs += [k * P - 1, k * P, k * P + 1, (k << 254) - 1, k << 254, (k << 254) + 1]
    # W = (V mod 2^254) - q t with q = floor(V / 2^254): W = -1 (q = 1, low part t - 1) and W = 2^254 (q = -1, low part 2^254 - t) through the finish itself
    Vs += [(1 << 254) + t - 1, -(1 << 254) + (1 << 254) - t]
    cases = pats + [split_digits(V) for V in Vs]
    got = {value(s) - (value(s) >> 254) * P for s in cases}
    assert {-1, 0, 1 << 254}.issubset(got)
    check_finish_recoded(hostcheck, cases + [[rng.randint(-LIM, LIM) for _ in range(32)] for _ in range(20000)])


def test_signed_residue_recode_is_exact(hostcheck):
    """recode_signed on the sign-extended pack of W, at and beyond both ends of the finish's range (-2^144.02, 2^254 + 2^144.02): W = -1, -2^144, 0, 2^254 and
    2^254 + 2^144 - 1, their neighbours and seeded values in between: 32 digits in [-128, 127] (int8) whose weighted sum is W itself"""
    rng = random.Random(0x51ED)
    Ws = [-1, -2, -(1 << 144), -(1 << 144) - 1, 0, 1, 1 << 254, (1 << 254) + (1 << 144) - 1, (1 << 254) + (1 << 144), (1 << 254) - 1]
    Ws += [rng.randint(-(1 << 145), (1 << 254) + (1 << 145)) for _ in range(2000)] + [-rng.randrange(1 << 145) for _ in range(500)]
    l = np.ascontiguousarray([[(W >> (29 * i)) & M29 for i in range(8)] + [(W >> 232) & 0xffffffff] for W in Ws], dtype=np.uint32)
    d = np.zeros((len(Ws), 32), np.int8)
    hostcheck.l.hc_recode_lazy29(ptr(l), C.c_size_t(len(Ws)), ptr(d))
    for W, dig in zip(Ws, d):
        assert sum(int(v) << (8 * c) for c, v in enumerate(dig)) == W, hex(W)


X5_MAX = 104 * P // 100           # pow5_lazy29's output is below 1.04 r


def test_unreduced_recode_is_exact(hostcheck):
    """recode_lazy29 on x5 in [0, 1.04 r): 32 digits in [-128, 127] whose weighted sum is x5 itself (not x5 mod r); the top byte of 1.04 r is 0x42, so the
    0x80 added to it never carries out"""
    rng = random.Random(0x7EC0)
    xs = [0, 1, P - 1, P, P + 1, X5_MAX - 1, (1 << 254) - 1, 1 << 254, int("7f" * 31, 16), int("80" * 31, 16)] + [rng.randrange(X5_MAX) for _ in range(2000)]
    assert (X5_MAX >> 248) == 0x42
    l = np.ascontiguousarray([limbs_of(x) for x in xs], dtype=np.uint32); d = np.zeros((len(xs), 32), np.int8)
    hostcheck.l.hc_recode_lazy29(ptr(l), C.c_size_t(len(xs)), ptr(d))
    for x, dig in zip(xs, d):
        assert sum(int(v) << (8 * c) for c, v in enumerate(dig)) == x, hex(x)


def census(hostcheck, us):
    u = np.ascontiguousarray(us, dtype=np.uint32)
    x245 = np.zeros((u.shape[0], 27), np.uint32); cm = np.zeros((u.shape[0], 2), np.uint64); tb = np.zeros(u.shape[0], np.uint8)
    rc = hostcheck.l.hc_chain_census(ptr(u), C.c_size_t(u.shape[0]), ptr(x245), ptr(cm), ptr(tb))
    return rc, x245, [int(a) | (int(b) << 64) for a, b in cm], tb


def test_chain_sbox_census(hostcheck):
    """pow5_lazy29 on u = x5 + W' limb by limb: every limb at its maximum (x5: 2^29 - 1 with the top limb of 1.04 r; W': 2^29 - 1 with the top limb at the
    top of its range), x5 = 1.04 r with W' at both ends of its range, the stored corners plus multiples of r, and seeded random pairs.  The 128-bit census
    of the same statements: the largest column stays below 2^64, x2 < 1.08 r, x4 < 1.01 r, x5 < 1.03 r, the top byte of the packed x5 at most 0x42; the
    result is congruent to u^5 / 2^(4 * 261)."""
    rng = random.Random(0xCE25)
    pairs = [([M29] * 8 + [X5_MAX >> 232], [M29] * 8 + [(W_HI >> 232)]),
             (limbs_of(X5_MAX - 1), limbs_of(W_HI - 1)), (limbs_of(X5_MAX - 1), limbs_of(W_LO + 1)), (limbs_of(0), limbs_of(W_LO + 1)), (limbs_of(0), limbs_of(0))]
    for x in list(cv.stored_corners(P)) + [rng.randrange(P) for _ in range(300)]:
        pairs.append((limbs_of(rng.choice((x, x + X5_MAX - P))), limbs_of(rng.randint(W_LO + 1, W_HI - 1))))
    us = [[a + b for a, b in zip(x5, w)] for x5, w in pairs]
    assert max(max(u[:8]) for u in us) == 2 * M29 < 1 << 30 and max(limbs_value(u) for u in us) < 305 * P // 100
    rc, x245, colmax, tb = census(hostcheck, us)
    assert rc == 0, rc
    x2 = max(limbs_value(r[:9]) for r in x245); x4 = max(limbs_value(r[9:18]) for r in x245); x5 = max(limbs_value(r[18:]) for r in x245)
    print("largest column 2^%.3f, x2 %.4f r, x4 %.4f r, x5 %.4f r, top byte of packed x5 0x%02x" % (np.log2(float(max(colmax))), x2 / P, x4 / P, x5 / P, int(tb.max())))
    assert max(colmax) < 1 << 64
    assert x2 < 108 * P // 100 and x4 < 101 * P // 100 and x5 < 103 * P // 100 and int(tb.max()) <= 0x42 < 0x7f
    for u, r in zip(us, x245):
        assert all(int(v) <= M29 for v in r[18:26]) and limbs_value(r[18:]) % P == pow(limbs_value(u), 5, P) * INV_POW5 % P
    assert census(hostcheck, [[1 << 30] + [0] * 8])[0] == -1


def test_scaled_constants_in_limb_form(hostcheck):
    """rc_partial_scaled29: rp + 1 entries, entry q the nine 29-bit limbs of the stored lambda_q c_q (table 7), the last entry zero"""
    h = hostcheck.params(0, 17, b"")
    try:
        hostcheck.l.hc_rc_partial_scaled29_table.restype = C.c_size_t
        n = hostcheck.l.hc_rc_partial_scaled29_table(h, None, C.c_size_t(0))
        assert n == 65 * 9
        tab = np.zeros(n, np.uint32)
        assert hostcheck.l.hc_rc_partial_scaled29_table(h, ptr(tab), C.c_size_t(n)) == n
        stored = [cv.raw_to_int(x) for x in sc.raw_table(hostcheck, h, 7).view(np.uint64).reshape(-1, 4)]
    finally:
        hostcheck.params_free(h)
    tab = tab.reshape(65, 9)
    assert [limbs_value(r) for r in tab[:64]] == stored and not tab[64].any() and all(int(v) <= M29 for r in tab for v in r)


def check(hostcheck, h, s):
    got = b8.permute_block8(hostcheck, h, s); want = hostcheck.permute_dense(h, s, 17)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (want != s).any()


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_lazy_chain_permutation_equals_dense_rounds(hostcheck, name):
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        check(hostcheck, h, states(270)); check(hostcheck, h, states(271))
    finally:
        hostcheck.params_free(h)


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


def test_lazy_chain_permutation_two_full_rounds(hostcheck, base17):
    """rf = 2: the chain's final value feeds the LAST round's S-box"""
    h = hostcheck.params_upload(*cv.params_arrays(dict(base17, rf=2, rc_full=base17["rc_full"][:2])))
    try:
        check(hostcheck, h, states(272))
    finally:
        hostcheck.params_free(h)


@pytest.mark.parametrize("side", ["out", "in"])
def test_lazy_chain_permutation_uniform_corners(hostcheck, base17, side):
    """every uniform corner delivered (out) or read mod r (in) by the chain's S-box in all 64 rounds at once: the steered state and random states"""
    lam = sc.lambdas(base17["mds"], 64); Ri = pow(R, -1, P)
    for i, c in enumerate(cv.uniform_corners(P)):
        if side == "out":
            tp = [c * pow(pow(lam[q], 5, P), -1, P) % P for q in range(64)]
        else:
            tp = [cv.restored(pow(c * Ri % P * pow(lam[q], -1, P) % P, 5, P)) for q in range(64)]
        nd = cv.steered_set(base17, ("scaled uniform", cv.target_schedules(base17)[i][1], tp), 1, 7300 + i, 3, 42)
        ins, outs = sc.scaled_chain_values(nd["params"], nd["state"])
        assert (outs if side == "out" else ins) == [c] * 64
        h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
        try:
            check(hostcheck, h, cv.raw_array([v * R % P for v in nd["state"]]))
            check(hostcheck, h, states(280 + i)[:17 * 4])      # four whole states
        finally:
            hostcheck.params_free(h)
