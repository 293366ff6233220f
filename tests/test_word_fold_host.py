"""The word-column finish to nine limbs, host side (mfma_digits.hpp mfma_word_cols_mad / mfma_words_add_c29 / mfma_finish_words: word columns folded by
a multiply-add chain where a lane holds the sums, a quotient estimate without a carry pass, one pass over eight words, then the nine limbs of the words)
against Python big integers, for rows of 9, 17 and 23 K-steps, with and without a stored constant in the columns, to the limbs and — for the products
that end canonical — through two conditional subtractions (W is below 3 r); the S-box census at the wider range the
finish hands over; and the whole permutation in the kernels' sequence (hc_permute_block8, which runs this finish for the fused full-round rows, the H_q rows
and the last block's lane rows) against the reference's dense rounds.  CPU only.

The domain of a row is |S_c| <= K * 32 * 128 * 128.  V = k r and k 2^254 with |k| = 2^17 need |S_31| = 2^23, which 17 and 23 K-steps reach and 9 do not:
the 9-K-step rows take k = +-2^16 in their place, the largest power of two inside their domain (as tests/test_byte_finish_host.py does)."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref
import scaled_chain_lib as sc
from test_lazy_residue_host import census
from test_limb_handover_host import INV_POW5, M29, SETS17, limbs_of, limbs_value, split_digits, value
from test_partial_block8_host import states

P = pyref.P_PALLAS
R = pyref.R
KSTEPS = (9, 17, 23)
BOUND = {k: k * 32 * 128 * 128 for k in KSTEPS}
COL_BOUND = int(2 ** 47.6)               # |col| <= 16 843 009 |S| at 23 K-steps; a constant adds one word
QH_BOUND = int(2 ** 18.6)
W_LO, W_HI = P - (1 << 146), 3 * P + (1 << 146)          # the range stated next to mfma_finish_words
KS = {9: (-(1 << 16), -1, 0, 1, 1 << 16), 17: (-(1 << 17), -1, 0, 1, 1 << 17), 23: (-(1 << 17), -1, 0, 1, 1 << 17)}
DELTAS = (-3, -1, 0, 1, 3)
INT64 = 1 << 63
vp = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(vp)


def finish_words(hostcheck, sums, consts=None):
    s = np.ascontiguousarray(sums, dtype=np.int32); n = s.shape[0]
    assert s.shape == (n, 32)
    c = None if consts is None else np.ascontiguousarray([limbs_of(x) for x in consts], dtype=np.uint32)
    cols = np.zeros((n, 8), np.int64); qh = np.zeros(n, np.int32); carry = np.zeros(n, np.int64); limbs = np.zeros((n, 9), np.uint32)
    canon = np.zeros((n, 4), np.uint64)
    rc = hostcheck.l.hc_mfma_finish_words(ptr(s), ptr(c) if c is not None else None, C.c_size_t(n), ptr(cols), ptr(qh), ptr(carry), ptr(limbs), ptr(canon))
    return rc, cols, qh, carry, limbs, [cv.raw_to_int(x) for x in canon]


def check(hostcheck, cases, ksteps, consts=None):
    """the columns are the word columns of V (+ the constant's words) inside the stated bound; q^ is floor((V + c) / 2^254) or one more; every intermediate of
    the pass, recomputed here from the columns, stays inside an int64; no carry leaves word 7; the limbs are in range and are W = V + c - (q^ - 2) r exactly,
    inside (r - 2^146, 3 r + 2^146), so W == V + c (mod r) — and below 3 r, by the finer argument next to
    mfma_finish_words_canonical, whose two conditional subtractions return (V + c) mod r.  Returns the
    q^ - floor differences and the floor(W / r) seen."""
    assert all(abs(x) <= BOUND[ksteps] for s in cases for x in s)
    rc, cols, qh, carry, limbs, canon = finish_words(hostcheck, cases, consts)
    assert rc == 0, rc
    seen = set(); mult = set()
    for i, (s, col, q, cy, l, z) in enumerate(zip(cases, cols, qh, carry, limbs, canon)):
        c = 0 if consts is None else consts[i]
        V = value(s) + c
        want_cols = [s[4 * k] + 256 * s[4 * k + 1] + 65536 * s[4 * k + 2] + 16777216 * s[4 * k + 3] + ((c >> (32 * k)) & 0xffffffff) for k in range(8)]
        assert [int(x) for x in col] == want_cols and sum(x << (32 * k) for k, x in enumerate(want_cols)) == V
        assert all(abs(x) < COL_BOUND + (1 << 32) for x in want_cols), s
        fl = V >> 254
        assert int(q) in (fl, fl + 1) and abs(int(q)) < QH_BOUND, (s, int(q), fl)
        seen.add(int(q) - fl)
        q1 = int(q) - 2; t = 0; tw = [(P >> (32 * k)) & 0xffffffff for k in range(4)]
        for k in range(8):                                    # the pass, statement by statement, on unbounded integers
            for part in (want_cols[k] + t, q1 * (tw[k] if k < 4 else 0), q1 << 30 if k == 7 else 0):
                assert -INT64 <= part < INT64
            t = want_cols[k] + t - (q1 * tw[k] if k < 4 else 0) - ((q1 << 30) if k == 7 else 0)
            assert -INT64 <= t < INT64
            t >>= 32
        assert t == 0 and int(cy) == 0, (s, t, int(cy))
        W = limbs_value(l)
        assert all(int(x) <= M29 for x in l[:8]) and int(l[8]) < 1 << 24, (s, l)
        assert W == V - q1 * P and W % P == V % P, (s, hex(W))
        assert W_LO < W < W_HI and W < 1 << 256, (s, hex(W))
        assert W < 3 * P and z == V % P, (s, hex(W), hex(z))
        mult.add(W // P)
    return seen, mult


def with_consts(cases, consts):
    return [s for s in cases for _ in consts], [c for _ in cases for c in consts]


CONSTS = (0, 1, P - 1, P - (1 << 224), (1 << 254) - 1, 0x1234567 << 200)


def extreme_cases(B):
    cases = [[B] * 32, [-B] * 32, [B if c % 2 == 0 else -B for c in range(32)], [-B if c % 2 == 0 else B for c in range(32)], [0] * 32]
    for sg in itertools.product((1, -1), repeat=4):            # every sign pattern of the four sums of a word, over all words and over the top two
        cases.append([sg[c % 4] * B for c in range(32)])
        for rest in (0, B, -B):
            cases.append([rest] * 24 + [sg[c % 4] * B for c in range(8)])
    for sg in itertools.product((1, 0, -1), repeat=8):          # the top two words sum by sum, signs and zeros
        cases.append([0] * 24 + [x * B for x in sg])
    for c in (0, 23, 24, 27, 28, 31):
        for v in (1, -1, B, -B):
            s = [0] * 32; s[c] = v; cases.append(s)
    return cases


@pytest.mark.parametrize("ksteps", KSTEPS)
def test_all_sums_at_the_bound_and_sign_corners(hostcheck, ksteps):
    cases = extreme_cases(BOUND[ksteps])
    check(hostcheck, cases, ksteps)
    cs, cc = with_consts(cases[:80], CONSTS)
    check(hostcheck, cs, ksteps, cc)


def crafted_values(ksteps):
    Vs = []
    for k in KS[ksteps]:
        for d in DELTAS:
            Vs += [k * P + d, (k << 254) + d]
    # the estimate's rounding edge: x + 2 crosses a multiple of 2^30 while V has not reached the multiple of 2^254
    for k in (-1, 0, 1, 5):
        Vs += [(k << 254) - (1 << 224), (k << 254) - (2 << 224), (k << 254) - (2 << 224) - 1, (k << 254) - (3 << 224), (k << 254) - (3 << 224) + 1]
    return Vs


@pytest.mark.parametrize("ksteps", KSTEPS)
def test_crafted_multiples_and_the_rounding_edge(hostcheck, ksteps):
    """V = k r + d and k 2^254 + d, and the rounding edge of the estimate; then the same values reached as V + c with a constant below r in the columns
    (V = target - c), so that the constant carries the sum across each edge.  Both outcomes of the estimate occur, with and without a constant."""
    Vs = crafted_values(ksteps)
    cases = [split_digits(V) for V in Vs]
    assert all(value(s) == V for V, s in zip(Vs, cases))
    seen, mult = check(hostcheck, cases, ksteps)
    assert seen == {0, 1} and mult == {1, 2}          # both outcomes of the estimate; W on either side of 2 r: the second subtraction fires and idles
    cs, cc = with_consts(cases, CONSTS)
    check(hostcheck, cs, ksteps, cc)
    shifted = [(split_digits(V - c), c) for V in Vs for c in CONSTS[1:]]
    shifted = [(s, c) for s, c in shifted if all(abs(x) <= BOUND[ksteps] for x in s)]
    assert len(shifted) > len(Vs)
    seen, mult = check(hostcheck, [s for s, _ in shifted], ksteps, [c for _, c in shifted])
    assert seen == {0, 1} and mult == {1, 2}


@pytest.mark.parametrize("ksteps", KSTEPS)
def test_random_rows(hostcheck, ksteps):
    rng = random.Random(0xF01D + ksteps); B = BOUND[ksteps]
    check(hostcheck, [[rng.randint(-B, B) for _ in range(32)] for _ in range(20000)], ksteps)
    check(hostcheck, [[rng.randint(-200, 200) for _ in range(32)] for _ in range(500)], ksteps)          # small sums: V near 0, either sign
    rows = [[rng.randint(-B, B) for _ in range(32)] for _ in range(4000)] + [[rng.randint(-200, 200) for _ in range(32)] for _ in range(500)]
    check(hostcheck, rows, ksteps, [rng.choice((rng.randrange(P), P - 1 - rng.randrange(1 << 130), rng.randrange(1 << 130))) for _ in rows])


def test_rejects_rows_outside_the_form(hostcheck):
    s = [0] * 32; s[7] = BOUND[23] + 1
    assert finish_words(hostcheck, [s])[0] == -1
    s[7] = -BOUND[23]
    assert finish_words(hostcheck, [s])[0] == 0
    bad = np.zeros((1, 9), np.uint32); bad[0, 3] = 1 << 29
    out = [np.zeros((1, 8), np.int64), np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros((1, 9), np.uint32)]
    assert hostcheck.l.hc_mfma_finish_words(ptr(np.zeros((1, 32), np.int32)), ptr(bad), C.c_size_t(1), *[ptr(a) for a in out], None) == -1


X5_MAX = 104 * P // 100           # pow5_lazy29's output is below 1.04 r


def test_sbox_census_at_the_wider_range(hostcheck):
    """pow5_lazy29 at the largest u the word-column finish hands over.  The chain: u = x5 + W' limb by limb, x5 up to 1.04 r and W' up to 3 r + 2^146, and every
    limb at its maximum (x5: 2^29 - 1 with the top limb of 1.04 r; W': 2^29 - 1 with the top limb of 3 r + 2^146).  A fused row: u = W + c, c up to r - 1.  And u
    at the restated contract's own edge, 4.25 r.  The 128-bit census of the same statements: the largest column below 2^64, x2 < 1.15 r, x4 < 1.02 r, x5 < 1.04 r,
    the packed x5's top byte at most 0x42; the result congruent to u^5 / 2^(4 * 261)."""
    rng = random.Random(0xCE26)
    pairs = [([M29] * 8 + [X5_MAX >> 232], [M29] * 8 + [W_HI >> 232]), ([M29] * 8 + [(P - 1) >> 232], [M29] * 8 + [W_HI >> 232]),
             (limbs_of(X5_MAX - 1), limbs_of(W_HI - 1)), (limbs_of(P - 1), limbs_of(W_HI - 1)), (limbs_of(X5_MAX - 1), limbs_of(W_LO + 1)),
             (limbs_of(0), limbs_of(W_LO + 1)), (limbs_of(0), limbs_of(0)), (limbs_of(425 * P // 100 - 1 - (W_HI - 1)), limbs_of(W_HI - 1))]
    for x in list(cv.stored_corners(P)) + [rng.randrange(P) for _ in range(300)]:
        pairs.append((limbs_of(rng.choice((x, x + X5_MAX - P))), limbs_of(rng.randint(W_LO + 1, W_HI - 1))))
    us = [[a + b for a, b in zip(x5, w)] for x5, w in pairs]
    assert max(max(u[:8]) for u in us) == 2 * M29 < 1 << 30
    assert 405 * P // 100 > limbs_value(us[2]) > 404 * P // 100 and max(limbs_value(u) for u in us) < 425 * P // 100 + (1 << 233)
    rc, x245, colmax, tb = census(hostcheck, us)
    assert rc == 0, rc
    x2 = max(limbs_value(r[:9]) for r in x245); x4 = max(limbs_value(r[9:18]) for r in x245); x5 = max(limbs_value(r[18:]) for r in x245)
    print("largest column 2^%.3f, x2 %.4f r, x4 %.4f r, x5 %.4f r, top byte of packed x5 0x%02x" % (np.log2(float(max(colmax))), x2 / P, x4 / P, x5 / P, int(tb.max())))
    assert max(colmax) < 1 << 64
    assert x2 < 115 * P // 100 and x4 < 102 * P // 100 and x5 < 104 * P // 100 and int(tb.max()) <= 0x42
    for u, r in zip(us, x245):
        assert all(int(v) <= M29 for v in r[18:26]) and limbs_value(r[18:]) % P == pow(limbs_value(u), 5, P) * INV_POW5 % P


def check_permutation(hostcheck, h, s):
    got = b8.permute_block8(hostcheck, h, s); want = hostcheck.permute_dense(h, s, 17)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (want != s).any()


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_permutation_equals_dense_rounds(hostcheck, name):
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        check_permutation(hostcheck, h, states(470)); check_permutation(hostcheck, h, states(471))
    finally:
        hostcheck.params_free(h)


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


def test_permutation_two_full_rounds(hostcheck, base17):
    """rf = 2: no fused product; the last block's lane rows and the chain's final value feed the LAST round's S-box"""
    h = hostcheck.params_upload(*cv.params_arrays(dict(base17, rf=2, rc_full=base17["rc_full"][:2])))
    try:
        check_permutation(hostcheck, h, states(472))
    finally:
        hostcheck.params_free(h)


@pytest.mark.parametrize("r", range(8))
def test_permutation_steered_block_positions(hostcheck, base17, r):
    """chosen corners behind the S-box at every position of an 8-round block (partial_block8_lib.block8_schedule): the steered state and random states"""
    nd = cv.steered_set(base17, b8.block8_schedule(base17, r), 1, 7600 + r, 3, 42)
    h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
    try:
        check_permutation(hostcheck, h, cv.raw_array([v * R % P for v in nd["state"]]))
        check_permutation(hostcheck, h, states(480 + r)[:17 * 4])
    finally:
        hostcheck.params_free(h)


def test_permutation_uniform_corners(hostcheck, base17):
    """every uniform corner delivered by the scaled chain's S-box in all 64 rounds at once (scaled_chain_lib): the steered state and random states"""
    lam = sc.lambdas(base17["mds"], 64)
    for i, c in enumerate(cv.uniform_corners(P)):
        tp = [c * pow(pow(lam[q], 5, P), -1, P) % P for q in range(64)]
        nd = cv.steered_set(base17, ("scaled uniform", cv.target_schedules(base17)[i][1], tp), 1, 7700 + i, 3, 42)
        assert sc.scaled_chain_values(nd["params"], nd["state"])[1] == [c] * 64
        h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
        try:
            check_permutation(hostcheck, h, cv.raw_array([v * R % P for v in nd["state"]]))
            check_permutation(hostcheck, h, states(490 + i)[:17 * 4])
        finally:
            hostcheck.params_free(h)
