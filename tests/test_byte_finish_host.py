"""The byte-domain finish of the lanes between two 8-round blocks, host side (mfma_digits.hpp mfma_word_cols / mfma_finish_bytes: word columns folded
where a lane holds the sums, a quotient estimate without a carry pass, one pass over eight words) against Python big integers, in both forms — the int32
pairs of the 9-K-step lane rows and the 64-bit pairs for rows of up to 17 K-steps — and the whole permutation in the kernels' sequence (hc_permute_block8,
which runs this finish between the blocks) against the reference's dense rounds.  CPU only.

The domain of a form is |S_c| <= K * 32 * 128 * 128 (K = 9 or 17 K-steps).  V = k r and k 2^254 with |k| = 2^17 need |S_31| = 2^23, which 17 K-steps reach
and 9 do not (the largest |V| nine K-steps can form is below 2^16.2 * 2^254): the 9-K-step form takes k = +-2^16 in their place, the largest power of two
inside its domain; every other case of the set runs in both forms."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref
import scaled_chain_lib as sc
from test_limb_handover_host import SETS17, split_digits, value
from test_partial_block8_host import states

P = pyref.P_PALLAS
R = pyref.R
T_LOW = P - (1 << 254)
BOUND = {9: 9 * 32 * 128 * 128, 17: 17 * 32 * 128 * 128}
# |col| <= 65537 * 257 * |S|: below 2^46.2 for 9 K-steps; the 17-K-step form states 2^48.1 (the sums allow 2^47.1)
COL_BOUND = {9: int(2 ** 46.2), 17: int(2 ** 48.1)}
QH_BOUND = int(2 ** 18.2)
KS = {9: (-(1 << 16), -1, 0, 1, 1 << 16), 17: (-(1 << 17), -1, 0, 1, 1 << 17)}
vp = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(vp)


def finish_bytes(hostcheck, sums, ksteps):
    s = np.ascontiguousarray(sums, dtype=np.int32); n = s.shape[0]
    assert s.shape == (n, 32)
    cols = np.zeros((n, 8), np.int64); qh = np.zeros(n, np.int32); carry = np.zeros(n, np.int64); digits = np.zeros((n, 32), np.int8)
    rc = hostcheck.l.hc_mfma_finish_bytes(ptr(s), C.c_size_t(n), C.c_int(1 if ksteps == 17 else 0), ptr(cols), ptr(qh), ptr(carry), ptr(digits))
    return rc, cols, qh, carry, digits


def check(hostcheck, cases, ksteps):
    """the columns are the word columns of V inside the stated bound (and the int32 pairs of the 9-K-step form fit), q^ is floor(V / 2^254) or one more,
    no carry leaves word 7, and the 32 digits (int8: in [-128, 127] by construction) sum to W = V - q^ r exactly, so W == V (mod r)"""
    assert all(abs(x) <= BOUND[ksteps] for s in cases for x in s)
    rc, cols, qh, carry, digits = finish_bytes(hostcheck, cases, ksteps)
    assert rc == 0, rc
    assert digits.dtype == np.int8
    for s, col, q, cy, d in zip(cases, cols, qh, carry, digits):
        V = value(s)
        want_cols = [s[4 * k] + 256 * s[4 * k + 1] + 65536 * (s[4 * k + 2] + 256 * s[4 * k + 3]) for k in range(8)]
        assert [int(x) for x in col] == want_cols and sum(c << (32 * k) for k, c in enumerate(want_cols)) == V
        assert all(abs(c) < COL_BOUND[ksteps] for c in want_cols), s
        if ksteps == 9:
            assert all(abs(s[2 * i] + 256 * s[2 * i + 1]) < 1 << 31 for i in range(16)), s
        fl = V >> 254
        assert int(q) in (fl, fl + 1) and abs(int(q)) < QH_BOUND, (s, int(q), fl)
        assert int(cy) == 0, (s, int(cy))
        assert all(-128 <= int(v) <= 127 for v in d)
        W = sum(int(v) << (8 * c) for c, v in enumerate(d))
        assert W == V - int(q) * P and W % P == V % P, (s, hex(W))
        assert -P - (1 << 145) < W < (1 << 254) + (1 << 145)


@pytest.mark.parametrize("ksteps", [9, 17])
def test_all_sums_at_the_bound_and_sign_corners(hostcheck, ksteps):
    """all 32 sums at +-bound in one sign and alternating; every sign pattern of the four sums of a word (the pair and column extremes) laid over all eight
    words, and over the top two words alone with the rest at zero and at the opposite bound (the quotient estimate reads words 6 and 7); single sums"""
    B = BOUND[ksteps]
    cases = [[B] * 32, [-B] * 32, [B if c % 2 == 0 else -B for c in range(32)], [-B if c % 2 == 0 else B for c in range(32)], [0] * 32]
    for sg in itertools.product((1, -1), repeat=4):
        cases.append([sg[c % 4] * B for c in range(32)])
        for rest in (0, B, -B):
            cases.append([rest] * 24 + [sg[c % 4] * B for c in range(8)])
    for sg in itertools.product((1, 0, -1), repeat=8):          # the top two words sum by sum, signs and zeros
        cases.append([0] * 24 + [x * B for x in sg])
    for c in (0, 23, 24, 27, 28, 31):
        for v in (1, -1, B, -B):
            s = [0] * 32; s[c] = v; cases.append(s)
    check(hostcheck, cases, ksteps)


@pytest.mark.parametrize("ksteps", [9, 17])
def test_crafted_multiples(hostcheck, ksteps):
    """V = k r - 1, k r, k r + 1 and k 2^254 - 1, k 2^254, k 2^254 + 1 (the module's docstring on k), and V within 3 of the multiples"""
    Vs = []
    for k in KS[ksteps]:
        Vs += [k * P - 1, k * P, k * P + 1, (k << 254) - 1, k << 254, (k << 254) + 1, k * P - 3, k * P + 3, (k << 254) - 3, (k << 254) + 3]
    # the estimate's rounding edge: x + 2 crosses a multiple of 2^30 while V has not reached the multiple of 2^254
    for k in (-1, 0, 1, 5):
        Vs += [(k << 254) - (1 << 224), (k << 254) - (2 << 224), (k << 254) - (2 << 224) - 1, (k << 254) - (3 << 224), (k << 254) - (3 << 224) + 1]
    cases = [split_digits(V) for V in Vs]
    assert all(value(s) == V for V, s in zip(Vs, cases))
    check(hostcheck, cases, ksteps)
    qs = finish_bytes(hostcheck, cases, ksteps)[2]
    assert any(int(q) == (V >> 254) + 1 for q, V in zip(qs, Vs)) and any(int(q) == V >> 254 for q, V in zip(qs, Vs))      # both outcomes of the estimate occur


@pytest.mark.parametrize("ksteps", [9, 17])
def test_random_rows(hostcheck, ksteps):
    rng = random.Random(0xB17E + ksteps); B = BOUND[ksteps]
    check(hostcheck, [[rng.randint(-B, B) for _ in range(32)] for _ in range(20000)], ksteps)
    check(hostcheck, [[rng.randint(-200, 200) for _ in range(32)] for _ in range(500)], ksteps)          # small sums: V near 0, either sign


def test_rejects_sums_outside_the_form(hostcheck):
    s = [0] * 32; s[7] = BOUND[9] + 1
    assert finish_bytes(hostcheck, [s], 9)[0] == -1 and finish_bytes(hostcheck, [s], 17)[0] == 0
    s[7] = -(BOUND[17] + 1)
    assert finish_bytes(hostcheck, [s], 17)[0] == -1


def check_permutation(hostcheck, h, s):
    got = b8.permute_block8(hostcheck, h, s); want = hostcheck.permute_dense(h, s, 17)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (want != s).any()


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_permutation_equals_dense_rounds(hostcheck, name):
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        check_permutation(hostcheck, h, states(370)); check_permutation(hostcheck, h, states(371))
    finally:
        hostcheck.params_free(h)


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


@pytest.mark.parametrize("r", range(8))
def test_permutation_steered_block_positions(hostcheck, base17, r):
    """chosen corners behind the S-box at every position of an 8-round block (partial_block8_lib.block8_schedule): the steered state and random states"""
    nd = cv.steered_set(base17, b8.block8_schedule(base17, r), 1, 7400 + r, 3, 42)
    h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
    try:
        check_permutation(hostcheck, h, cv.raw_array([v * R % P for v in nd["state"]]))
        check_permutation(hostcheck, h, states(380 + r)[:17 * 4])
    finally:
        hostcheck.params_free(h)


def test_permutation_uniform_corners(hostcheck, base17):
    """every uniform corner delivered by the scaled chain's S-box in all 64 rounds at once (scaled_chain_lib): the steered state and random states"""
    lam = sc.lambdas(base17["mds"], 64)
    for i, c in enumerate(cv.uniform_corners(P)):
        tp = [c * pow(pow(lam[q], 5, P), -1, P) % P for q in range(64)]
        nd = cv.steered_set(base17, ("scaled uniform", cv.target_schedules(base17)[i][1], tp), 1, 7500 + i, 3, 42)
        assert sc.scaled_chain_values(nd["params"], nd["state"])[1] == [c] * 64
        h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
        try:
            check_permutation(hostcheck, h, cv.raw_array([v * R % P for v in nd["state"]]))
            check_permutation(hostcheck, h, states(390 + i)[:17 * 4])
        finally:
            hostcheck.params_free(h)
