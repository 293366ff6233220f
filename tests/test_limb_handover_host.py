"""The limb-form hand-over of the t = 17 wave-pair kernels' full rounds (poseidon_pair.hpp pair_mds_sbox_mfma), host side: the finishing step
stopped at its nine limbs (mfma_finish_limbs) over the whole stated input domain |S_c| < 2^24, the S-box on lazy limbs (sbox_lazy29) on x + k r for
every k the proven range allows with the largest column sum it reaches, the table of the round constants in limb form, and the whole permutation in
the kernels' new sequence (hc_permute_block8) against the reference's dense rounds — all against Python big integers.  CPU only."""
import ctypes as C
import random

import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref

P = pyref.P_PALLAS
R = pyref.R
SETS17 = {"merkle": (0, b""), "transcript": (1, b""), "bench": (2, b"POSEIDON-T17-X5")}
LIM = (1 << 24) - 1                      # the finishing step's domain: |S_c| <= 2^24 - 1
M29 = (1 << 29) - 1
# W = (V mod 2^254) + 2^254 - q1 t with |q1| < 2^18.02 and t = r - 2^254 < 2^126: the range stated next to mfma_finish_limbs, rounded outwards
W_LO, W_HI = (1 << 254) - (1 << 145), (1 << 255) + (1 << 145)
INV_POW5 = pow(pow(2, 261, P), -4, P)    # fr_pow5_r29: x^2 / 2^261, its square / 2^261, x times that / 2^261 = x^5 / 2^(4 * 261)


def value(sums):
    return sum(int(s) << (8 * c) for c, s in enumerate(sums))


def split_digits(V):
    """V (any sign) -> 32 digit sums with V = sum S_c 256^c: signed radix-256 digits at c < 31, S_31 carries the surplus"""
    S = []
    for _ in range(31):
        d = ((V + 128) & 0xff) - 128
        S.append(d); V = (V - d) >> 8
    S.append(V)
    return S


def limbs_value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def limbs_of(v):
    """the normalised nine limbs of 0 <= v < 2^261"""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def finish_limbs(hostcheck, sums):
    s = np.ascontiguousarray(sums, dtype=np.int32)
    assert s.ndim == 2 and s.shape[1] == 32
    out = np.zeros((s.shape[0], 9), np.uint32)
    rc = hostcheck.l.hc_mfma_finish_limbs(s.ctypes.data_as(C.c_void_p), C.c_size_t(s.shape[0]), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


def finish(hostcheck, sums):
    s = np.ascontiguousarray(sums, dtype=np.int32)
    out = np.zeros((s.shape[0], 4), np.uint64)
    assert hostcheck.l.hc_mfma_finish(s.ctypes.data_as(C.c_void_p), C.c_size_t(s.shape[0]), out.ctypes.data_as(C.c_void_p)) == 0
    return [cv.raw_to_int(x) for x in out]


def check_finish_limbs(hostcheck, cases):
    got = finish_limbs(hostcheck, cases); canon = finish(hostcheck, cases)
    for s, l, z in zip(cases, got, canon):
        W = limbs_value(l)
        assert all(int(x) <= M29 for x in l[:8]) and int(l[8]) < 1 << 24, (s, l)
        assert W_LO < W < W_HI and 0 < W < 3 * P, (s, hex(W))
        assert W % P == value(s) % P == z, s


def test_finish_to_limbs_extremes_and_single_sums(hostcheck):
    cases = [[LIM] * 32, [-LIM] * 32, [LIM if c % 2 == 0 else -LIM for c in range(32)], [-LIM if c % 2 == 0 else LIM for c in range(32)], [0] * 32]
    for c in (0, 31):
        for v in (1, -1, LIM, -LIM, 8912896, -8912896):
            s = [0] * 32; s[c] = v; cases.append(s)
    check_finish_limbs(hostcheck, cases)


def test_finish_to_limbs_crafted_multiples(hostcheck):
    """V = k r - 1, k r, k r + 1 and k 2^254 - 1, k 2^254, k 2^254 + 1 for k in {-2^17, -1, 0, 1, 2^17}: both ends of W's range"""
    Vs = []
    for k in (-(1 << 17), -1, 0, 1, 1 << 17):
        Vs += [k * P - 1, k * P, k * P + 1, (k << 254) - 1, k << 254, (k << 254) + 1]
    cases = [split_digits(V) for V in Vs]
    for V, s in zip(Vs, cases):
        assert value(s) == V and all(-128 <= d <= 127 for d in s[:31]) and abs(s[31]) < 1 << 24
    check_finish_limbs(hostcheck, cases)


def test_finish_to_limbs_random(hostcheck):
    rng = random.Random(0x11B5)
    check_finish_limbs(hostcheck, [[rng.randint(-LIM, LIM) for _ in range(32)] for _ in range(20000)])


def test_finish_to_limbs_rejects_sums_outside_its_domain(hostcheck):
    s = np.zeros((1, 32), np.int32); s[0, 5] = -(1 << 24)
    out = np.zeros((1, 9), np.uint32)
    assert hostcheck.l.hc_mfma_finish_limbs(s.ctypes.data_as(C.c_void_p), C.c_size_t(1), out.ctypes.data_as(C.c_void_p)) == -1


def sbox_lazy(hostcheck, l, c):
    l = np.ascontiguousarray(l, dtype=np.uint32); c = np.ascontiguousarray(c, dtype=np.uint32)
    assert l.shape == c.shape and l.shape[1] == 9
    out = np.zeros((l.shape[0], 4), np.uint64); cm = np.zeros((l.shape[0], 2), np.uint64)
    rc = hostcheck.l.hc_sbox_lazy29(l.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), C.c_size_t(l.shape[0]), out.ctypes.data_as(C.c_void_p), cm.ctypes.data_as(C.c_void_p))
    return rc, [cv.raw_to_int(x) for x in out], [int(a) | (int(b) << 64) for a, b in cm]


def test_sbox_on_lazy_limbs(hostcheck):
    """u = x + k r for k = 0..3 (the proven range: u below 4r), x the stored corners and seeded random values, handed over as a finish part l below 3r
    and a constant c below r in every split the kernels can meet (c = 0, c as large as the split allows, random), and every limb at its maximum
    (l_i = c_i = 2^29 - 1 with the top limbs at the ends of their ranges): the result is fr_pow5_r29 of the canonical value, and the largest column
    the three steps reach in 128-bit arithmetic stays below 2^64."""
    rng = random.Random(0x5B0C)
    xs = list(cv.stored_corners(P)) + [rng.randrange(P) for _ in range(300)]
    L, Cc, U = [], [], []
    for x in xs:
        for k in range(4):
            u = x + k * P
            lo, hi = max(0, u - 3 * P + 1), min(P - 1, u)
            if lo > hi:                   # u = 4r - 1: not a sum of a part below 3r and a constant below r
                continue
            for c in {lo, hi, rng.randint(lo, hi)}:
                L.append(limbs_of(u - c)); Cc.append(limbs_of(c)); U.append(u)
    for l8 in (0, 1 << 22, 3 * (1 << 22) - 1):
        for c8 in (0, (1 << 22) - 1):
            l = [M29] * 8 + [l8]; c = [M29] * 8 + [c8]
            assert limbs_value(l) < 3 * P and limbs_value(c) < P
            L.append(l); Cc.append(c); U.append(limbs_value(l) + limbs_value(c))
    assert max(U) < 4 * P and max(max(a + b for a, b in zip(l[:8], c[:8])) for l, c in zip(L, Cc)) == 2 * M29
    rc, got, colmax = sbox_lazy(hostcheck, L, Cc)
    assert rc == 0, rc
    print("largest column: 2^%.3f" % np.log2(float(max(colmax))))
    assert max(colmax) < 1 << 64
    canon = {}
    for u, g in zip(U, got):
        x = u % P
        if x not in canon:
            canon[x] = cv.raw_to_int(hostcheck.fr_op(0, 8, cv.raw(x)))
            assert canon[x] == pow(x, 5, P) * INV_POW5 % P
        assert g == canon[x], hex(u)


def test_sbox_on_lazy_limbs_rejects_limbs_outside_its_domain(hostcheck):
    l = [[0] * 9, [0] * 8 + [1 << 24]]; c = [[1 << 29] + [0] * 8, [0] * 9]
    for i in range(2):
        assert sbox_lazy(hostcheck, [l[i]], [c[i]])[0] == -1


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_round_constants_in_limb_form(hostcheck, name):
    """rc_full29: nine 29-bit limbs of every full-round constant AS STORED (not the R' domain of the multiplier tables)"""
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        _, rcf, _ = hostcheck.params_export(h, 17, 8, 64)
        hostcheck.l.hc_rc_full29_table.restype = C.c_size_t
        n = hostcheck.l.hc_rc_full29_table(h, None, C.c_size_t(0))
        assert n == 8 * 17 * 9
        tab = np.zeros(n, np.uint32)
        assert hostcheck.l.hc_rc_full29_table(h, tab.ctypes.data_as(C.c_void_p), C.c_size_t(n)) == n
        for i, l in enumerate(tab.reshape(-1, 9)):
            assert [int(x) for x in l] == limbs_of(cv.raw_to_int(rcf[i])), i
    finally:
        hostcheck.params_free(h)


def states(seed):
    rng = np.random.default_rng(seed)
    rows = [[int.from_bytes(rng.bytes(40), "little") % P for _ in range(17)] for _ in range(3)] + [[0] * 17, [P - 1] * 17, [(P - 1) if j % 2 else 0 for j in range(17)]]
    return cv.raw_array([v for row in rows for v in row])


def check_set(hostcheck, h, extra=None):
    for s in [states(29)] + ([extra] if extra is not None else []):
        got = b8.permute_block8(hostcheck, h, s); want = hostcheck.permute_dense(h, s, 17)
        assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
        assert (want != s).any()


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_permutation_in_the_new_sequence_equals_dense_rounds(hostcheck, name):
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        check_set(hostcheck, h)
    finally:
        hostcheck.params_free(h)


@pytest.mark.parametrize("which,r", [(1, 0), (2, 3)])
def test_permutation_in_the_new_sequence_equals_dense_rounds_steered_sets(hostcheck, which, r):
    """the steered sets of tests/test_partial_block8_host.py: chosen corners behind every S-box, the fused ones included, and the steered state itself"""
    base = pyref.params_for_width(17)
    sc = cv.target_schedules(base)
    nd = cv.steered_set(base, sc[len(cv.uniform_corners(P)) + r], which, 7000 + r, 3, 42)
    h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
    try:
        check_set(hostcheck, h, cv.raw_array([v * R % P for v in nd["state"]]))
    finally:
        hostcheck.params_free(h)


def test_permutation_in_the_new_sequence_with_two_full_rounds(hostcheck):
    """rf = 2: half = rf - 1, no fused product at all — the first S-box, the product in front of the partial rounds, the S-box after them and the last product"""
    base = pyref.params_for_width(17)
    h = hostcheck.params_upload(*cv.params_arrays(dict(base, rf=2, rc_full=base["rc_full"][:2])))
    try:
        check_set(hostcheck, h)
    finally:
        hostcheck.params_free(h)
