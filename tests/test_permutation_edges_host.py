"""The once-per-permutation edges of the t = 17 wave-pair kernels on the row pipeline, host side, against Python big integers:

* the leaf's round 0 as a product of two K-steps (poseidon_pair.hpp pair_leaf_round0_mfma, re-enacted by hc_leaf_round0 with the statements of
  mfma_digits.hpp): the table (K_i + round 1's constant) that ctx_leaf_init uploads, the rows' finish limbs plus that table against the dense round 0
  followed by round 1's constant add, and round 1's S-box on them — over random (f, f_next), the zero f_next, and inputs whose x4 / x5 are the uniform
  corners (by the fifth root);
* the squeeze row as one matrix-core row (pair_squeeze_row_mfma, hc_squeeze_row): row 0 of the fragment table against the field row `row0`, and the
  emulated 17-K-step row with the canonical finish against the row0 dot product;
* the entry to the partial rounds (pair_mds_sbox_mfma, entry): mfma_finish_bytes on 17-K-step columns folded by the multiply-add chain
  (hc_mfma_finish_bytes_mad) — digits that sum to a value congruent to the canonical finish.

CPU only."""
import ctypes as C
import random

import numpy as np
import pytest

import corner_values as cv
import pyref
from test_limb_handover_host import INV_POW5, M29, SETS17, finish, limbs_of, limbs_value, split_digits, value

P = pyref.P_PALLAS
R = pyref.R
RI = pow(R, -1, P)
W_LO, W_HI = P - (1 << 146), 3 * P + (1 << 146)          # the range stated next to mfma_finish_words
vp = C.c_void_p


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def ints(a):
    return [cv.raw_to_int(x) for x in np.asarray(a, np.uint64).reshape(-1, 4)]


@pytest.fixture(scope="module")
def tset(hostcheck):
    """the transcript set (hash_leaf_pair's): the handle and its constants as STORED integers (mds [17][17], rc_full [8][17])"""
    kind, seed = SETS17["transcript"]
    h = hostcheck.params(kind, 17, seed)
    mds, rcf, _ = hostcheck.params_export(h, 17, 8, 64)
    mds = ints(mds); rcf = ints(rcf)
    yield h, [mds[17 * i:17 * i + 17] for i in range(17)], [rcf[17 * r:17 * r + 17] for r in range(8)]
    hostcheck.params_free(h)


def leaf_round0(hostcheck, h, f, fn):
    f = np.ascontiguousarray(cv.raw_array(f)); n = f.shape[0]
    fn = None if fn is None else np.ascontiguousarray(cv.raw_array(fn))
    init = np.zeros((17, 4), np.uint64); tab = np.zeros((17, 9), np.uint32); x45 = np.zeros((n, 2, 4), np.uint64)
    limbs = np.zeros((n, 17, 9), np.uint32); sbox = np.zeros((n, 17, 4), np.uint64)
    rc = hostcheck.l.hc_leaf_round0(h, ptr(f), ptr(fn), C.c_size_t(n), ptr(init), ptr(tab), ptr(x45), ptr(limbs), ptr(sbox))
    assert rc == 0, rc
    return ints(init), tab, [ints(x) for x in x45], limbs, [ints(x) for x in sbox]


def pow5_stored(x):
    """fr_pow5_r29 on a stored value (any representative): the stored limbs of x^5 / 2^20"""
    return pow(x, 5, P) * INV_POW5 % P


def check_round0(hostcheck, tset, f, fn):
    """returns the (x4, x5) the S-boxes delivered, as stored integers"""
    h, M, rc = tset
    init, tab, x45, limbs, sbox = leaf_round0(hostcheck, h, f, fn)
    assert init[4] == 0 and init[5] == 0 and init[16] != 0
    # stored domain throughout: M is stored (M R), so M_stored * RI * y_stored is the stored form of M y; y_stored = stored of the logical x^5
    y0 = [pow5_stored((init[j] + rc[0][j]) % P) * (1 << cv.SBOX_SHIFT) % P for j in range(17)]
    K = [sum(M[i][j] * RI % P * y0[j] for j in range(17) if j not in (4, 5)) % P for i in range(17)]
    for i in range(17):
        assert [int(x) for x in tab[i]] == limbs_of((K[i] + rc[1][i]) % P), i
    for s in range(len(f)):
        x4 = pow5_stored((f[s] + rc[0][4]) % P); x5 = pow5_stored(((0 if fn is None else fn[s]) + rc[0][5]) % P)
        assert x45[s] == [x4, x5]
        for i in range(17):
            dense = (K[i] + M[i][4] * RI % P * (x4 << cv.SBOX_SHIFT) + M[i][5] * RI % P * (x5 << cv.SBOX_SHIFT)) % P          # round 0, dense, stored
            l = limbs[s][i]; W = limbs_value(l)
            assert all(int(v) <= M29 for v in l[:8]) and int(l[8]) < 1 << 24 and W_LO < W < W_HI, (s, i, hex(W))
            u = W + limbs_value(tab[i])
            assert u < 4 * P + (1 << 147) and all(int(a) + int(b) < 1 << 30 for a, b in zip(l, tab[i]))          # pow5_lazy29's contract, the fused rows' bound
            assert u % P == (dense + rc[1][i]) % P, (s, i)
            assert sbox[s][i] == pow5_stored(u % P), (s, i)
    return x45


def test_round0_dense_check_is_the_reference_round(hostcheck, tset):
    """the dense round 0 restated in check_round0 is the one hc_permute_dense runs: same state after round 0's product, by the S-box outputs of round 1 it implies"""
    h, M, rc = tset
    init = leaf_round0(hostcheck, h, [1], [2])[0]
    f, fn = 0x1234567 * R % P, 0x7654321 * R % P
    st = list(init); st[4] = f; st[5] = fn
    y0 = [pow5_stored((st[j] + rc[0][j]) % P) * (1 << cv.SBOX_SHIFT) % P for j in range(17)]
    s1 = [sum(M[i][j] * RI % P * y0[j] for j in range(17)) % P for i in range(17)]
    # pyref's permutation on the logical values, stopped after round 0
    lg = lambda v: v * RI % P
    par = dict(t=17, rf=8, rp=64, mds=[[lg(x) for x in row] for row in M], rc_full=[[lg(x) for x in r] for r in rc], rc_partial=[0] * 64)
    s = [pow((lg(st[j]) + par["rc_full"][0][j]) % P, 5, P) for j in range(17)]
    want = [sum(par["mds"][i][j] * s[j] for j in range(17)) % P * R % P for i in range(17)]
    assert s1 == want


def test_round0_random_inputs(hostcheck, tset):
    rng = random.Random(0xED6E0)
    f = [rng.randrange(P) for _ in range(40)]; fn = [rng.randrange(P) for _ in range(40)]
    check_round0(hostcheck, tset, f, fn)
    check_round0(hostcheck, tset, f + [0, P - 1], None)                  # f_next == nullptr: the zero input
    check_round0(hostcheck, tset, [0, P - 1, 0, P - 1], [0, 0, P - 1, P - 1])


def test_round0_uniform_corners_behind_the_first_sbox(hostcheck, tset):
    """x4 and x5 each every uniform corner (all pairs), placed by the fifth root"""
    h, M, rc = tset
    corners = cv.uniform_corners(P)
    pre4 = [cv.sbox_preimage(c, rc[0][4]) for c in corners]; pre5 = [cv.sbox_preimage(c, rc[0][5]) for c in corners]
    f = [a for a in pre4 for _ in pre5]; fn = [b for _ in pre4 for b in pre5]
    x45 = check_round0(hostcheck, tset, f, fn)
    assert x45 == [[a, b] for a in corners for b in corners]
    x45 = check_round0(hostcheck, tset, pre4, None)
    assert [x[0] for x in x45] == corners


# ---- the squeeze row -------------------------------------------------------------------------------------------------------------------------------
def row0_of(hostcheck, h):
    hostcheck.l.hc_row0_table.restype = C.c_size_t
    out = np.zeros((17, 4), np.uint64)
    assert hostcheck.l.hc_row0_table(h, ptr(out), C.c_size_t(17)) == 17
    return ints(out)


def squeeze_row(hostcheck, h, states):
    s = np.ascontiguousarray(cv.raw_array([v for st in states for v in st])); n = len(states)
    out = np.zeros((n, 4), np.uint64)
    rc = hostcheck.l.hc_squeeze_row(h, ptr(s), C.c_size_t(n), ptr(out))
    assert rc == 0, rc
    return ints(out)


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_fragment_row0_is_the_field_row(hostcheck, name):
    """fragment (0, e), input digit position b: signed digits of (row0[e] * 2^20 * 256^b) mod r, the plain integer"""
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        row0 = row0_of(hostcheck, h)
        mds, _, _ = hostcheck.params_export(h, 17, 8, 64)
        assert row0 == ints(mds)[:17]
        hostcheck.l.hc_mfma_frag_table.restype = C.c_size_t
        frag = np.zeros(17 * 17 * 1024, np.int8)
        assert hostcheck.l.hc_mfma_frag_table(h, 0, ptr(frag), C.c_size_t(frag.size)) == frag.size
        fr = frag.reshape(17, 17, 64, 16)[0]
        for e in range(17):
            coeff = row0[e] * RI % P * (1 << cv.SBOX_SHIFT) % P
            for b in range(32):
                digits = [int(fr[e, c + 32 * (b >> 4), b & 15]) for c in range(32)]
                assert sum(d << (8 * c) for c, d in enumerate(digits)) == coeff * pow(256, b, P) % P, (e, b)
    finally:
        hostcheck.params_free(h)


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_squeeze_row_equals_row0_dot_product(hostcheck, name):
    """random states of S-box outputs, every uniform corner in all 17 elements at once and alternating with 0 and r - 1"""
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        row0 = row0_of(hostcheck, h)
        rng = random.Random(0x5EE2E + kind)
        states = [[rng.randrange(P) for _ in range(17)] for _ in range(60)]
        for c in cv.uniform_corners(P):
            states += [[c] * 17, [c if j % 2 else 0 for j in range(17)], [P - 1 if j % 2 else c for j in range(17)]]
        states += [[0] * 17, [P - 1] * 17]
        got = squeeze_row(hostcheck, h, states)
        for st, g in zip(states, got):
            assert g == sum(row0[e] * RI % P * (st[e] << cv.SBOX_SHIFT) for e in range(17)) % P, st[:2]
    finally:
        hostcheck.params_free(h)


# ---- the entry to the partial rounds ---------------------------------------------------------------------------------------------------------------
B17 = 17 * 32 * 128 * 128          # 8 912 896: the digit-sum bound of a row of 17 K-steps


def finish_bytes_mad(hostcheck, sums):
    s = np.ascontiguousarray(sums, dtype=np.int32); n = s.shape[0]
    assert s.shape == (n, 32)
    cols = np.zeros((n, 8), np.int64); qh = np.zeros(n, np.int32); carry = np.zeros(n, np.int64); digits = np.zeros((n, 32), np.int8)
    rc = hostcheck.l.hc_mfma_finish_bytes_mad(ptr(s), C.c_size_t(n), ptr(cols), ptr(qh), ptr(carry), ptr(digits))
    return rc, cols, qh, carry, digits


def check_entry_rows(hostcheck, cases):
    """the columns are V's word columns inside the stated bound; q^ is floor(V / 2^254) or one more; no carry leaves word 7; the digits sum to
    W = V - q^ r exactly, inside (-r - 2^145, 2^254 + 2^145), so W == V (mod r): the canonical finish of the same sums.  Returns the q^ - floor seen."""
    assert all(abs(x) <= B17 for s in cases for x in s)
    rc, cols, qh, carry, digits = finish_bytes_mad(hostcheck, cases)
    assert rc == 0, rc
    canon = finish(hostcheck, cases)
    seen = set()
    for s, col, q, cy, d, z in zip(cases, cols, qh, carry, digits, canon):
        V = value(s)
        want_cols = [s[4 * k] + 256 * s[4 * k + 1] + 65536 * s[4 * k + 2] + 16777216 * s[4 * k + 3] for k in range(8)]
        assert [int(x) for x in col] == want_cols and all(abs(x) < int(2 ** 47.1) for x in want_cols), s
        fl = V >> 254
        assert int(q) in (fl, fl + 1) and abs(int(q)) < int(2 ** 18.2) and int(cy) == 0, (s, int(q), fl)
        seen.add(int(q) - fl)
        W = value([int(x) for x in d])
        assert W == V - int(q) * P and -P - (1 << 145) < W < (1 << 254) + (1 << 145), (s, hex(W))
        assert W % P == V % P == z, s
    return seen


def test_entry_rows_extremes(hostcheck):
    B = B17
    cases = [[B] * 32, [-B] * 32, [B if c % 2 == 0 else -B for c in range(32)], [-B if c % 2 == 0 else B for c in range(32)], [0] * 32]
    for c in (0, 27, 28, 31):
        for v in (1, -1, B, -B):
            s = [0] * 32; s[c] = v; cases.append(s)
    check_entry_rows(hostcheck, cases)
    s = [0] * 32; s[3] = B + 1
    assert finish_bytes_mad(hostcheck, [s])[0] == -1


def test_entry_rows_crafted_multiples(hostcheck):
    """V = k r +- 1, k r and k 2^254 +- 1, k 2^254 for |k| up to 2^17 (|S_31| = 2^23, inside 17 K-steps' domain): both outcomes of the estimate"""
    Vs = []
    for k in (-(1 << 17), -1, 0, 1, 1 << 17):
        for d in (-1, 0, 1):
            Vs += [k * P + d, (k << 254) + d]
    cases = [split_digits(V) for V in Vs]
    assert all(value(s) == V for V, s in zip(Vs, cases))
    assert check_entry_rows(hostcheck, cases) == {0, 1}


def test_entry_rows_random(hostcheck):
    rng = random.Random(0xE27B)
    check_entry_rows(hostcheck, [[rng.randint(-B17, B17) for _ in range(32)] for _ in range(20000)])
