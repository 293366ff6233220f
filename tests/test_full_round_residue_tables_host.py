"""The residue-table form of the t = 17 full rounds' matrix-core product (poseidon_pair.hpp pair_mds_sbox_mfma), host side: the int8 fragment
tables host_util.hpp mfma_frags builds, read back through their documented lane layout, and the finishing step (fold of the 32 digit sums, signed
carry pass, product-free reduction: mfma_digits.hpp) over its whole stated input domain |S_c| < 2^24 — both against Python big integers.  CPU only."""
import ctypes as C
import random

import numpy as np
import pytest

import corner_values as cv
import pyref

P = pyref.P_PALLAS
R = pyref.R
SETS17 = {"merkle": (0, b""), "transcript": (1, b""), "bench": (2, b"POSEIDON-T17-X5")}
LIM = (1 << 24) - 1                      # the finishing step's domain: |S_c| <= 2^24 - 1 (the kernels' sums stay below 17 * 32 * 128 * 128)


def frag_table(hostcheck, h, pre):
    """the fragment table as an int8 array [i][e][lane][16 bytes]"""
    l = hostcheck.l
    l.hc_mfma_frag_table.restype = C.c_size_t
    n = l.hc_mfma_frag_table(h, pre, None, C.c_size_t(0))
    assert n == 17 * 17 * 64 * 16
    out = np.zeros(n, np.int8)
    assert l.hc_mfma_frag_table(h, pre, out.ctypes.data_as(C.c_void_p), C.c_size_t(n)) == n
    return out.reshape(17, 17, 64, 16)


def finish(hostcheck, sums):
    """(n, 32) digit sums -> list of n integers (the stored limbs the finishing step returns)"""
    s = np.ascontiguousarray(sums, dtype=np.int32)
    assert s.ndim == 2 and s.shape[1] == 32
    out = np.zeros((s.shape[0], 4), np.uint64)
    rc = hostcheck.l.hc_mfma_finish(s.ctypes.data_as(C.c_void_p), C.c_size_t(s.shape[0]), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return [cv.raw_to_int(x) for x in out]


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


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_fragment_tables_hold_the_residues(hostcheck, name):
    """For M and for B_1 * M (recomputed in Python from the exported M) and every (i, e, b): the 32 digits of fragment (i, e) at K position b — lane
    l = c + 32 (b >> 4), byte b & 15 — are in [-128, 127] (int8 by construction; asserted through the round trip) and sum to
    (M[i][e] * 2^20 * 256^b) mod r."""
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    mds, _, _ = hostcheck.params_export(h, 17, 8, 64)
    Ri = pow(R, -1, P)
    M = [[cv.raw_to_int(mds[i * 17 + j]) * Ri % P for j in range(17)] for i in range(17)]
    mats = {0: M, 1: cv.mds_pre_canonical({"t": 17, "mds": M, "rp": 64})}
    K = sum(0x80 << (8 * c) for c in range(32))
    for pre in (0, 1):
        F = frag_table(hostcheck, h, pre).astype(np.int16)
        assert F.min() >= -128 and F.max() <= 127
        # [i][e][kh][c][j] -> [i][e][b = 16 kh + j][c]
        D = F.reshape(17, 17, 2, 32, 16).transpose(0, 1, 2, 4, 3).reshape(17, 17, 32, 32)
        U = (D + 128).astype(np.uint8)
        for i in range(17):
            for e in range(17):
                c0 = (mats[pre][i][e] << cv.SBOX_SHIFT) % P
                for b in range(32):
                    got = int.from_bytes(U[i, e, b].tobytes(), "little") - K
                    assert got == (c0 << (8 * b)) % P, (name, pre, i, e, b)
    hostcheck.params_free(h)


def test_finishing_step_extremes_and_single_sums(hostcheck):
    cases = [[LIM] * 32, [-LIM] * 32, [LIM if c % 2 == 0 else -LIM for c in range(32)], [-LIM if c % 2 == 0 else LIM for c in range(32)], [0] * 32]
    for c in (0, 31):
        for v in (1, -1, LIM, -LIM, 8912896, -8912896):
            s = [0] * 32; s[c] = v; cases.append(s)
    for s, got in zip(cases, finish(hostcheck, cases)):
        assert got < P and got == value(s) % P, s


def test_finishing_step_crafted_multiples(hostcheck):
    """V = k r - 1, k r, k r + 1 and k 2^254 - 1, k 2^254 + 1 for k in {-2^17, -1, 0, 1, 2^17}: the two ends of the range of the value left before the
    conditional subtractions."""
    Vs = []
    for k in (-(1 << 17), -1, 0, 1, 1 << 17):
        Vs += [k * P - 1, k * P, k * P + 1, (k << 254) - 1, (k << 254) + 1]
    cases = [split_digits(V) for V in Vs]
    for V, s in zip(Vs, cases):
        assert value(s) == V and all(-128 <= d <= 127 for d in s[:31]) and abs(s[31]) < 1 << 24
    for V, got in zip(Vs, finish(hostcheck, cases)):
        assert got < P and got == V % P, hex(V)


def test_finishing_step_random(hostcheck):
    rng = random.Random(0x5EED17)
    cases = [[rng.randint(-LIM, LIM) for _ in range(32)] for _ in range(10000)]
    for s, got in zip(cases, finish(hostcheck, cases)):
        assert got < P and got == value(s) % P, s


def test_finishing_step_rejects_sums_outside_its_domain(hostcheck):
    s = np.zeros((1, 32), np.int32); s[0, 5] = 1 << 24
    out = np.zeros((1, 4), np.uint64)
    assert hostcheck.l.hc_mfma_finish(s.ctypes.data_as(C.c_void_p), C.c_size_t(1), out.ctypes.data_as(C.c_void_p)) == -1
