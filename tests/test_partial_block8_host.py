"""The 8-round partial blocks of the t = 17 wave-pair kernels (poseidon_pair.hpp pair_block8), host side: the whole permutation through the block
form with the very tables the device gets (hostcheck.cpp hc_permute_block8: recode, emulated 32-row tiles with the unit K-step, fold, finish, gamma
sums) against the reference's dense rounds; the E, lane and unit fragments and gamma8_29 against Python big integers; the finish with the base lane
in the tile over the extremes of its domain.  CPU only."""
import random

import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref

P = pyref.P_PALLAS
R = pyref.R
SETS17 = {"merkle": (0, b""), "transcript": (1, b""), "bench": (2, b"POSEIDON-T17-X5")}
LIM = (1 << 24) - 1
UNIT_MAX = 32 * 128 * 128                 # the unit K-step's share of a digit sum: 32 digit products of at most 2^14
K80 = sum(0x80 << (8 * c) for c in range(32))


def states(seed):
    rng = np.random.default_rng(seed)
    rows = [[int.from_bytes(rng.bytes(40), "little") % P for _ in range(17)] for _ in range(3)] + [[0] * 17, [P - 1] * 17, [(P - 1) if j % 2 else 0 for j in range(17)]]
    return cv.raw_array([v for row in rows for v in row])


def check_set(hostcheck, h):
    s = states(17)
    got = b8.permute_block8(hostcheck, h, s); want = hostcheck.permute_dense(h, s, 17)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (want != s).any()


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_block8_permutation_equals_dense_rounds(hostcheck, name):
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        check_set(hostcheck, h)
    finally:
        hostcheck.params_free(h)


@pytest.mark.parametrize("which,r", [(1, 0), (2, 3)])
def test_block8_permutation_equals_dense_rounds_steered_sets(hostcheck, which, r):
    """two corner_values.steered_set sets (first permutation steered; both): chosen corners behind every S-box, and the steered state itself"""
    base = pyref.params_for_width(17)
    sc = cv.target_schedules(base)
    nd = cv.steered_set(base, sc[len(cv.uniform_corners(P)) + r], which, 7000 + r, 3, 42)
    h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
    try:
        check_set(hostcheck, h)
        s = cv.raw_array([v * R % P for v in nd["state"]])
        assert (b8.permute_block8(hostcheck, h, s) == hostcheck.permute_dense(h, s, 17)).all()
    finally:
        hostcheck.params_free(h)


def sparse_of(params):
    """the sparse factorisation of the partial rounds, recomputed in Python from the set's M (host_util.hpp make_kernel_consts): [(a, u[16], w[16])] per round"""
    t, rp, M = params["t"], params["rp"], params["mds"]
    n = t - 1
    def inv(a):
        a = [row[:] + [int(i == j) for j in range(n)] for i, row in enumerate(a)]
        for c in range(n):
            p = next(r for r in range(c, n) if a[r][c]); a[c], a[p] = a[p], a[c]
            iv = pow(a[c][c], -1, P); a[c] = [x * iv % P for x in a[c]]
            for r in range(n):
                if r != c and a[r][c]:
                    f = a[r][c]; a[r] = [(x - f * y) % P for x, y in zip(a[r], a[c])]
        return [row[n:] for row in a]
    cur = [row[:] for row in M]; out = [None] * rp
    for r in range(rp - 1, -1, -1):
        hat = [[cur[i + 1][j + 1] for j in range(n)] for i in range(n)]; hi = inv(hat)
        u = [sum(cur[0][q + 1] * hi[q][j] for q in range(n)) % P for j in range(n)]
        out[r] = (cur[0][0], u, [cur[i + 1][0] for i in range(n)])
        cur = [M[0][:]] + [[sum(hat[i][q] * M[q + 1][j] for q in range(n)) % P for j in range(t)] for i in range(n)]
    return out


def frag_value(frag, b):
    """the integer whose 32 signed digits fragment `frag` [64][16] holds at K position b: lane c + 32 (b >> 4), byte b & 15"""
    d = frag.reshape(2, 32, 16)[b >> 4, :, b & 15].astype(np.int16)
    assert d.min() >= -128 and d.max() <= 127
    return int.from_bytes((d + 128).astype(np.uint8).tobytes(), "little") - K80


@pytest.mark.parametrize("name", ["merkle", "bench"])
def test_block8_tables_hold_the_stated_residues(hostcheck, name):
    """sampled entries: E fragment (block, q, j) = (u_{q,j} 256^b) mod r; lane fragment (block, j, p) = (w_{p,j} 2^20 256^b) mod r; the unit fragment
    = 256^b mod r; gamma8_29 = nine 29-bit limbs of (sum_j u_{q,j} w_{p,j}) 2^20 2^261 mod r — all with u, w recomputed in Python from the exported M."""
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        mds, _, _ = hostcheck.params_export(h, 17, 8, 64)
        Ri = pow(R, -1, P)
        M = [[cv.raw_to_int(mds[i * 17 + j]) * Ri % P for j in range(17)] for i in range(17)]
        sp = sparse_of({"t": 17, "rp": 64, "mds": M})
        E = b8.table(hostcheck, h, 0); L, unit = b8.table(hostcheck, h, 1); G = b8.table(hostcheck, h, 2)
        assert E.shape[0] == 8 and L.shape[0] == 8 and G.shape[0] == 8
        rng = random.Random(8)
        for b in range(32):
            assert frag_value(unit, b) == (1 << (8 * b)) % P
        for _ in range(300):
            blk, q, j, p, b = rng.randrange(8), rng.randrange(8), rng.randrange(16), rng.randrange(8), rng.choice([0, 1, 15, 16, 30, 31, rng.randrange(32)])
            assert frag_value(E[blk, q, j], b) == (sp[8 * blk + q][1][j] << (8 * b)) % P, (blk, q, j, b)
            assert frag_value(L[blk, j, p], b) == ((sp[8 * blk + p][2][j] << cv.SBOX_SHIFT) << (8 * b)) % P, (blk, j, p, b)
        for blk in range(8):
            for q in range(1, 8):
                for p in range(q):
                    g = sum(sp[8 * blk + q][1][j] * sp[8 * blk + p][2][j] for j in range(16)) % P
                    limbs = G[blk, q * (q - 1) // 2 + p]
                    assert all(int(x) < 1 << 29 for x in limbs)
                    assert sum(int(x) << (29 * i) for i, x in enumerate(limbs)) == (g << cv.SBOX_SHIFT) * (1 << 261) % P, (blk, q, p)
    finally:
        hostcheck.params_free(h)


def value(sums):
    return sum(int(s) << (8 * c) for c, s in enumerate(sums))


def split_digits(V):
    S = []
    for _ in range(31):
        d = ((V + 128) & 0xff) - 128
        S.append(d); V = (V - d) >> 8
    S.append(V)
    return S


def unit_sums(unit, base):
    """the unit K-step's digit sums for a canonical base, in Python from the exported fragment: U_c = sum_b unit_b[c] * digit_b(base)"""
    v = base + K80
    bd = [((v >> (8 * b)) & 0xff) - 128 for b in range(32)]
    u = unit.reshape(2, 32, 16).astype(np.int64)
    return [sum(int(u[b >> 4, c, b & 15]) * bd[b] for b in range(32)) for c in range(32)]


def test_finish_with_base_in_the_tile(hostcheck):
    """The lane product's finish with the base lane as the ninth K-step: TOTAL digit sums at +-(2^24 - 1) (all, alternating), zero, the crafted
    multiples of r and of 2^254 of the residue-table test, and random ones, each with base in {0, 1, r - 1} and random bases: the result is
    (sum_c S_c 256^c + base) mod r for the y part S.  A y part that the base pushes out of the domain is refused; the kernel's own bound
    8 * 32 * 128 * 128 + 32 * 128 * 128 = 9 * 32 * 128 * 128 < 2^24 is asserted on the unit part."""
    h = hostcheck.params(0, 17, b"")
    try:
        _, unit = b8.table(hostcheck, h, 1)
        rng = random.Random(0xB8)
        bases = [0, 1, P - 1] + [rng.randrange(P) for _ in range(3)]
        totals = [[LIM] * 32, [-LIM] * 32, [LIM if c % 2 == 0 else -LIM for c in range(32)], [-LIM if c % 2 == 0 else LIM for c in range(32)], [0] * 32]
        for k in (-(1 << 17), -1, 0, 1, 1 << 17):
            totals += [split_digits(V) for V in (k * P - 1, k * P, k * P + 1, (k << 254) - 1, (k << 254) + 1)]
        totals += [[rng.randint(-LIM, LIM) for _ in range(32)] for _ in range(2000)]
        sums, bs, want = [], [], []
        for i, tot in enumerate(totals):
            for base in (bases if i < 30 else [bases[i % len(bases)]]):
                U = unit_sums(unit, base)
                assert all(abs(x) <= UNIT_MAX for x in U) and value(U) % P == base
                sums.append([a - b for a, b in zip(tot, U)]); bs.append(base); want.append(value(tot) % P)
        rc, got = b8.finish_with_base(hostcheck, h, sums, bs)
        assert rc == 0
        for s, b, g, w in zip(sums, bs, got, want):
            assert g < P and g == w == (value(s) + b) % P, (s, b)
        out_of_domain = [LIM] * 32                      # the y part alone at the limit: any non-zero unit part leaves the domain somewhere
        rc, _ = b8.finish_with_base(hostcheck, h, [out_of_domain, [-x for x in out_of_domain]], [P - 1, P - 1])
        assert rc == -1
    finally:
        hostcheck.params_free(h)


def test_block8_schedules_put_every_corner_at_every_block_position():
    """the steered schedules of tests/test_gpu_partial_block8.py: over r = 0..7 every non-uniform corner at every position of an 8-round block"""
    base = pyref.params_for_width(17)
    uni = cv.uniform_corners(P); rest = [c for c in cv.stored_corners(P) if c not in uni]
    seen = {(c, q % 8) for r in range(8) for q, c in enumerate(b8.block8_schedule(base, r)[2])}
    assert seen == {(c, pos) for c in rest for pos in range(8)}
