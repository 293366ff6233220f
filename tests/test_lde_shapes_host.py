"""The LDE shape matrix covers every first-pass route (tests/lde_shapes.py), and the oracle's LDE — the reference of
tests/test_gpu_lde_blowups.py — equals the definition computed without the oracle's NTT.  No GPU."""
import numpy as np
import pytest

import lde_shapes as ls
import pyref

PRIMES = {0: pyref.P_PALLAS, 1: pyref.P_BLS}
GEN = {0: 5, 1: 7}

# every (passes, route, pre-scale) the library can take, written out: dropping a shape from SHAPES, or a route from `route`, fails here
EXPECTED = {(1, ls.NO_EXTENSION, 0), (1, ls.NO_EXTENSION, 1), (1, ls.PADDED, 0), (1, ls.PADDED, 1)}
for _P in (2, 3):
    EXPECTED |= {(_P, ls.NO_EXTENSION, 0), (_P, ls.NO_EXTENSION, 1), (_P, ls.PADDED, 0), (_P, ls.PADDED, 1), (_P, ls.UNIT, 0),
                 (_P, ls.FAST, 1), (_P, ls.FAST_ZERO, 1), (_P, ls.FAST_ZERO_ONE, 1), (_P, ls.GENERAL, 1)}


def test_split_restates_the_plan_sizes():
    assert ls.split(0) == [0] and ls.split(10) == [10]
    assert ls.split(11) == [6, 5] and ls.split(16) == [8, 8] and ls.split(20) == [10, 10]
    assert ls.split(21) == [7, 7, 7] and ls.split(23) == [8, 8, 7] and ls.split(24) == [8, 8, 8] and ls.split(30) == [10, 10, 10]
    for lg in range(0, 31):
        s = ls.split(lg)
        assert sum(s) == lg and max(s) <= 10 and len(s) == (1 if lg <= 10 else 2 if lg <= 20 else 3)


def test_shapes_hit_every_route():
    assert ls.all_routes() == EXPECTED
    hit = {}
    for log_n, lb in ls.SHAPES:
        assert log_n + lb <= 21
        for pre in (0, 1):
            hit.setdefault(ls.route(log_n, lb, pre) + (pre,), []).append((log_n, lb))
    assert set(hit) == EXPECTED, sorted(EXPECTED - set(hit))
    for P in (2, 3):        # the zero-group loop: at least two blow-ups per pass count, besides its nz == 1 edge
        assert len({lb for _, lb in hit[(P, ls.FAST_ZERO, 1)]}) >= 2, P
    # nz == B/2, the largest count the general path sees, and nz == B/4
    for P in (2, 3):
        assert {lb for _, lb in hit[(P, ls.GENERAL, 1)]} == {1, 2}, P


def test_route_examples():
    assert ls.route(20, 3, 1) == (3, ls.FAST) and ls.route(20, 3, 0) == (3, ls.UNIT)          # the bench step
    assert ls.route(7, 4, 1) == (2, ls.FAST_ZERO) and ls.route(5, 6, 1) == (2, ls.FAST_ZERO_ONE) and ls.route(4, 7, 1) == (2, ls.PADDED)
    assert ls.route(10, 1, 1) == (2, ls.GENERAL) and ls.route(8, 2, 1) == (1, ls.PADDED) and ls.route(21, 0, 1) == (3, ls.NO_EXTENSION)
    assert ls.route(20, 4, 1) == (3, ls.FAST_ZERO) and ls.route(18, 6, 1) == (3, ls.FAST_ZERO)


def ints(limbs, p):
    return [pyref.from_limbs(x, p) for x in limbs]


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("log_n,lb", [s for s in ls.SHAPES if s[0] <= 5])
def test_oracle_lde_is_the_definition(oracle, field, log_n, lb):
    """Interpolate with the O(n^2) DFT on Python integers, evaluate by Horner at g * w_N^j for every j: the oracle's LDE on all outputs."""
    p = PRIMES[field]; n, N = 1 << log_n, 1 << (log_n + lb)
    ev = oracle.synth_column(0xA11 + log_n, lb, 0, n)                   # stored values below 2^254: elements of both fields
    x = ints(ev, p)
    wN = oracle.to_int(oracle.root_of_unity(log_n + lb, field), field)
    assert pow(wN, N, p) == 1 and (N == 1 or pow(wN, N // 2, p) == p - 1)
    wn = pow(wN, 1 << lb, p)
    coeffs = [c * pow(n, -1, p) % p for c in pyref.dft(x, pow(wn, -1, p), p)]
    assert [sum(c * pow(wn, i * j, p) for j, c in enumerate(coeffs)) % p for i in range(n)] == x
    for g in (None, GEN[field]):
        want = []
        for j in range(N):
            pt = (g or 1) * pow(wN, j, p) % p; acc = 0
            for c in reversed(coeffs):
                acc = (acc * pt + c) % p
            want.append(pyref.to_limbs(acc, p))
        got = oracle.lde(field, ev, lb, None if g is None else oracle.from_u64(g, field))
        assert got.shape == (N, 4)
        assert (got == np.array(want, np.uint64)).all(), (field, log_n, lb, g)


@pytest.mark.parametrize("field", [0, 1])
def test_oracle_lde_with_shift_one_is_the_unshifted_lde(oracle, field):
    one = oracle.from_u64(1, field)
    assert pyref.from_limbs(one, PRIMES[field]) == 1
    for log_n, lb in [s for s in ls.SHAPES if s[0] + s[1] <= 12]:
        ev = oracle.synth_column(0xB22 + log_n, lb, 0, 1 << log_n)
        assert (oracle.lde(field, ev, lb, one) == oracle.lde(field, ev, lb)).all(), (field, log_n, lb)
