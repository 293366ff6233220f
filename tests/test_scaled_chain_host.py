"""The scaled S-box chain of the 8-round partial blocks (host_util.hpp blk8s_*, poseidon_pair.hpp pair_block8: wave X carries lambda_q X_q and no
round multiplies a_q y_q), host side.  The tables the device gets against Python big integers, lambda recomputed from the exported M; the whole
permutation through the scaled block form (hostcheck.cpp hc_permute_block8) against the reference's dense rounds on random states, the all-0 and
all-(r - 1) states and steered sets that put every stored corner at the S-box of the SCALED chain — delivered by it, and read by it — at every
position of a block; a set with M[0][0] = 0, for which no lambda exists.  CPU only."""
import ctypes as C
import random

import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref
import scaled_chain_lib as sc
from hostcheck_lib import A, P as PTR, vp
from test_partial_block8_host import SETS17, frag_value, sparse_of, states

P = pyref.P_PALLAS
R = pyref.R


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_scaled_tables_hold_the_stated_values(hostcheck, name):
    """lambda_q over all 64 rounds, every scaled constant lambda_q c_q, the unscale limbs = nine 29-bit limbs of (1 / lambda_64) 2^261 mod r (a
    multiplier-table entry without the S-box scale), and sampled fragments (block, row, lane, K position with 0 / 1 / 15 / 16 / 30 / 31 included):
    E = (u_{q,j} lambda_{q+1} 256^b) mod r, lane = (w_{p,j} / (kappa lambda_p^5) 256^b) mod r, Gamma = (Gamma_{q,p} lambda_{q+1} / (kappa lambda_p^5) 256^b)
    mod r.  The unscaled family (codes 0..3) is still there, the unit fragment with it."""
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        M, rcp = sc.mds_of(hostcheck, h)
        lam = sc.lambdas(M, 64)
        E, L, G, rcs, got_lam, limbs = sc.scaled_tables(hostcheck, h)
        assert got_lam == lam and lam[0] == 1 and all(lam)
        assert rcs == [lam[q] * rcp[q] % P for q in range(64)]
        assert all(x < 1 << 29 for x in limbs) and sum(x << (29 * i) for i, x in enumerate(limbs)) == pow(lam[64], -1, P) * (1 << 261) % P
        assert E.shape[0] == 8 and L.shape[0] == 8 and G.shape[0] == 8
        assert b8.table(hostcheck, h, 0).shape == E.shape and b8.table(hostcheck, h, 1)[0].shape == L.shape
        sp = sparse_of({"t": 17, "rp": 64, "mds": M})
        assert all(s[0] == M[0][0] for s in sp)                 # a_q is M[0][0] in every round: what lambda's recurrence divides by
        rng = random.Random(88)
        for _ in range(300):
            blk, q, j, p, b = rng.randrange(8), rng.randrange(8), rng.randrange(16), rng.randrange(8), rng.choice([0, 1, 15, 16, 30, 31, rng.randrange(32)])
            assert frag_value(E[blk, q, j], b) == (sp[8 * blk + q][1][j] * lam[8 * blk + q + 1] % P << (8 * b)) % P, (blk, q, j, b)
            assert frag_value(L[blk, j, p], b) == (sp[8 * blk + p][2][j] * sc.yinv(lam, 8 * blk + p) % P << (8 * b)) % P, (blk, j, p, b)
            if q:
                p2 = p % q
                g = sum(sp[8 * blk + q][1][i] * sp[8 * blk + p2][2][i] for i in range(16)) % P
                assert frag_value(G[blk, q * (q - 1) // 2 + p2], b) == (g * lam[8 * blk + q + 1] % P * sc.yinv(lam, 8 * blk + p2) % P << (8 * b)) % P, (blk, q, p2, b)
    finally:
        hostcheck.params_free(h)


def check(hostcheck, h, s):
    got = b8.permute_block8(hostcheck, h, s); want = hostcheck.permute_dense(h, s, 17)
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (want != s).any()


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_scaled_block8_permutation_equals_dense_rounds(hostcheck, name):
    """random states, all 0, all r - 1 and alternating (test_partial_block8_host.states)"""
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        check(hostcheck, h, states(170)); check(hostcheck, h, states(171))
    finally:
        hostcheck.params_free(h)


def steered(base17, r, side):
    sched, corners = sc.scaled_schedule(base17, r, side)
    nd = cv.steered_set(base17, sched, 1, 9100 + 977 * r + (0 if side == "out" else 5), 3, 42)
    ins, outs = sc.scaled_chain_values(nd["params"], nd["state"])
    assert (outs if side == "out" else ins) == corners          # the scaled chain's S-boxes deliver / read the scheduled corners themselves
    return nd, corners


def test_scaled_schedules_put_every_corner_at_every_block_position(base17):
    uni = cv.uniform_corners(P); rest = [c for c in cv.stored_corners(P) if c not in uni]
    for side in ("out", "in"):
        seen = {(c, q % 8) for r in range(8) for q, c in enumerate(sc.scaled_schedule(base17, r, side)[1])}
        assert seen == {(c, pos) for c in rest for pos in range(8)}


@pytest.mark.parametrize("side", ["out", "in"])
@pytest.mark.parametrize("r", range(8))
def test_scaled_block8_permutation_equals_dense_rounds_steered(hostcheck, base17, r, side):
    """window r of the non-uniform stored corners at the S-box of the scaled chain, delivered (out) or read (in), the steered state itself and
    random states"""
    nd, _ = steered(base17, r, side)
    h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
    try:
        check(hostcheck, h, cv.raw_array([v * R % P for v in nd["state"]]))
        check(hostcheck, h, states(180 + r))
    finally:
        hostcheck.params_free(h)


@pytest.mark.parametrize("side", ["out", "in"])
def test_scaled_block8_permutation_equals_dense_rounds_uniform_corners(hostcheck, base17, side):
    """every uniform corner at the scaled chain's S-box in all 64 rounds at once"""
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
        finally:
            hostcheck.params_free(h)


def test_set_with_zero_m00_is_refused_as_before(hostcheck, base17):
    """M[0][0] = 0 leaves lambda undefined.  Such a set never reaches the block tables: the kernel-form constants need the in-place LU of M without
    pivoting, whose first pivot is M[0][0], so the host library reports the set not ok (as it did before the chain was scaled) and no 8-round form
    is offered for it."""
    a = cv.params_arrays(sc.zero_m00_params(base17))
    hostcheck.l.hc_params_upload.restype = vp
    h = vp(hostcheck.l.hc_params_upload(a[0], a[1], a[2], PTR(A(a[3])), PTR(A(a[4])), PTR(A(a[5]))))
    assert h.value
    try:
        assert not hostcheck.params_ok(h)
        s = states(5)
        assert hostcheck.l.hc_permute_block8(h, PTR(s), C.c_size_t(s.size // (17 * 4))) == -1
        assert sc.raw_table(hostcheck, h, 4).size == 0 and sc.raw_table(hostcheck, h, 0).size == 0
    finally:
        hostcheck.params_free(h)
