"""The scaled S-box chain of the 8-round partial blocks (host_util.hpp blk8s_*, poseidon_pair.hpp pair_block8) for the tests: lambda recomputed in
Python from a set's M, the host-check library's scaled tables (hc_blk8_table codes 4..8), the steered schedules that put the stored corners at the
S-box of the SCALED chain, and a set with M[0][0] = 0."""
import ctypes as C

import numpy as np

import corner_values as cv
import partial_block8_lib as b8
import pyref

P = pyref.P_PALLAS
R = pyref.R
KAPPA = pow(1 << cv.SBOX_SHIFT, -1, P)          # fr_pow5_r29's scale


def lambdas(M, rp):
    """lambda_0 = 1, lambda_{q+1} = lambda_q^5 kappa / M[0][0], q over all rp rounds (canonical integers)"""
    ai = pow(M[0][0], -1, P); lam = [1]
    for _ in range(rp):
        lam.append(pow(lam[-1], 5, P) * KAPPA % P * ai % P)
    return lam


def yinv(lam, q):
    """1 / (kappa lambda_q^5): what turns the scaled chain's S-box output back into y_q"""
    return pow(KAPPA * pow(lam[q], 5, P) % P, -1, P)


def raw_table(hc, h, which):
    hc.l.hc_blk8_table.restype = C.c_size_t
    n = hc.l.hc_blk8_table(h, which, None, C.c_size_t(0))
    raw = np.zeros(n, np.int8)
    assert hc.l.hc_blk8_table(h, which, raw.ctypes.data_as(C.c_void_p), C.c_size_t(n)) == n
    return raw


def scaled_tables(hc, h, rp=64):
    """(E int8 [blocks][8][16][64][16], L int8 [blocks][16][8][64][16], G int8 [blocks][28][64][16], rc_scaled [rp] canonical integers,
    lambda [rp + 1] canonical integers, the nine unscale limbs)"""
    Ri = pow(R, -1, P)
    E = raw_table(hc, h, 4).reshape(-1, 8, 16, 64, 16); L = raw_table(hc, h, 5).reshape(-1, 16, 8, 64, 16); G = raw_table(hc, h, 6).reshape(-1, 28, 64, 16)
    rcs = [cv.raw_to_int(x) * Ri % P for x in raw_table(hc, h, 7).view(np.uint64).reshape(-1, 4)]
    t8 = raw_table(hc, h, 8)
    lam = [cv.raw_to_int(x) * Ri % P for x in t8[:(rp + 1) * 32].view(np.uint64).reshape(-1, 4)]
    limbs = [int(x) for x in t8[(rp + 1) * 32:].view(np.uint32)]
    assert len(rcs) == rp and len(lam) == rp + 1 and len(limbs) == 9
    return E, L, G, rcs, lam, limbs


def mds_of(hc, h):
    mds, _, rcp = hc.params_export(h, 17, 8, 64)
    Ri = pow(R, -1, P)
    return [[cv.raw_to_int(mds[i * 17 + j]) * Ri % P for j in range(17)] for i in range(17)], [cv.raw_to_int(x) * Ri % P for x in rcp]


def scaled_schedule(base, r, side):
    """partial_block8_lib.block8_schedule moved to the SCALED chain: corner c scheduled at round q becomes the unscaled target under which the scaled
    chain meets c itself.
      side = "out": the scaled S-box DELIVERS c (stored limbs of yt_q = kappa lambda_q^5 y_q): unscaled target c / lambda_q^5;
      side = "in" : the scaled S-box READS c (stored limbs of lambda_q (X_q + c_q)): the unscaled input is c / lambda_q, target = what its S-box delivers.
    Returns (schedule for corner_values.steered_set, the scheduled corners [rp])."""
    name, tf, corners = b8.block8_schedule(base, r)
    lam = lambdas(base["mds"], base["rp"]); Ri = pow(R, -1, P)
    if side == "out":
        tp = [c * pow(pow(lam[q], 5, P), -1, P) % P for q, c in enumerate(corners)]
    else:
        tp = [cv.restored(pow(c * Ri % P * pow(lam[q], -1, P) % P, 5, P)) for q, c in enumerate(corners)]
    return ("scaled chain, %s, %s" % (side, name), tf, tp), corners


def scaled_chain_values(params, state):
    """what the scaled chain's partial-round S-boxes read and deliver, as STORED values, for pyref's permutation of `state`: (inputs [rp], outputs [rp])"""
    t, half = params["t"], params["rf"] // 2
    lam = lambdas(params["mds"], params["rp"])
    s = list(state)
    for r in range(half):
        s = cv._mds(params, [pow((s[i] + params["rc_full"][r][i]) % P, 5, P) for i in range(t)], P)
    ins, outs = [], []
    for q in range(params["rp"]):
        x = (s[0] + params["rc_partial"][q]) % P
        ins.append(lam[q] * x % P * R % P); outs.append(KAPPA * pow(lam[q] * x % P, 5, P) % P * R % P)
        s[0] = pow(x, 5, P); s = cv._mds(params, s, P)
    return ins, outs


def zero_m00_params(base):
    """the base set with M[0][0] = 0: no lambda exists.  The library refuses such a set altogether: the in-place LU of M has no pivoting"""
    M = [row[:] for row in base["mds"]]; M[0][0] = 0
    return dict(base, mds=M)
