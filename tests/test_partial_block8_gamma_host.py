"""The Gamma terms of the 8-round partial blocks as K-steps of the E rows' tiles (poseidon_pair.hpp pair_block8, host_util.hpp blk8_gfrag), host side:
every Gamma fragment against Python big integers, with Gamma recomputed from the set's M; the whole permutation through the block form with the very
tables the device gets (hostcheck.cpp hc_permute_block8: row q one tile of 16 + q K-steps) against the reference's dense rounds, on random states and
on states whose partial-round S-box outputs are ONE uniform corner at all eight positions of every block, so that row 7's seven Gamma steps carry the
same extreme digits together; and the largest |digit sum| a row of 16 + 7 K-steps reached over those runs, which must stay inside the finishing
step's domain |S| < 2^24 (the a-priori bound is 23 * 32 * 128 * 128 = 12 058 624).  CPU only."""
import ctypes as C

import numpy as np
import pytest

import corner_values as cv
import partial_block8_lib as b8
import pyref
from test_partial_block8_host import SETS17, frag_value, sparse_of, states

P = pyref.P_PALLAS
R = pyref.R
ROW23_BOUND = 23 * 32 * 128 * 128
STEER = dict(which=1, pos=7100, level=3, label=42)


def gfrag(hc, h):
    """blk8_gfrag of a host-check set: int8 [blocks][28][64][16], fragment q (q - 1) / 2 + p of a block = Gamma_{q,p}"""
    hc.l.hc_blk8_table.restype = C.c_size_t
    n = hc.l.hc_blk8_table(h, 3, None, C.c_size_t(0))
    raw = np.zeros(n, np.int8)
    assert n and hc.l.hc_blk8_table(h, 3, raw.ctypes.data_as(C.c_void_p), C.c_size_t(n)) == n
    return raw.reshape(-1, 28, 64, 16)


def row23_max(hc, reset=False):
    hc.l.hc_blk8_row23_max.restype = C.c_int32
    return hc.l.hc_blk8_row23_max(C.c_int(1 if reset else 0))


@pytest.fixture(scope="module")
def base17():
    return pyref.params_for_width(17)


def uniform_node(base17, i):
    """the steered set of uniform corner i: that corner behind every S-box of the first permutation of its state"""
    uni = cv.uniform_corners(P)
    nd = cv.steered_set(base17, cv.target_schedules(base17)[i], STEER["which"], STEER["pos"] + i, STEER["level"], STEER["label"])
    assert nd["tp"] == [uni[i]] * base17["rp"]
    return nd


def check_tables(hostcheck, h, M):
    sp = sparse_of({"t": 17, "rp": 64, "mds": M})
    G = gfrag(hostcheck, h)
    assert G.shape[0] == 8
    for blk in range(8):
        for q in range(1, 8):
            for p in range(q):
                g = sum(sp[8 * blk + q][1][j] * sp[8 * blk + p][2][j] for j in range(16)) % P
                for b in range(32):
                    assert frag_value(G[blk, q * (q - 1) // 2 + p], b) == ((g << cv.SBOX_SHIFT) << (8 * b)) % P, (blk, q, p, b)


@pytest.mark.parametrize("name", ["merkle", "transcript", "bench"])
def test_gamma_fragments_hold_the_stated_residues(hostcheck, name):
    """EVERY fragment (block, q, p) and digit position b: the signed radix-256 digits of (Gamma_{q,p} 2^20 256^b) mod r, Gamma = sum_j u_{q,j} w_{p,j}"""
    kind, seed = SETS17[name]
    h = hostcheck.params(kind, 17, seed)
    try:
        mds, _, _ = hostcheck.params_export(h, 17, 8, 64)
        Ri = pow(R, -1, P)
        check_tables(hostcheck, h, [[cv.raw_to_int(mds[i * 17 + j]) * Ri % P for j in range(17)] for i in range(17)])
    finally:
        hostcheck.params_free(h)


def test_gamma_fragments_hold_the_stated_residues_steered_set(hostcheck, base17):
    nd = uniform_node(base17, 0)
    h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
    try:
        check_tables(hostcheck, h, nd["params"]["mds"])
    finally:
        hostcheck.params_free(h)


def test_block8_rows_of_up_to_23_k_steps_equal_dense_rounds(hostcheck, base17):
    """hc_permute_block8 against hc_permute_dense: random states and 0 / r - 1 states on the merkle, transcript and bench sets; on the steered set
    of every uniform corner the steered state itself (all eight S-box outputs of every block that corner) and the random states.  The mirror refuses
    (-2) any digit sum outside |S| < 2^24; the largest one its 23-step rows saw is reported and checked against both limits."""
    row23_max(hostcheck, reset=True)

    def check(h, s):
        got = b8.permute_block8(hostcheck, h, s); want = hostcheck.permute_dense(h, s, 17)
        assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
        assert (want != s).any()
    for name in ("merkle", "transcript", "bench"):
        kind, seed = SETS17[name]
        h = hostcheck.params(kind, 17, seed)
        try:
            check(h, states(23))
        finally:
            hostcheck.params_free(h)
    running = []                                              # (corner, the largest |digit sum| of a 23-step row so far)
    for i, c in enumerate(cv.uniform_corners(P)):
        nd = uniform_node(base17, i)
        _, op, _ = cv.sbox_outputs(nd["params"], nd["state"])
        assert op == [c] * base17["rp"]                       # the partial-round S-boxes deliver the corner in all eight positions of every block
        h = hostcheck.params_upload(*cv.params_arrays(nd["params"]))
        try:
            check(h, cv.raw_array([v * R % P for v in nd["state"]]))
            check(h, states(40 + i))
        finally:
            hostcheck.params_free(h)
        running.append(("%064x" % c, row23_max(hostcheck)))
    seen = row23_max(hostcheck)
    report = "largest |digit sum| in a row of 16 + 7 K-steps: %d (a-priori bound %d, finishing step's domain below %d); running maximum after each uniform corner: %s" % (seen, ROW23_BOUND, 1 << 24, running)
    print(report)
    assert 0 < seen <= ROW23_BOUND < 1 << 24, report
