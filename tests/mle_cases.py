"""Shared inputs of the Mle::evaluate batch tests (test_mle_batch_host.py on the CPU, test_gpu_mle_batch.py on the device): the k matrix, seeded tables
and points, the stored-limb corner tables, and the ctypes wrapper of the host instantiation hc_mle_evaluate_batch (csrc/hostcheck.cpp)."""
import ctypes as C

import numpy as np

import corner_values as cv
import pyref

K_MATRIX = (0, 1, 2, 3, 4, 6, 7, 10)
PASSES_AT_TILE_3 = (0, 1, 1, 1, 2, 2, 3, 4)          # ceil(k / 3)
LOG_TILES = tuple(range(3, 13))                      # the range of the context option "mle_log_tile"
P = pyref.P_PALLAS


def default_log_tile(hostcheck):
    return int(hostcheck.l.hc_mle_default_log_tile())


def hc_evaluate(hostcheck, tables, k, r, log_tile=-1, contig=-1):
    """hc_mle_evaluate_batch: the driver's passes, every workgroup of k_mle_fold_pass in lockstep on the host -> ((B, 4) results, launches per evaluation)"""
    B = len(tables)
    tabs = [np.ascontiguousarray(t, dtype=np.uint64) for t in tables]
    assert all(t.shape == (1 << k, 4) for t in tabs)
    ptrs = (C.c_void_p * max(B, 1))(*[t.ctypes.data for t in tabs])
    rr = np.ascontiguousarray(r, dtype=np.uint64).reshape(B * k, 4) if B * k else np.zeros((1, 4), np.uint64)
    out = np.full((B, 4), 0x5A5A5A5A5A5A5A5A, np.uint64); passes = C.c_size_t(99)
    rc = hostcheck.l.hc_mle_evaluate_batch(C.c_size_t(B), ptrs, C.c_size_t(k), rr.ctypes.data_as(C.c_void_p), C.c_int(log_tile), C.c_int(contig),
                                           out.ctypes.data_as(C.c_void_p), C.byref(passes))
    assert rc == 0, rc
    return out, passes.value


def tables_and_points(oracle, k, B, seed=0x3E1E):
    """B seeded tables of 2^k stored elements and B points of k stored elements ((B, k, 4))"""
    tabs = [oracle.synth_column(seed + k, b, 0, 1 << k) for b in range(B)]
    pts = np.stack([oracle.synth_column(seed + 0x100 + k, b, 0, max(k, 1))[:k] for b in range(B)]) if B else np.zeros((0, k, 4), np.uint64)
    return tabs, pts


def reference(oracle, tables, k, pts):
    return np.stack([oracle.mle_evaluate(t, pts[b]) if k else np.asarray(t[0]) for b, t in enumerate(tables)])


def boolean_points(oracle, k):
    """every x in {0, 1}^k as a point: bit j of x -> r_j (r_0 binds the least significant index bit)"""
    zero, one = np.zeros(4, np.uint64), oracle.from_u64(1)
    return np.stack([np.stack([one if (x >> j) & 1 else zero for j in range(k)]) for x in range(1 << k)])


def corner_case(k, B):
    """tables and points whose stored limbs are the corners of corner_values.stored_corners: 0, 1, r - 1, the Montgomery one and its negative, limb edges"""
    c = cv.raw_array(cv.stored_corners(P)); L = c.shape[0]
    tabs = [c[(np.arange(1 << k) * (2 * b + 1) + 5 * b) % L] for b in range(B)]
    pts = np.stack([c[(np.arange(k) * 3 + 7 * b + 3) % L] for b in range(B)])
    return tabs, pts
