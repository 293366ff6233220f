"""ctypes bindings of the host-check library's mirror of the 8-round partial blocks (hostcheck.cpp hc_permute_block8, hc_blk8_table,
hc_blk8_finish_with_base), on top of a hostcheck_lib.HostCheck."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import corner_values as cv
import pyref
from hostcheck_lib import A, P


def permute_block8(hc, h, states):
    """t = 17 states (stored limbs) through the block-8 form of the wave-pair kernels, with the tables the device gets"""
    s = A(states).copy(); rc = hc.l.hc_permute_block8(h, P(s), C.c_size_t(s.size // (17 * 4)))
    assert rc == 0, rc; return s


def table(hc, h, which):
    """which = 0: E fragments int8 [blocks][8][16][64][16]; 1: lane fragments int8 [blocks][16][8][64][16] and the unit fragment [64][16];
    2: gamma8_29 uint32 [blocks][28][9]"""
    hc.l.hc_blk8_table.restype = C.c_size_t
    n = hc.l.hc_blk8_table(h, which, None, C.c_size_t(0))
    raw = np.zeros(n, np.int8)
    assert hc.l.hc_blk8_table(h, which, raw.ctypes.data_as(C.c_void_p), C.c_size_t(n)) == n
    if which == 0:
        return raw.reshape(-1, 8, 16, 64, 16)
    if which == 1:
        return raw[:-1024].reshape(-1, 16, 8, 64, 16), raw[-1024:].reshape(64, 16)
    return raw.view(np.uint32).reshape(-1, 28, 9)


def finish_with_base(hc, h, sums, bases):
    """(n, 32) digit sums of the y K-steps and n canonical bases (integers below r) -> (return code, list of n integers)"""
    s = np.ascontiguousarray(sums, dtype=np.int32); assert s.ndim == 2 and s.shape[1] == 32
    b = np.array([[(int(v) >> (64 * i)) & ((1 << 64) - 1) for i in range(4)] for v in bases], np.uint64).reshape(-1, 4)
    out = np.zeros((s.shape[0], 4), np.uint64)
    rc = hc.l.hc_blk8_finish_with_base(h, s.ctypes.data_as(C.c_void_p), P(b), C.c_size_t(s.shape[0]), P(out))
    return rc, [sum(int(x[i]) << (64 * i) for i in range(4)) for x in out]


def block8_schedule(base, r):
    """(name, targets_full, targets_partial) for corner_values.steered_set: the full-round targets of the first rotation of target_schedules; in the
    partial rounds position q mod 8 of every block gets the window [8 r, 8 r + 8) of the non-uniform corners, shifted by 5 (q mod 8): over
    r = 0..7 the windows tile the list, so every such corner stands behind the S-box at every position of an 8-round block."""
    p = pyref.P_PALLAS
    tf = next(s for s in cv.target_schedules(base) if s[0].startswith("rotation"))[1]
    uni = cv.uniform_corners(p); rest = [c for c in cv.stored_corners(p) if c not in uni]; n = len(rest)
    rp = base["rp"]
    return ("block-of-8 window %d" % r, tf, [rest[(r * (rp // 8) + q // 8 + 5 * (q % 8)) % n] for q in range(rp)])


def dense_level16(hc, h, from_u64, level, pos0, label, children, workers=16):
    """hash_with_ds_dynamic of every node of an arity-16 level (all nodes full) under the host-check set h, through the REFERENCE's dense rounds
    (hc_permute_dense: M and the round constants as given, none of the kernel-form tables): the stream [16, level, pos, label] || 16 children || 1
    is two permutations, the second after children 12..15 and the closing 1 went into elements 0..4.  The states are cut into `workers` slices
    permuted side by side (the library call releases the interpreter lock)."""
    p = pyref.P_PALLAS
    ch = A(children).reshape(-1, 16, 4); nodes = ch.shape[0]
    st = np.zeros((nodes, 17, 4), np.uint64)
    st[:, 0] = from_u64(16); st[:, 1] = from_u64(level); st[:, 3] = from_u64(label)
    for k in range(nodes):
        st[k, 2] = from_u64(pos0 + k)
    st[:, 4:16] = ch[:, :12]

    def permute(x):
        cuts = np.array_split(np.arange(nodes), workers)
        with ThreadPoolExecutor(workers) as ex:
            parts = list(ex.map(lambda idx: hc.permute_dense(h, x[idx].reshape(-1, 4), 17).reshape(-1, 17, 4), [c for c in cuts if len(c)]))
        return np.concatenate(parts)
    st = permute(st)
    one = cv.raw_to_int(from_u64(1))
    for k in range(nodes):
        for j in range(5):
            add = cv.raw_to_int(ch[k, 12 + j]) if j < 4 else one
            st[k, j] = cv.raw((cv.raw_to_int(st[k, j]) + add) % p)
    return permute(st)[:, 0].copy()
