"""Shared cases of the ragged prove tail (option "mixed_prove_tail"; stark_mlwe_amd/csrc/fri_mixed.hpp), used by tests/test_fri_mixed_host.py (the host
twin) and tests/test_gpu_mixed_tail.py (the device)."""
import ctypes as C

import numpy as np

vp = C.c_void_p
SEED_Z = 0xDEEFBAAD

# the twelve traces (n0, schedule, r), classes interleaved in the caller's order
TRACES = [
    (1 << 6, [4, 2], 4),      # 0  base trace of the [4,2] class
    (1 << 10, [16, 8], 8),    # 1  base trace of the [16,8] class
    (1 << 3, [4, 2], 4),      # 2  layers 8, 2, 1: a one-element last layer beside arity-2 ones
    (1 << 7, [128], 4),       # 3  a class of one trace: the single commit
    (1 << 12, [16, 8], 4),    # 4  two merge blocks, so the stride is not 1
    (1 << 8, [], 4),          # 5  L = 0
    (1 << 11, [4, 2], 8),     # 6  exactly one merge block of 2048 elements
    (1 << 7, [16, 8], 8),     # 7  layers 128, 8, 1 in a hashed class
    (2, [], 4),               # 8  the smallest domain
    (1 << 6, [4, 2], 2),      # 9  the size of trace 0 with another r: shared z, different query counts
    (1 << 10, [16, 8], 8),    # 10 the shape of trace 1 with other data
    (1 << 13, [16, 8], 4),    # 11 four merge blocks; the other traces exit early
]
CLASS_OF = [0, 1, 0, 2, 1, 3, 0, 1, 3, 0, 1, 1]
CLASS_ORDER = [0, 2, 6, 9, 1, 4, 7, 10, 11, 3, 5, 8]
PASS_ROWS = 5000                                   # prove_batch_max_rows of the pass tests: the [16,8] class becomes {1}, {4, 7}, {10}, {11}
# the classes of the host root test (n0 per trace); [128] is left out there: its host constants take about 100 s to derive
HOST_CLASSES = [([4, 2], [8, 64, 64, 2048]), ([16, 8], [128, 1024, 1024]), ([], [2, 256])]


def flat_schedules(scheds):
    flat, off = [], [0]
    for s in scheds:
        flat += list(s); off.append(len(flat))
    return (C.c_size_t * max(len(flat), 1))(*flat), (C.c_size_t * (len(scheds) + 1))(*off)


def classes_of(hc, shapes):
    """hc_mixed_prove_classes over shapes [(n0, schedule, r)] -> (class of every trace, the traces class by class, number of classes)"""
    B = len(shapes)
    sch, offs = flat_schedules([s[1] for s in shapes])
    cls = (C.c_size_t * B)(); order = (C.c_size_t * B)()
    hc.l.hc_mixed_prove_classes.restype = C.c_size_t
    nc = hc.l.hc_mixed_prove_classes(C.c_size_t(B), sch, offs, cls, order)
    return list(cls), list(order), nc


def passes_of(hc, n0s, max_rows, max_traces=32768):
    """hc_mixed_prove_passes -> the traces per pass"""
    B = len(n0s); out = (C.c_size_t * B)()
    hc.l.hc_mixed_prove_passes.restype = C.c_size_t
    k = hc.l.hc_mixed_prove_passes(C.c_size_t(B), (C.c_size_t * B)(*n0s), C.c_size_t(max_rows), C.c_size_t(max_traces), out, C.c_size_t(B))
    return list(out)[:k]


def commit_mixed(hc, tp, f0s, sched, seed_z=SEED_Z):
    """hc_fri_commit_mixed over host layers f0s (any lengths, one schedule) -> roots[b][l]"""
    B, L = len(f0s), len(sched)
    f0s = [np.ascontiguousarray(f, dtype=np.uint64) for f in f0s]
    tab = (vp * B)(*[f.ctypes.data for f in f0s]); n0 = (C.c_size_t * B)(*[f.shape[0] for f in f0s])
    sch = (C.c_size_t * max(L, 1))(*sched); roots = np.zeros((B, L + 1, 4), np.uint64)
    rc = hc.l.hc_fri_commit_mixed(tp, C.c_size_t(B), tab, n0, sch, C.c_size_t(L), C.c_uint64(seed_z), roots.ctypes.data_as(vp))
    assert rc == 0, rc
    return roots


def commit_steps(hc, n0s, sched):
    """hc_fri_commit_mixed_steps -> dict of the driver's census"""
    B, L = len(n0s), len(sched); out = (C.c_size_t * 7)()
    rc = hc.l.hc_fri_commit_mixed_steps(C.c_size_t(B), (C.c_size_t * B)(*n0s), (C.c_size_t * max(L, 1))(*sched), C.c_size_t(L), out)
    assert rc == 0, rc
    return dict(zip(("folds", "leaf_pairs", "pair_streams", "levels", "blocks", "zpows", "gathers"), list(out)))


def ragged_pairs_level(hc, params, arity, labels, segs, in1, cp_div):
    """hc_hash_ds_ragged_pairs_level: segs = the trees' layers, in1 = the launch's one partner array (or None) -> the hashes back to back"""
    n_seg = len(segs); segs = [np.ascontiguousarray(s, dtype=np.uint64) for s in segs]
    tab = (vp * n_seg)(*[s.ctypes.data for s in segs]); n_in = (C.c_size_t * n_seg)(*[s.shape[0] for s in segs])
    lab = (C.c_uint64 * n_seg)(*labels); total = sum(s.shape[0] for s in segs); out = np.zeros((total, 4), np.uint64)
    in1 = None if in1 is None else np.ascontiguousarray(in1, dtype=np.uint64)
    hc.l.hc_hash_ds_ragged_pairs_level.restype = C.c_long
    k = hc.l.hc_hash_ds_ragged_pairs_level(params, C.c_size_t(arity), C.c_size_t(n_seg), lab, tab, n_in, None if in1 is None else in1.ctypes.data_as(vp),
                                           C.c_size_t(0 if in1 is None else in1.shape[0]), C.c_size_t(cp_div), out.ctypes.data_as(vp))
    assert k == total, k
    return out


def fold_ragged(hc, f, first_out, zp_off, zp, m):
    f = np.ascontiguousarray(f, dtype=np.uint64); zp = np.ascontiguousarray(zp, dtype=np.uint64); k = len(first_out)
    out = np.zeros((f.shape[0] // m, 4), np.uint64)
    rc = hc.l.hc_fri_fold_ragged(f.ctypes.data_as(vp), C.c_size_t(f.shape[0]), (C.c_uint64 * k)(*first_out), (C.c_uint64 * k)(*zp_off), C.c_size_t(k), zp.ctypes.data_as(vp),
                                 C.c_size_t(zp.shape[0]), C.c_size_t(m), out.ctypes.data_as(vp))
    assert rc == 0, rc
    return out


def layer_sizes(n0, sched):
    n = [n0]
    for m in sched:
        n.append(n[-1] // m)
    return n


def pick_arity(n, m):
    for a in (128, 64, 32, 16, 8, 4):
        if m >= a and n % a == 0:
            return a
    return 2 if n % 2 == 0 else 1


def tree_levels(n, arity):
    k = 1
    while n > 1:
        n = (n + arity - 1) // arity; k += 1
    return k
