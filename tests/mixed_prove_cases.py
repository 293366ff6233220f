"""Shared cases of the ragged transcript hash (stark_tr_hash_many_dev / hc_tr_hash_many) and of the mixed-size prover's grouping, used by
tests/test_mixed_prove_host.py (host twin) and tests/test_gpu_mixed_prove.py (device)."""
import ctypes as C

import numpy as np

vp = C.c_void_p
TAGS = [b"ALI/A", b"ALI/seed", b"FRI/index", b"FRI/seed"]
BOUNDARIES = (15, 16, 17, 31, 32, 33)            # absorbed lengths around one and two rate blocks of the lazy duplex at rate 16
COUNTS = (1, 4, 5, 70)
POOL_ROWS = 104                                  # the longest item reads rows off .. off + 100, off <= 3
SEED = 0x4A66ED


def frame_dims(hc, tag):
    """(np, ns) of a tag's frame, from the product's own host::tr_hash_frame"""
    a, b = C.c_int(), C.c_int()
    assert hc.l.hc_tr_frame_dims(tag, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def lengths_for(hc, tag):
    """the k of a tag's items: np + k + ns on every boundary the frame allows, then k = 0, 1, 100"""
    np_, ns = frame_dims(hc, tag)
    return [T - np_ - ns for T in BOUNDARIES if T - np_ - ns >= 0] + [0, 1, 100]


def items_for(hc, count):
    """count items (tag, offset into the pool, k): the tags in rotation, each tag walking through lengths_for(tag); items 0 and 4 (and every
    j, j + 4) read from the same pool offset, so a pointer is used more than once as soon as count >= 5"""
    out = []
    for j in range(count):
        tag = TAGS[j % 4]; ks = lengths_for(hc, tag)
        out.append((tag, j % 4, ks[(j // 4) % len(ks)]))
    return out


def pool(oracle):
    return oracle.rand_fr_columns(SEED, POOL_ROWS, 1)[0]


def oracle_digests(oracle, pl, items):
    return np.stack([oracle.tr_hash_fields_tagged(tag, pl[off:off + k]) for tag, off, k in items])


def total_of(hc, item):
    np_, ns = frame_dims(hc, item[0])
    return np_ + item[2] + ns


def hc_hash_many(hc, tp, pl, items):
    """hc_tr_hash_many over host pointers into `pl` -> (digests in the caller's order, launch order)"""
    n = len(items)
    tags = (C.c_char_p * n)(*[it[0] for it in items])
    flds = (vp * n)(*[(pl.ctypes.data + 32 * it[1]) if it[2] else None for it in items])
    ks = (C.c_size_t * n)(*[it[2] for it in items])
    out = np.zeros((n, 4), np.uint64); order = (C.c_size_t * n)()
    assert hc.l.hc_tr_hash_many(tp, C.c_size_t(n), tags, flds, ks, out.ctypes.data_as(vp), order) == 0
    return out, list(order)


def groups_of(hc, shapes):
    """hc_mixed_prove_groups over shapes [(n0, schedule, r)] -> (group of every trace, the traces group by group, number of groups)"""
    B = len(shapes)
    flat, off = [], [0]
    for _, sched, _ in shapes:
        flat += list(sched); off.append(len(flat))
    n0 = (C.c_size_t * B)(*[s[0] for s in shapes]); r = (C.c_size_t * B)(*[s[2] for s in shapes])
    sch = (C.c_size_t * max(len(flat), 1))(*flat); offs = (C.c_size_t * (B + 1))(*off)
    grp = (C.c_size_t * B)(); order = (C.c_size_t * B)()
    hc.l.hc_mixed_prove_groups.restype = C.c_size_t
    ng = hc.l.hc_mixed_prove_groups(C.c_size_t(B), n0, sch, offs, r, grp, order)
    return list(grp), list(order), ng


# the mixed prove of the GPU test: shapes of tests/test_gpu_prove_batch_tail.py, a group of three, a group of two and two singletons, interleaved
PROVE_SHAPES = {6: ([4, 2], 4), 7: ([128], 4), 8: ([], 4), 10: ([16, 8], 8)}
PROVE_ORDER = [6, 10, 6, 7, 8, 6, 10]
