"""Shared inputs of the sharded lagrange_eval_on_h tests (test_lagrange_shard_host.py on the CPU, test_gpu_lagrange_shard.py on the device): the
partition matrix, the mixed points of a partition, 17 seeded columns for the column groups, and the ctypes wrappers of the host instantiations
hc_lagrange_eval_shard / hc_lagrange_eval_from_partials / hc_lagrange_shard_header / hc_lagrange_headers_agree / hc_lagrange_col_groups
(csrc/hostcheck.cpp).  Columns, seeded points and the reference R2 (the oracle's inverse NTT plus Horner) are lagrange_cases.py's; equality, not a
tolerance, is the criterion everywhere."""
import ctypes as C

import numpy as np

import lagrange_cases as lc

vp = C.c_void_p
HDR_WORDS = 8                                                  # csrc/lagrange_dev.hpp: kLagHdrWords
GROUPS = (1, 2, 3, 9, 64)                                      # an uneven last group (17 columns in 2, 3 or 9) and more groups than columns
GROUP_NCOLS = (9, 17)
_cache = {}


def even(n, W):
    return [(q * (n // W), n // W) for q in range(W)]


# (n_global, [(j0, n_local)]): one row per block; one workgroup owns 256 lanes x 8 positions = 2048 rows
PARTITIONS = [(8, even(8, 8)),                                 # n_local = 1
              (8, even(8, 2)),
              (256, even(256, 4)),
              (1 << 12, even(1 << 12, 2)),                     # one full tile per block
              (1 << 12, even(1 << 12, 4)),                     # n_local = 1024: one workgroup, half of its K positions dead
              (1 << 12, [(0, 1000), (1000, 1), (1001, 3095)]),  # uneven blocks; the last one has two workgroups and a ragged end
              (1 << 14, even(1 << 14, 2)),                     # four workgroups per block: the finish sums several partials
              (1 << 14, even(1 << 14, 8))]
PARTITION_IDS = ["n%d-%s" % (n, "x".join(str(l) for _, l in b) if len(set(l for _, l in b)) > 1 else "W%d" % len(b)) for n, b in PARTITIONS]


def inside_js(n, blocks):
    """j = 0, n/2, n - 1, the first and last index of the second block, and j = 0 again"""
    j0, nl = blocks[1]
    return [0, n // 2, n - 1, j0, j0 + nl - 1, 0]


def mixed_points(oracle, n, blocks):
    """-> (zs (8, 4), [(index in zs, j)]): the two seeded points outside H around the points inside H of inside_js"""
    key = ("mixed", n, tuple(blocks))
    if key not in _cache:
        w = lc.omega_of(oracle, n); outs = lc.points(oracle, n, 2); js = inside_js(n, blocks)
        zs = np.ascontiguousarray(np.stack([outs[0]] + [oracle.pow(w, j) for j in js] + [outs[1]]))
        _cache[key] = (zs, [(1 + q, j) for q, j in enumerate(js)])
    return _cache[key]


def reference(oracle, n, blocks, ncols=3):
    """R2 of the first ncols seeded columns at mixed_points, computed once per (n, points)"""
    zs, _ = mixed_points(oracle, n, blocks)
    key = ("ref", n, zs.tobytes())
    if key not in _cache:
        _cache[key] = lc.r2(oracle, lc.columns(oracle, n, 3), zs)
    return _cache[key][:, :ncols]


def columns17(oracle, n):
    """17 distinct seeded columns: lagrange_cases' nine and eight more"""
    key = ("cols17", n)
    if key not in _cache:
        _cache[key] = lc.columns(oracle, n) + [oracle.synth_column(lc.SEED + 0x200 + n, c, 0, n) for c in range(17 - lc.MAX_COLS)]
    return _cache[key]


def reference17(oracle, n, zs):
    key = ("ref17", n, np.ascontiguousarray(zs).tobytes())
    if key not in _cache:
        _cache[key] = lc.r2(oracle, columns17(oracle, n), zs)
    return _cache[key]


def block_rows(cols, j0, nl):
    return [np.ascontiguousarray(v[j0:j0 + nl]) for v in cols]


# ---- the host instantiations ---------------------------------------------------------------------------------------------------------------
def _w(omega):
    return None if omega is None else np.ascontiguousarray(omega, dtype=np.uint64)


def hc_shard_rc(hostcheck, rows, n_local, j0, n_global, zs, omega=None, max_partials=0, col_groups=-1):
    """hc_lagrange_eval_shard on the block's rows -> (rc, (P, C, 4) shares, passes); the output starts as 0x5A bytes"""
    f = hostcheck.l.hc_lagrange_eval_shard
    f.argtypes = [C.c_size_t, vp, C.c_size_t, C.c_uint64, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp, C.POINTER(C.c_size_t)]; f.restype = C.c_int
    keep = {id(v): np.ascontiguousarray(v, dtype=np.uint64) for v in rows}
    ptrs = (vp * max(len(rows), 1))(*[keep[id(v)].ctypes.data for v in rows])
    z = np.ascontiguousarray(zs, dtype=np.uint64).reshape(-1, 4); npts = z.shape[0]; w = _w(omega)
    out = np.full((npts, len(rows), 4), 0x5A5A5A5A5A5A5A5A, np.uint64); passes = C.c_size_t(99)
    rc = f(len(rows), ptrs, n_local, j0, n_global, None if w is None else w.ctypes.data_as(vp), npts, z.ctypes.data_as(vp) if npts else None, max_partials, col_groups,
           out.ctypes.data_as(vp), C.byref(passes))
    return rc, out, passes.value


def hc_shard(hostcheck, rows, n_local, j0, n_global, zs, **kw):
    rc, out, passes = hc_shard_rc(hostcheck, rows, n_local, j0, n_global, zs, **kw)
    assert rc == 0, rc
    return out, passes


def hc_from_partials_rc(hostcheck, parts, ncols, n_global, zs, omega=None):
    """hc_lagrange_eval_from_partials on the stacked shares ((W, P, C, 4)) -> (rc, (P, C, 4))"""
    f = hostcheck.l.hc_lagrange_eval_from_partials
    f.argtypes = [C.c_size_t, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, vp, vp]; f.restype = C.c_int
    z = np.ascontiguousarray(zs, dtype=np.uint64).reshape(-1, 4); npts = z.shape[0]; w = _w(omega)
    p = np.ascontiguousarray(parts, dtype=np.uint64); nparts = p.shape[0] if p.size else 0
    out = np.full((npts, ncols, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
    rc = f(nparts, p.ctypes.data_as(vp) if p.size else None, ncols, n_global, None if w is None else w.ctypes.data_as(vp), npts, z.ctypes.data_as(vp), out.ctypes.data_as(vp))
    return rc, out


def hc_partitioned(hostcheck, cols, n, blocks, zs, omega=None, max_partials=0, col_groups=-1):
    """shard per block, then from_partials -> ((P, C, 4) result, (W, P, C, 4) shares, [passes per block])"""
    shares, passes = [], []
    for j0, nl in blocks:
        s, k = hc_shard(hostcheck, block_rows(cols, j0, nl), nl, j0, n, zs, omega=omega, max_partials=max_partials, col_groups=col_groups)
        shares.append(s); passes.append(k)
    shares = np.stack(shares)
    rc, out = hc_from_partials_rc(hostcheck, shares, len(cols), n, zs, omega=omega)
    assert rc == 0, rc
    return out, shares, passes


def hc_header(hostcheck, n_global, ncols, zs, omega):
    f = hostcheck.l.hc_lagrange_shard_header
    f.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, vp]; f.restype = C.c_int
    z = np.ascontiguousarray(zs, dtype=np.uint64).reshape(-1, 4); w = _w(omega); out = np.zeros(HDR_WORDS, np.uint64)
    assert f(n_global, ncols, z.shape[0], w.ctypes.data_as(vp), z.ctypes.data_as(vp), out.ctypes.data_as(vp)) == HDR_WORDS
    return out


def hc_headers_agree(hostcheck, headers, mine):
    f = hostcheck.l.hc_lagrange_headers_agree
    f.argtypes = [vp, C.c_size_t, vp]; f.restype = C.c_int
    a = np.ascontiguousarray(np.stack(headers), dtype=np.uint64); m = np.ascontiguousarray(mine, dtype=np.uint64)
    return bool(f(a.ctypes.data_as(vp), a.shape[0], m.ctypes.data_as(vp)))


def hc_col_groups(hostcheck, opt, ncols, n_local, pass_points):
    """-> (column groups of the launch, columns per group) of the driver's rule (lag_col_groups)"""
    f = hostcheck.l.hc_lagrange_col_groups
    f.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]; f.restype = C.c_uint
    per = C.c_size_t(0); g = f(opt, ncols, n_local, pass_points, C.byref(per))
    return g, per.value
