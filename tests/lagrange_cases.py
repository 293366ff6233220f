"""Shared inputs of the lagrange_eval_on_h tests (test_lagrange_eval_host.py on the CPU, test_gpu_lagrange_eval.py on the device): the shape matrix, seeded
columns and points, the points inside H, the stored-limb corner sets, the ctypes wrapper of the host instantiation hc_lagrange_eval_batch
(csrc/hostcheck.cpp), and the three references, none of which touches the code under test:

  R1  the reference's own function: oracle.ali_merge(v, ones, zeros, zeros, omega, z) returns c* = lagrange_eval_on_h(v, z, omega) / (z^n - 1)
      (oracle/fri.hpp), multiplied back by z^n - 1.  n >= 2, z outside H.
  R2  the definition: the coefficients by the oracle's inverse NTT, evaluated by Horner (oracle.poly_eval_many).  Every z, inside H too.
  R3  z = omega^j gives v[j]; n = 1 gives v[0].

R1 and R2 agree byte for byte (test_lagrange_eval_host.py keeps that as a test), so equality, not a tolerance, is the criterion everywhere."""
import ctypes as C

import numpy as np

import corner_values as cv
import pyref

N_MATRIX = (1, 2, 8, 64, 256, 1 << 11, 1 << 12, 1 << 14)       # 2^11: one tile at K = 8; 2^12: two workgroups, the finish sums more than one partial
NCOLS = (1, 3, 4, 9)
NPOINTS = (1, 2, 5)
MAX_COLS, MAX_POINTS = max(NCOLS), max(NPOINTS)
K, THREADS = 8, 256                                            # csrc/lagrange_dev.hpp: kLagK positions per lane, 256-thread workgroups
DEFAULT_MAX_PARTIALS = 1 << 21
P = pyref.P_PALLAS
SEED = 0x1A64
vp = C.c_void_p
_cache = {}


def workgroups(n):
    """workgroups per column of k_lagrange_partials (lag_geom)"""
    return -(-(-(-n // K)) // THREADS)


def expected_passes(n, ncols, n_outside, max_partials=DEFAULT_MAX_PARTIALS):
    """partial passes of one call: points outside H only, max_partials // (ncols * workgroups) of them per pass and never fewer than one"""
    if not n_outside or not ncols:
        return 0
    per = min(max(max_partials // (ncols * workgroups(n)), 1), n_outside)
    return -(-n_outside // per)


def columns(oracle, n, ncols=MAX_COLS):
    key = ("cols", n)
    if key not in _cache:
        _cache[key] = [oracle.synth_column(SEED + n, c, 0, n) for c in range(MAX_COLS)]
    return _cache[key][:ncols]


def points(oracle, n, npoints=MAX_POINTS):
    """seeded stored elements: outside H (a random element is an n-th root of unity with probability n / r)"""
    key = ("pts", n)
    if key not in _cache:
        _cache[key] = oracle.synth_column(SEED + 0x100 + n, 0, 0, MAX_POINTS)
    return _cache[key][:npoints]


def omega_of(oracle, n):
    return oracle.domain_omega(n) if n > 1 else oracle.from_u64(1)


def coefficients(oracle, v):
    return oracle.ntt(0, v, inverse=True) if v.shape[0] > 1 else np.array(v, np.uint64)


def r2(oracle, cols, zs):
    """(P, C, 4): the definition, over the radix-2 generator of size n"""
    zs = np.ascontiguousarray(zs, np.uint64).reshape(-1, 4)
    per_col = [oracle.poly_eval_many(0, coefficients(oracle, v), zs) if v.shape[0] > 1 else np.tile(v[0], (zs.shape[0], 1)) for v in cols]
    return np.stack(per_col, axis=1)


def r1(oracle, cols, zs, omega=None):
    """(P, C, 4): c* of the oracle's merge with s = 1, e = t = 0, times z^n - 1"""
    n = cols[0].shape[0]; assert n >= 2
    omega = omega_of(oracle, n) if omega is None else omega
    one = oracle.from_u64(1); ones = np.tile(one, (n, 1)); zeros = np.zeros((n, 4), np.uint64)
    zs = np.ascontiguousarray(zs, np.uint64).reshape(-1, 4)
    return np.stack([np.stack([oracle.mul(oracle.ali_merge(v, ones, zeros, zeros, omega, z)[1], oracle.sub(oracle.pow(z, n), one)) for v in cols]) for z in zs])


def matrix_reference(oracle, n):
    """R2 of the MAX_COLS seeded columns at the MAX_POINTS seeded points of size n, computed once ((P, C, 4); R3 at n = 1)"""
    key = ("ref", n)
    if key not in _cache:
        _cache[key] = r2(oracle, columns(oracle, n), points(oracle, n))
    return _cache[key]


def inside_points(oracle, n):
    """[(z, j)] with z = omega^j: 1, -1, omega^(n-1), a j of the second workgroup's tile at n = 2^12 (lane 300 of the launch, second position), and the first again"""
    w = omega_of(oracle, n); one = oracle.from_u64(1)
    js = [0] + ([n // 2, n - 1] if n >= 2 else []) + ([300 + workgroups(n) * THREADS] if n >= 1 << 12 else []) + [0]
    out = []
    for j in js:
        z = oracle.sub(np.zeros(4, np.uint64), one) if (n >= 2 and j == n // 2) else oracle.pow(w, j)
        out.append((z, j))
    return out


def corners():
    return cv.raw_array(cv.stored_corners(P))


def corner_columns(n, ncols):
    """columns whose stored limbs are the corners of corner_values.stored_corners: 0, 1, r - 1, the Montgomery one and its negative, limb edges"""
    c = corners(); L = c.shape[0]
    return [c[(np.arange(n) * (2 * b + 1) + 5 * b) % L] for b in range(ncols)]


def third_power_domain(oracle, v):
    """(omega^3, u): the column v read over the generator omega^3 (v[j] is the value at omega^(3 j)) is the column u over omega"""
    n = v.shape[0]; u = np.zeros_like(v); u[(3 * np.arange(n)) % n] = v
    return oracle.pow(omega_of(oracle, n), 3), u


def hc_eval_rc(hostcheck, cols, n, zs, omega=None, max_partials=0):
    """hc_lagrange_eval_batch: the driver of stark_lagrange_eval_on_h_batch_dev, every workgroup in lockstep on the host -> (rc, (P, C, 4), passes).
    A column object that repeats in `cols` is passed as a repeated pointer.  max_partials 0: the default."""
    f = hostcheck.l.hc_lagrange_eval_batch
    f.argtypes = [C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(C.c_size_t)]; f.restype = C.c_int
    keep = {id(v): np.ascontiguousarray(v, dtype=np.uint64) for v in cols}
    assert all(a.shape == (n, 4) for a in keep.values())
    ptrs = (vp * max(len(cols), 1))(*[keep[id(v)].ctypes.data for v in cols])
    z = np.ascontiguousarray(zs, dtype=np.uint64).reshape(-1, 4); npts = z.shape[0]
    w = None if omega is None else np.ascontiguousarray(omega, dtype=np.uint64)
    out = np.full((npts, len(cols), 4), 0x5A5A5A5A5A5A5A5A, np.uint64); passes = C.c_size_t(99)
    rc = f(len(cols), ptrs, n, None if w is None else w.ctypes.data_as(vp), npts, z.ctypes.data_as(vp) if npts else None, max_partials, out.ctypes.data_as(vp), C.byref(passes))
    return rc, out, passes.value


def hc_eval(hostcheck, cols, n, zs, omega=None, max_partials=0):
    """hc_eval_rc of a call that succeeds -> ((P, C, 4), passes)"""
    rc, out, passes = hc_eval_rc(hostcheck, cols, n, zs, omega=omega, max_partials=max_partials)
    assert rc == 0, rc
    return out, passes


def hc_refused(hostcheck, n, omega):
    """True when the host instantiation refuses (n, omega) as the entry point does"""
    f = hostcheck.l.hc_lagrange_eval_batch
    f.argtypes = [C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(C.c_size_t)]; f.restype = C.c_int
    assert n <= 4 or n > 1 << 30 or n & (n - 1), "a size that may be accepted must fit the four-row column below"
    col = np.zeros((4, 4), np.uint64); z = np.zeros((1, 4), np.uint64); out = np.zeros((1, 4), np.uint64)
    w = None if omega is None else np.ascontiguousarray(omega, dtype=np.uint64)
    return f(1, (vp * 1)(col.ctypes.data), n, None if w is None else w.ctypes.data_as(vp), 1, z.ctypes.data_as(vp), 0, out.ctypes.data_as(vp), None) == -1
