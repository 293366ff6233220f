"""Shape matrix of the LDE tests and a restatement of the route the first pass of the big forward transform takes (test
infrastructure, plain Python).

`lde_run` (csrc/capi_ntt.hip) interpolates, then transforms 2^(log_n + lb) points of which only the first 2^log_n are non-zero.  When
the big plan has a strided first pass whose stride is at most n, the padding is never written: the pass gets
nz_points = 2^(b0 - lb) and `k_ntt_strided` (csrc/ntt_dev.hpp) treats the points p >= nz_points of every sub-NTT as zero in one of
several ways.  Which one depends on the blow-up, on the plan split and on whether a coset pre-scale is applied — restated here from
the conditions in those two files, so that the tests can name the route a shape exercises and prove that every route is exercised."""

NO_EXTENSION = "no extension (lb == 0)"
PADDED = "real padding (k_zero_fill)"
FAST = "fast head, no zero groups (nz == B/8)"
FAST_ZERO = "fast head, zero-group loop (1 < nz < B/8)"
FAST_ZERO_ONE = "fast head, zero-group loop, nz == 1"
GENERAL = "general pre-scale path, points p >= nz zeroed (nz > B/8)"
UNIT = "no pre-scale, zeros inside head_dispatch"

SKIP_COSET = (FAST, FAST_ZERO, FAST_ZERO_ONE, GENERAL)      # routes that never write the padding and read a coset pre-scale


def split(log_n):
    """pass sizes [b0, b1, b2][:P] of get_plan for a transform of 2^log_n points"""
    if log_n <= 10:
        return [log_n]
    if log_n <= 20:
        b0 = (log_n + 1) // 2
        return [b0, log_n - b0]
    b0 = (log_n + 2) // 3
    b1 = (log_n - b0 + 1) // 2
    return [b0, b1, log_n - b0 - b1]


def passes(log_n, lb):
    """number of passes of the big forward transform of an LDE 2^log_n -> 2^(log_n + lb)"""
    return len(split(log_n + lb))


def route(log_n, lb, pre):
    """(P, route name) of the big forward transform's first pass; pre: a coset pre-scale is applied (shift given and != 1)"""
    s = split(log_n + lb)
    P, b0 = len(s), s[0]
    if lb == 0:
        return P, NO_EXTENSION
    skip = P > 1 and log_n + lb - b0 <= log_n
    if not skip:
        return P, PADDED
    nz, B = 1 << (b0 - lb), 1 << b0
    if not pre:
        return P, UNIT
    if b0 >= 3 and nz <= B >> 3:
        return P, FAST if nz == B >> 3 else FAST_ZERO_ONE if nz == 1 else FAST_ZERO
    return P, GENERAL


def all_routes():
    """every (P, route name, pre) the library can take, enumerated from the conditions above over all shapes up to 2^24 outputs"""
    out = set()
    for log_n in range(0, 25):
        for lb in range(0, 25 - log_n):
            for pre in (0, 1):
                out.add(route(log_n, lb, pre) + (pre,))
    return out


# (log_n, lb): every route for P = 1, 2, 3 with and without pre-scale, including nz == 1 and nz == B/2; log_n + lb <= 21 so that one
# oracle LDE stays around a second
SHAPES = [(0, 3), (3, 0), (3, 3), (8, 2), (8, 3), (7, 4), (5, 6), (4, 7), (10, 1), (9, 2), (11, 0), (12, 4), (11, 5), (14, 6), (10, 10),
          (16, 4), (17, 4), (16, 5), (15, 6), (14, 7), (13, 8), (19, 2), (20, 1), (18, 3), (21, 0)]
