"""tools/lagrange_eval_timing.py — stark_lagrange_eval_on_h_batch_dev against the only route to the same values without it, and its two floors.

    python tools/lagrange_eval_timing.py LIB [OUT.jsonl]     (default profiles/lagrange_eval_timing.jsonl)

Shapes (the library's own workloads): n = 2^20 with C = 4 columns at P = 1 and P = 2 points, n = 2^16 with C = 64 at P = 2, n = 2^23 with C = 1 at P = 1.
Variants, alternated in one process, every shape warmed up first, REPS repetitions each, every repetition between stark_timer_start / stop (HIP events):
  batch_wide / batch_plain   one stark_lagrange_eval_on_h_batch_dev call, a lane's products of a column through the lazy accumulator ("lagrange_wide_acc" 1)
                             or as products and additions (0); the two results are checked equal first;
  merge_route                C * P calls of stark_ali_merge_dev with s = ones, e = t = zeros, reading c* (each call writes an f0 nobody wants and
                             synchronises: that is its contract, and what a caller of it pays).
Each line carries the median and the spread (min, max) of every variant and the two floors of DESIGN §4.5a:
  hbm_floor_ms   C n 32 bytes (every column read once; the P - 1 re-reads of a tile are L2's) over the measured copy peak 6.29 TB/s;
  mac_floor_ms   field products x 96 MACs over stark_diag_mac_rate measured in the same run; products = P n (5.75 + C) + P W 381, W the workgroups
                 per column: per (point, position) 7/8 prefix + 12/8 scan + 5/8 lane inverse + 22/8 peel, per (point, position, column) 1, and one
                 Fermat inversion (254 squarings + 127 products) per (point, workgroup);
and the achieved fraction of the binding (larger) floor.

    python tools/lagrange_eval_timing.py LIB OUT.jsonl shared     (profiles/lagrange_shared_timing.jsonl)

measures the options "lagrange_shared_inverse" and "lagrange_share_cosets" instead: the arms opt_00, opt_10, opt_01, opt_11 (shared inverse, cosets) of
one stark_lagrange_eval_on_h_batch_dev call, alternated, the results checked byte-equal first, for the four shapes above with random points
(points "random"), for the two-point shapes with the DEEP pair (z, z w) (points "pair") and for n = 2^20, C = 4 at sixteen shifts z w^s of one z
(points "shifts").  Each line carries the same two floors (the MAC floor is option 0's: it counts one inversion per workgroup and one weight set per
point), over_opt_00 = median(arm) / median(opt_00) and slower_beyond_spread: the arms whose median exceeds opt_00's by more than the spread
(max - min) of either arm."""
import ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import stark_mlwe_amd._abi as abi
path = os.path.abspath(sys.argv[1]); abi.lib_path = lambda: path
from stark_mlwe_amd.api import Context, root_of_unity
dev = torch.device("cuda", 0)
ctx = Context(0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)); lib = ctx.lib
rng = np.random.default_rng(0x1A64)
REPS = 20
HBM_BPS = 6.29e12
SHAPES = ((20, 4, 1), (20, 4, 2), (16, 64, 2), (23, 1, 1))
MONT_ONE = np.array([0x5b2b3e9cfffffffd, 0x992c350be3420567, 0xffffffffffffffff, 0x3fffffffffffffff], np.uint64)    # 2^256 mod r (Pallas Fr), csrc/fr.hpp

def synth(seed, col, n):
    t = torch.empty((n, 4), dtype=torch.int64, device=dev)
    ctx._chk(lib.stark_synth_column_dev(ctx.h, seed, col, 0, n, C.c_void_p(t.data_ptr()))); return t

def timed(fn):
    ms = C.c_float(); ctx._chk(lib.stark_timer_start(ctx.h)); fn(); ctx._chk(lib.stark_timer_stop_ms(ctx.h, C.byref(ms))); return ms.value

def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5)}

mac_rate = C.c_double(); ctx._chk(lib.stark_diag_mac_rate(ctx.h, C.byref(mac_rate)))

def shape_row(lg, ncols, npoints):
    n = 1 << lg
    cols = [synth(0x1A64 + lg, c, n) for c in range(ncols)]; ptrs = [t.data_ptr() for t in cols]
    zs = np.ascontiguousarray(rng.integers(0, 1 << 62, size=(npoints, 4), dtype=np.uint64))          # stored limbs below 2^254 < r: outside H
    omega = root_of_unity(lg)
    ones = torch.from_numpy(np.tile(MONT_ONE, (n, 1)).view(np.int64)).to(dev); zeros = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    f0 = torch.empty((n, 4), dtype=torch.int64, device=dev); cs = np.zeros(4, np.uint64)
    out = {v: torch.zeros((npoints * ncols, 4), dtype=torch.int64, device=dev) for v in ("batch_wide", "batch_plain")}
    vp = C.c_void_p
    def batch(wide, o):
        def run(): ctx.lagrange_eval_on_h_batch_dev(ptrs, n, zs, o.data_ptr())
        return run
    def merge_route():
        for p in range(npoints):
            for c in range(ncols):
                ctx._chk(lib.stark_ali_merge_dev(ctx.h, vp(ptrs[c]), vp(ones.data_ptr()), vp(zeros.data_ptr()), vp(zeros.data_ptr()), None, None,
                                                 omega.ctypes.data_as(vp), zs[p].ctypes.data_as(vp), n, vp(f0.data_ptr()), cs.ctypes.data_as(vp)))
    variants = {"batch_wide": (1, batch(True, out["batch_wide"])), "batch_plain": (0, batch(False, out["batch_plain"])), "merge_route": (-1, merge_route)}
    times = {v: [] for v in variants}
    for rep in range(REPS + 1):                                       # repetition 0 is the warm-up of this shape
        for v, (acc, fn) in variants.items():
            ctx.set_option("lagrange_wide_acc", acc)
            t = timed(fn)
            if rep: times[v].append(t)
        if not rep:
            ctx.sync(); assert torch.equal(out["batch_wide"], out["batch_plain"]), (lg, ncols, npoints)
    ctx.set_option("lagrange_wide_acc", -1)
    W = -(-(-(-n // 8)) // 256)
    products = npoints * n * (5.75 + ncols) + npoints * W * 381
    hbm_ms = 1e3 * ncols * n * 32 / HBM_BPS; mac_ms = 1e3 * products * 96 / mac_rate.value
    row = {"log_n": lg, "ncols": ncols, "npoints": npoints, "reps": REPS, "lane_macs_per_s": mac_rate.value, "hbm_floor_ms": round(hbm_ms, 5), "mac_floor_ms": round(mac_ms, 5),
           "binding_floor": "mac" if mac_ms >= hbm_ms else "hbm"}
    for v in variants: row[v] = stats(times[v])
    best = min(row["batch_wide"]["median_ms"], row["batch_plain"]["median_ms"])
    row["ratio_merge_route_over_batch_wide"] = round(row["merge_route"]["median_ms"] / row["batch_wide"]["median_ms"], 3)
    row["ratio_plain_over_wide"] = round(row["batch_plain"]["median_ms"] / row["batch_wide"]["median_ms"], 4)
    row["fraction_of_binding_floor"] = round(max(hbm_ms, mac_ms) / best, 4)
    return row

R_MOD = ((1 << 256) - int.from_bytes(MONT_ONE.tobytes(), "little")) // 3                     # 2^256 = 3 r + (2^256 mod r): r is just above 2^254
R_INV = pow(1 << 256, -1, R_MOD)
ARMS = {"opt_00": (0, 0), "opt_10": (1, 0), "opt_01": (0, 1), "opt_11": (1, 1)}

def fr_mul(a, b):
    """the product of two stored (Montgomery) elements, on the host"""
    x = int.from_bytes(np.ascontiguousarray(a, np.uint64).tobytes(), "little") * int.from_bytes(np.ascontiguousarray(b, np.uint64).tobytes(), "little") * R_INV % R_MOD
    return np.frombuffer(x.to_bytes(32, "little"), np.uint64).copy()

def shared_points(lg, npoints, kind):
    zs = np.ascontiguousarray(rng.integers(0, 1 << 62, size=(npoints, 4), dtype=np.uint64))
    if kind != "random":                                              # z w^s: consecutive shifts for the pair, spread ones for the sixteen
        w = root_of_unity(lg); step = w if kind == "pair" else fr_mul(fr_mul(w, w), w)
        for p in range(1, npoints): zs[p] = fr_mul(zs[p - 1], step)
    return zs

def shared_row(lg, ncols, npoints, kind):
    n = 1 << lg
    cols = [synth(0x1A64 + lg, c, n) for c in range(ncols)]; ptrs = [t.data_ptr() for t in cols]; zs = shared_points(lg, npoints, kind)
    out = {v: torch.zeros((npoints * ncols, 4), dtype=torch.int64, device=dev) for v in ARMS}
    times = {v: [] for v in ARMS}
    for rep in range(REPS + 1):                                       # repetition 0 is the warm-up of this shape
        for v, (inv, cos) in ARMS.items():
            ctx.set_option("lagrange_shared_inverse", inv); ctx.set_option("lagrange_share_cosets", cos)
            t = timed(lambda: ctx.lagrange_eval_on_h_batch_dev(ptrs, n, zs, out[v].data_ptr()))
            if rep: times[v].append(t)
        if not rep:
            ctx.sync(); assert all(torch.equal(out[v], out["opt_00"]) for v in ARMS), (lg, ncols, npoints, kind)
    ctx.set_option("lagrange_shared_inverse", -1); ctx.set_option("lagrange_share_cosets", -1)
    W = -(-(-(-n // 8)) // 256)
    products = npoints * n * (5.75 + ncols) + npoints * W * 381
    hbm_ms = 1e3 * ncols * n * 32 / HBM_BPS; mac_ms = 1e3 * products * 96 / mac_rate.value
    row = {"tool": "lagrange_eval_timing", "call": "batch", "log_n": lg, "ncols": ncols, "npoints": npoints, "points": kind, "reps": REPS, "outputs_byte_equal": True,
           "lane_macs_per_s": mac_rate.value, "hbm_floor_ms": round(hbm_ms, 5), "mac_floor_ms": round(mac_ms, 5)}
    for v in ARMS: row[v] = stats(times[v])
    spread = lambda v: row[v]["max_ms"] - row[v]["min_ms"]
    row["over_opt_00"] = {v: round(row[v]["median_ms"] / row["opt_00"]["median_ms"], 4) for v in ARMS if v != "opt_00"}
    row["slower_beyond_spread"] = [v for v in ARMS if v != "opt_00" and row[v]["median_ms"] - row["opt_00"]["median_ms"] > max(spread(v), spread("opt_00"))]
    row["fraction_of_mac_floor"] = {v: round(mac_ms / row[v]["median_ms"], 4) for v in ARMS}
    return row

if len(sys.argv) > 3 and sys.argv[3] == "shared":
    rows = []
    for lg, ncols, npoints, kind in [s + ("random",) for s in SHAPES] + [(20, 4, 2, "pair"), (16, 64, 2, "pair"), (20, 4, 16, "shifts")]:
        rows.append(shared_row(lg, ncols, npoints, kind)); print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    open(sys.argv[2], "w").write("".join(json.dumps(r) + "\n" for r in rows))
    ctx.close(); sys.exit(0)

out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lagrange_eval_timing.jsonl")
rows = []
for lg, ncols, npoints in SHAPES:
    rows.append(shape_row(lg, ncols, npoints)); print(json.dumps(rows[-1]), flush=True)
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write("".join(json.dumps(r) + "\n" for r in rows))
ctx.close()
