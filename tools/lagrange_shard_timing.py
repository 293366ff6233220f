"""tools/lagrange_shard_timing.py — the column groups of k_lagrange_partials and the sharded lagrange_eval_on_h, by the method of lagrange_eval_timing.py.

    python tools/lagrange_shard_timing.py LIB [OUT.jsonl]     (default profiles/lagrange_shard_timing.jsonl)

Every shape is warmed up first; then REPS repetitions of its variants, alternated in one process, each between stark_timer_start / stop (HIP events);
medians with the spread (min, max).

(a) kind "col_groups": stark_lagrange_eval_on_h_batch_dev under "lagrange_col_groups" = 1 (one_a), -1 (auto) and 1 again (one_b), for the four shapes
    of DESIGN §4.5a and the shard-like shapes (n, C, P) = (2^17, 64, 2), (2^17, 4, 2), (2^16, 64, 2).  one_a and one_b are the same launch: the
    relative difference of their medians is the spread of the shape (spread_one_vs_one), and the largest over the shapes the spread of the session
    (the "rule" line), the margin within which auto counts as no slower (auto_over_one = median(auto) / median(one_a and one_b pooled)).  Where
    the rule picks one group (`groups` = 1, recomputed here from the constants of csrc/lagrange_dev.hpp) auto IS the launch of one_a and one_b —
    the same kernel, grid and arguments — so its distance from them is a third sample of the spread (spread_identical_launches) and cannot be a
    loss; a shape can lose only where groups > 1.  The results of the variants are checked equal first.
    kind "col_groups_sweep", informational: (2^17, 64, 2) under "lagrange_col_groups" = 1, 2, 4, 8, alternated.
(b) kind "sharded", informational: n = 2^20, C = 4, P = 2: the single batch call, stark_diag_lagrange_eval_sharded_emulated_dev with W = 8 (eight
    virtual ranks serialised on one GPU, the header synchronisation included) and the eight stark_lagrange_eval_shard_dev calls alone.  W > 1 over
    real links is not measured by this tool.
Each line carries the floors of lagrange_eval_timing.py for one group: hbm_floor_ms = C n 32 bytes over 6.29 TB/s; mac_floor_ms = (P n (5.75 + C) +
P W 381) field products x 96 MACs over stark_diag_mac_rate read in the same run; with G column groups the weights are computed G times:
mac_floor_groups_ms = (P n (5.75 G + C) + P W G 381) products.

    python tools/lagrange_shard_timing.py LIB OUT.jsonl shared     (appends to OUT: profiles/lagrange_shared_timing.jsonl)

measures the options "lagrange_shared_inverse" and "lagrange_share_cosets" on the shard-like shapes (2^17, 4, 2) and (2^17, 64, 2) instead: the arms
opt_00, opt_10, opt_01, opt_11 (shared inverse, cosets), alternated, results checked byte-equal first, of the batch call on 2^17 rows (call "batch") and
of stark_lagrange_eval_shard_dev on the rows [2^17, 2^18) of a 2^20-point domain (call "shard": the block form ignores the cosets).  The points are
the pair (z, z w) of the call's own domain.  Lines as in lagrange_eval_timing.py's shared mode."""
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
TABLE_SHAPES = ((20, 4, 1), (20, 4, 2), (16, 64, 2), (23, 1, 1))
SHARD_SHAPES = ((17, 64, 2), (17, 4, 2), (16, 64, 2))
K, THREADS, TARGET_WG, GROUP_TARGET_WG, MIN_GROUP_COLS = 8, 256, 1024, 512, 8                     # csrc/lagrange_dev.hpp

def synth(seed, col, n):
    t = torch.empty((n, 4), dtype=torch.int64, device=dev)
    ctx._chk(lib.stark_synth_column_dev(ctx.h, seed, col, 0, n, C.c_void_p(t.data_ptr()))); return t

def timed(fn):
    ms = C.c_float(); ctx._chk(lib.stark_timer_start(ctx.h)); fn(); ctx._chk(lib.stark_timer_stop_ms(ctx.h, C.byref(ms))); return ms.value

def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5)}

def workgroups(n):
    return -(-(-(-n // K)) // THREADS)

def auto_groups(n, ncols, npoints):
    grid = workgroups(n); pg = min(npoints, 65535, max(-(-TARGET_WG // grid), 1)); g = 1
    while ncols // (g + 1) >= MIN_GROUP_COLS and grid * pg * g < GROUP_TARGET_WG: g += 1
    per = -(-ncols // g); return -(-ncols // per)

mac_rate = C.c_double(); ctx._chk(lib.stark_diag_mac_rate(ctx.h, C.byref(mac_rate)))

def floors(n, ncols, npoints, groups):
    W = workgroups(n)
    mac = lambda g: 1e3 * (npoints * n * (5.75 * g + ncols) + npoints * W * g * 381) * 96 / mac_rate.value
    return {"lane_macs_per_s": mac_rate.value, "hbm_floor_ms": round(1e3 * ncols * n * 32 / HBM_BPS, 5), "mac_floor_ms": round(mac(1), 5), "mac_floor_groups_ms": round(mac(groups), 5)}

def points(npoints):
    return np.ascontiguousarray(rng.integers(0, 1 << 62, size=(npoints, 4), dtype=np.uint64))        # stored limbs below 2^254 < r: outside H

def run_variants(variants, check):
    times = {v: [] for v in variants}
    for rep in range(REPS + 1):                                       # repetition 0 is the warm-up of this shape
        for v, (opt, fn) in variants.items():
            ctx.set_option("lagrange_col_groups", opt)
            t = timed(fn)
            if rep: times[v].append(t)
        if not rep:
            ctx.sync(); check()
    ctx.set_option("lagrange_col_groups", -1)
    return times

def col_groups_row(lg, ncols, npoints, table):
    n = 1 << lg
    cols = [synth(0x1A64 + lg, c, n) for c in range(ncols)]; ptrs = [t.data_ptr() for t in cols]; zs = points(npoints)
    out = {v: torch.zeros((npoints * ncols, 4), dtype=torch.int64, device=dev) for v in ("one_a", "auto", "one_b")}
    def batch(o):
        return lambda: ctx.lagrange_eval_on_h_batch_dev(ptrs, n, zs, o.data_ptr())
    def check():
        assert torch.equal(out["one_a"], out["auto"]) and torch.equal(out["one_a"], out["one_b"]), (lg, ncols, npoints)
    times = run_variants({"one_a": (1, batch(out["one_a"])), "auto": (-1, batch(out["auto"])), "one_b": (1, batch(out["one_b"]))}, check)
    groups = auto_groups(n, ncols, npoints)
    row = {"kind": "col_groups", "log_n": lg, "ncols": ncols, "npoints": npoints, "reps": REPS, "design_table_shape": table, "groups": groups}
    row.update(floors(n, ncols, npoints, groups))
    for v in times: row[v] = stats(times[v])
    one = statistics.median(times["one_a"] + times["one_b"])
    row["spread_one_vs_one"] = round(abs(row["one_a"]["median_ms"] - row["one_b"]["median_ms"]) / one, 4)
    row["auto_over_one"] = round(row["auto"]["median_ms"] / one, 4)
    same = [row["one_a"]["median_ms"], row["one_b"]["median_ms"]] + ([row["auto"]["median_ms"]] if groups == 1 else [])
    row["spread_identical_launches"] = round((max(same) - min(same)) / one, 4)
    return row

def sweep_row(lg, ncols, npoints, settings):
    n = 1 << lg
    cols = [synth(0x1A64 + lg, c, n) for c in range(ncols)]; ptrs = [t.data_ptr() for t in cols]; zs = points(npoints)
    out = {g: torch.zeros((npoints * ncols, 4), dtype=torch.int64, device=dev) for g in settings}
    def check():
        assert all(torch.equal(out[g], out[settings[0]]) for g in settings), (lg, ncols, npoints)
    times = run_variants({"groups_%d" % g: (g, (lambda o: lambda: ctx.lagrange_eval_on_h_batch_dev(ptrs, n, zs, o.data_ptr()))(out[g])) for g in settings}, check)
    row = {"kind": "col_groups_sweep", "log_n": lg, "ncols": ncols, "npoints": npoints, "reps": REPS, "automatic_groups": auto_groups(n, ncols, npoints)}
    for v in times: row[v] = stats(times[v])
    return row

def sharded_row(lg, ncols, npoints, W):
    n = 1 << lg; nl = n // W
    cols = [synth(0x1A64 + lg, c, n) for c in range(ncols)]; ptrs = [t.data_ptr() for t in cols]; zs = points(npoints); total = npoints * ncols
    o_batch = torch.zeros((total, 4), dtype=torch.int64, device=dev); o_emu = torch.zeros((W * total, 4), dtype=torch.int64, device=dev)
    parts = torch.zeros((W * total, 4), dtype=torch.int64, device=dev); o_comb = torch.zeros((total, 4), dtype=torch.int64, device=dev)
    def shards():
        for q in range(W):
            ctx.lagrange_eval_shard_dev([p + 32 * q * nl for p in ptrs], nl, q * nl, n, zs, parts.data_ptr() + 32 * total * q)
    def shards_and_combine():
        shards(); ctx.lagrange_eval_from_partials_dev(W, parts.data_ptr(), ncols, n, zs, o_comb.data_ptr())
    def check():
        assert torch.equal(o_emu.reshape(W, total, 4), o_batch.expand(W, total, 4)) and torch.equal(o_comb, o_batch), (lg, ncols, npoints)
    times = run_variants({"batch": (-1, lambda: ctx.lagrange_eval_on_h_batch_dev(ptrs, n, zs, o_batch.data_ptr())),
                          "emulated_w8": (-1, lambda: ctx.diag_lagrange_eval_sharded_emulated(W, ptrs, n, zs, o_emu.data_ptr())),
                          "shard_calls_w8": (-1, shards), "shard_calls_and_combine_w8": (-1, shards_and_combine)}, check)
    row = {"kind": "sharded", "log_n": lg, "ncols": ncols, "npoints": npoints, "reps": REPS, "nranks": W, "note": "eight virtual ranks serialised on one GPU; W > 1 over real links is unmeasured"}
    row.update(floors(n, ncols, npoints, 1))
    for v in times: row[v] = stats(times[v])
    row["emulated_over_batch"] = round(row["emulated_w8"]["median_ms"] / row["batch"]["median_ms"], 3)
    row["shard_calls_over_batch"] = round(row["shard_calls_w8"]["median_ms"] / row["batch"]["median_ms"], 3)
    return row

MONT_ONE = np.array([0x5b2b3e9cfffffffd, 0x992c350be3420567, 0xffffffffffffffff, 0x3fffffffffffffff], np.uint64)    # 2^256 mod r (Pallas Fr), csrc/fr.hpp
R_MOD = ((1 << 256) - int.from_bytes(MONT_ONE.tobytes(), "little")) // 3                     # 2^256 = 3 r + (2^256 mod r): r is just above 2^254
R_INV = pow(1 << 256, -1, R_MOD)
ARMS = {"opt_00": (0, 0), "opt_10": (1, 0), "opt_01": (0, 1), "opt_11": (1, 1)}

def fr_mul(a, b):
    """the product of two stored (Montgomery) elements, on the host"""
    x = int.from_bytes(np.ascontiguousarray(a, np.uint64).tobytes(), "little") * int.from_bytes(np.ascontiguousarray(b, np.uint64).tobytes(), "little") * R_INV % R_MOD
    return np.frombuffer(x.to_bytes(32, "little"), np.uint64).copy()

def shared_row(lg, ncols, call):
    n = 1 << lg; lg_global = lg if call == "batch" else 20
    cols = [synth(0x1A64 + lg, c, n) for c in range(ncols)]; ptrs = [t.data_ptr() for t in cols]
    zs = points(2); zs[1] = fr_mul(zs[0], root_of_unity(lg_global))
    out = {v: torch.zeros((2 * ncols, 4), dtype=torch.int64, device=dev) for v in ARMS}
    def run(o):
        if call == "batch": return lambda: ctx.lagrange_eval_on_h_batch_dev(ptrs, n, zs, o.data_ptr())
        return lambda: ctx.lagrange_eval_shard_dev(ptrs, n, n, 1 << lg_global, zs, o.data_ptr())
    times = {v: [] for v in ARMS}
    for rep in range(REPS + 1):
        for v, (inv, cos) in ARMS.items():
            ctx.set_option("lagrange_shared_inverse", inv); ctx.set_option("lagrange_share_cosets", cos)
            t = timed(run(out[v]))
            if rep: times[v].append(t)
        if not rep:
            ctx.sync(); assert all(torch.equal(out[v], out["opt_00"]) for v in ARMS), (lg, ncols, call)
    ctx.set_option("lagrange_shared_inverse", -1); ctx.set_option("lagrange_share_cosets", -1)
    row = {"tool": "lagrange_shard_timing", "call": call, "log_n": lg, "log_n_global": lg_global, "ncols": ncols, "npoints": 2, "points": "pair", "reps": REPS, "outputs_byte_equal": True,
           "groups": auto_groups(n, ncols, 2)}
    row.update(floors(n, ncols, 2, row["groups"]))
    for v in ARMS: row[v] = stats(times[v])
    spread = lambda v: row[v]["max_ms"] - row[v]["min_ms"]
    row["over_opt_00"] = {v: round(row[v]["median_ms"] / row["opt_00"]["median_ms"], 4) for v in ARMS if v != "opt_00"}
    row["slower_beyond_spread"] = [v for v in ARMS if v != "opt_00" and row[v]["median_ms"] - row["opt_00"]["median_ms"] > max(spread(v), spread("opt_00"))]
    return row

if len(sys.argv) > 3 and sys.argv[3] == "shared":
    rows = []
    for lg, ncols in ((17, 4), (17, 64)):
        for call in ("batch", "shard"):
            rows.append(shared_row(lg, ncols, call)); print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    open(sys.argv[2], "a").write("".join(json.dumps(r) + "\n" for r in rows))
    ctx.close(); sys.exit(0)

out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lagrange_shard_timing.jsonl")
rows = []
for shapes, table in ((TABLE_SHAPES, True), (SHARD_SHAPES, False)):
    for lg, ncols, npoints in shapes:
        rows.append(col_groups_row(lg, ncols, npoints, table)); print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
rows.append(sweep_row(17, 64, 2, (1, 2, 4, 8))); print(json.dumps(rows[-1]), flush=True)
torch.cuda.empty_cache()
rows.append(sharded_row(20, 4, 2, 8)); print(json.dumps(rows[-1]), flush=True)
measured = [r for r in rows if r["kind"] == "col_groups"]
spread = max(r["spread_identical_launches"] for r in measured)
for r in measured: r["auto_slower_beyond_spread"] = bool(r["groups"] > 1 and r["auto_over_one"] > 1 + spread)
losers = [r for r in measured if r["design_table_shape"] and r["auto_slower_beyond_spread"]]
rows.append({"kind": "rule", "session_spread": spread, "table_shapes_where_auto_loses": [[r["log_n"], r["ncols"], r["npoints"]] for r in losers], "default_stays_automatic": not losers,
             "other_shapes_where_auto_loses": [[r["log_n"], r["ncols"], r["npoints"]] for r in measured if not r["design_table_shape"] and r["auto_slower_beyond_spread"]]})
print(json.dumps(rows[-1]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write("".join(json.dumps(r) + "\n" for r in rows))
ctx.close()
