"""tools/prove_batch_timing.py — the side-by-side tail of the batched DEEP-FRI provers against what it replaces, wall time per call, medians over
ten alternating pairs in one process (pool and parameter caches warmed first), every compared output checked byte-equal:
  (a) stark_deep_fri_prove_f0_batch_dev against B single stark_deep_fri_prove_dev(f0) calls, k = 11, 12, 14, 16 and B = 1, 4, 16, 64, 256 within memory;
  (c) option prove_batch_max_rows from 2^18 to 2^24 at k = 12 and k = 16, f0 batch at the largest B of the grid (so that the small settings cut it into several passes).
(Part (b) compared the side-by-side tail of stark_deep_fri_prove_batch_dev with the worker-context tail it replaced; that tail is gone, and its rows
stay in profiles/prove_batch_timing.jsonl as the record.)  Writes profiles/prove_batch_timing_ac.jsonl (or the path given as the first argument).  `--quick` as a further argument keeps the grid to what fits in a
couple of minutes (fewer pairs, B <= 64).  Not product code."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from stark_mlwe_amd.api import Context, DeepFriParams

args = [a for a in sys.argv[1:] if not a.startswith("--")]
QUICK = "--quick" in sys.argv
OUT = args[0] if args else os.path.join(ROOT, "profiles", "prove_batch_timing_ac.jsonl")
PAIRS = 3 if QUICK else 10
MAX_ROWS_TOTAL = 1 << 22 if QUICK else 1 << 24          # B * n0 kept within this (memory and time)
SEED_Z = 0xDEEFBAAD
vp = C.c_void_p
ctx = Context(0)


def shape(k):
    return ([16, 16, 8], 32) if k >= 12 else ([16, 8], 8)


def synth(k, B, seed):
    n0 = 1 << k; keep = []
    for p in range(B):
        cols = [torch.empty((n0, 4), dtype=torch.int64, device="cuda") for _ in range(4)]
        for c in range(4):
            ctx._chk(ctx.lib.stark_synth_column_dev(ctx.h, seed + p, c, 0, n0, vp(cols[c].data_ptr())))
        keep.append(cols)
    torch.cuda.synchronize()
    return keep


def single_f0(ptr, n0, sched, r):
    sch = np.ascontiguousarray(sched, dtype=np.uint64); h = vp()
    ctx._chk(ctx.lib.stark_deep_fri_prove_dev(ctx.h, None, None, None, None, vp(ptr), n0, sch.ctypes.data_as(vp), len(sched), r, SEED_Z, C.byref(h)))
    return ctx._proof_out(h)[0]


def alternate(f, g):
    """medians (ms) of f and g over PAIRS alternating pairs, after one warm call of each whose outputs must be equal"""
    assert f() == g()
    tf, tg = [], []
    for _ in range(PAIRS):
        t0 = time.perf_counter(); f(); tf.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); g(); tg.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(tf), 1e3 * statistics.median(tg)


rows = []
for k in (11, 12, 14, 16):
    sched, r = shape(k); n0 = 1 << k; prm = DeepFriParams(sched, r, SEED_Z)
    Bs = [B for B in (1, 4, 16, 64, 256) if B * n0 <= MAX_ROWS_TOTAL and (not QUICK or B <= 64)]
    keep = synth(k, max(Bs), 0x7B000000 + (k << 12))
    f0s = [cols[0].data_ptr() for cols in keep]          # any resident vector serves as an f0
    for B in Bs:
        b_ms, s_ms = alternate(lambda: [g[0] for g in ctx.deep_fri_prove_f0_batch_dev(f0s[:B], n0, prm)], lambda: [single_f0(p, n0, sched, r) for p in f0s[:B]])
        rows.append({"what": "f0_batch_vs_singles", "log_n0": k, "batch": B, "batch_ms": b_ms, "singles_ms": s_ms, "speedup": s_ms / b_ms})
        print(rows[-1], flush=True)

    if k in (12, 16):
        B = max(Bs)
        want = [g[0] for g in ctx.deep_fri_prove_f0_batch_dev(f0s[:B], n0, prm)]
        for lg in range(18, 25):
            ctx.set_option("prove_batch_max_rows", 1 << lg)
            try:
                f = lambda: [g[0] for g in ctx.deep_fri_prove_f0_batch_dev(f0s[:B], n0, prm)]
                assert f() == want
                ts = []
                for _ in range(PAIRS):
                    t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
            finally:
                ctx.set_option("prove_batch_max_rows", 1 << 22)
            rows.append({"what": "max_rows_sweep", "log_n0": k, "batch": B, "log_max_rows": lg, "traces_per_pass": max(1, (1 << lg) // n0), "ms": 1e3 * statistics.median(ts)})
            print(rows[-1], flush=True)
    del keep
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
ctx.close()
