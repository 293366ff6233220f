"""tools/sumcheck_batch_timing.py — stark_sumcheck_prove_{plain,mf}_batch_dev against a loop of B single stark_sumcheck_prove_*_dev calls, for
B = 1, 8, 64, 256 distinct witnesses at the reference bench's sizes (plain k = 12, 14, 16; mf k = 12, 14 with q = 2).  Witnesses are synthetic
columns made on the GPU, with two tree labels mixed.  Wall time on the host around each call (every call ends in a synchronisation), after one
warm-up of each path: the batch is the median of 3 runs; the single loop is one run, alternated with the batch runs.  At every size all B
batch proofs are compared with the single proofs.  The B = 1 row also times batch (B = 1) against one single prove alternately, 10 pairs, medians and spreads.
Writes profiles/sumcheck_batch_timing.jsonl (or the path given as the first argument).  Not product code."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from stark_mlwe_amd.api import Context

Q = 2
SIZES = [("plain", 12), ("plain", 14), ("plain", 16), ("mf", 12), ("mf", 14)]
BS = (1, 8, 64, 256)
ctx = Context(0); lib = ctx.lib


def wall_ms(fn):
    t0 = time.perf_counter(); v = fn(); return (time.perf_counter() - t0) * 1e3, v


def single(mf, k, label, p):
    h = C.c_void_p()
    if mf:
        ctx._chk(lib.stark_sumcheck_prove_mf_dev(ctx.h, C.c_void_p(p), k, label, Q, C.byref(h)))
    else:
        ctx._chk(lib.stark_sumcheck_prove_plain_dev(ctx.h, C.c_void_p(p), k, label, C.byref(h)))
    return ctx._proof_out(h)[0]


rows = []
for variant, k in SIZES:
    mf = variant == "mf"; n = 1 << k
    wit = torch.empty((max(BS), n, 4), dtype=torch.int64, device="cuda")
    for b in range(max(BS)):
        ctx._chk(lib.stark_synth_column_dev(ctx.h, 0x5C0B0000 + 64 * k + b, b % 4, 0, n, C.c_void_p(wit[b].data_ptr())))
    torch.cuda.synchronize()
    ptrs = [wit[b].data_ptr() for b in range(max(BS))]
    labels = [2025 if b % 2 == 0 else 7 for b in range(max(BS))]
    batch = (lambda B: ctx.prove_mf_batch_dev(k, labels[:B], Q, ptrs[:B])) if mf else (lambda B: ctx.prove_plain_batch_dev(k, labels[:B], ptrs[:B]))
    batch(1); single(mf, k, labels[0], ptrs[0])                                   # warm constants and the pool
    for B in BS:
        batch(B)
        runs, loop_ms, ones = [], None, None
        for rep in range(3):
            runs.append(wall_ms(lambda: batch(B)))
            if rep == 0:
                loop_ms, ones = wall_ms(lambda: [single(mf, k, labels[b], ptrs[b]) for b in range(B)])
        batch_ms = statistics.median(ms for ms, _ in runs)
        equal = all(v == ones for _, v in runs)
        row = {"variant": variant, "k": k, "q": Q if mf else None, "B": B, "batch_ms": round(batch_ms, 3), "batch_ms_per_proof": round(batch_ms / B, 3),
               "single_loop_ms": round(loop_ms, 3), "single_ms_per_proof": round(loop_ms / B, 3), "speedup": round(loop_ms / batch_ms, 2), "outputs_equal": bool(equal)}
        if B == 1:
            pairs = [(wall_ms(lambda: batch(1))[0], wall_ms(lambda: single(mf, k, labels[0], ptrs[0]))[0]) for _ in range(10)]
            bm, sm = [p[0] for p in pairs], [p[1] for p in pairs]
            row.update({"b1_batch_median_ms": round(statistics.median(bm), 3), "b1_batch_min_max_ms": [round(min(bm), 3), round(max(bm), 3)],
                        "b1_single_median_ms": round(statistics.median(sm), 3), "b1_single_min_max_ms": [round(min(sm), 3), round(max(sm), 3)]})
        rows.append(row); print(json.dumps(row), flush=True)
    del wit
with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sumcheck_batch_timing.jsonl"), "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
ctx.close()
