"""tools/verify_batch_timing.py — stark_deep_fri_verify_batch against a loop of stark_deep_fri_verify calls, for B = 1, 4, 16, 64, 256 proofs at
the reference bench's paper shape ([16,16,8], r = 32) and at uni128x2 ([128,128], r = 32), k = 16.  Eight distinct proofs per shape (made on the
GPU from synthetic f0s), repeated to fill the batch.  Wall time on the host around each call (both calls end in a synchronisation): the
batch is the median of 5 runs after one warm-up, the loop one run after one warm-up.  Writes profiles/verify_batch_timing.jsonl (or the path given as the first argument).  Not product code."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from stark_mlwe_amd.api import Context, DeepFriParams

SEED_Z, K, R, DISTINCT = 0xDEEFBAAD, 16, 32, 8
SHAPES = [("paper", [16, 16, 8]), ("uni128x2", [128, 128])]
ctx = Context(0); lib = ctx.lib


def make_proofs(sched):
    n0 = 1 << K; sch = np.ascontiguousarray(sched, dtype=np.uint64); out = []
    f0 = torch.empty((n0, 4), dtype=torch.int64, device="cuda")
    for i in range(DISTINCT):
        ctx._chk(lib.stark_synth_column_dev(ctx.h, 0x5EED0100 + i, 5, 0, n0, C.c_void_p(f0.data_ptr())))
        h = C.c_void_p()
        ctx._chk(lib.stark_deep_fri_prove_dev(ctx.h, None, None, None, None, C.c_void_p(f0.data_ptr()), n0, sch.ctypes.data_as(C.c_void_p), len(sched), R, SEED_Z, C.byref(h)))
        out.append(ctx._proof_out(h)[0])
    return out


def wall_ms(fn):
    t0 = time.perf_counter(); v = fn(); return (time.perf_counter() - t0) * 1e3, v


rows = []
for label, sched in SHAPES:
    prm = DeepFriParams(sched, R, SEED_Z); distinct = make_proofs(sched)
    for B in (1, 4, 16, 64, 256):
        proofs = [distinct[i % DISTINCT] for i in range(B)]
        ctx.deep_fri_verify_batch(prm, proofs)
        runs = [wall_ms(lambda: ctx.deep_fri_verify_batch(prm, proofs)) for _ in range(5)]
        batch_ms = statistics.median(ms for ms, _ in runs)
        ok_batch = all(all(v) for _, v in runs)
        ctx.deep_fri_verify(prm, proofs[0])
        loop_ms, single = wall_ms(lambda: [ctx.deep_fri_verify(prm, p) for p in proofs])
        row = {"label": label, "k": K, "schedule": sched, "r": R, "B": B, "batch_ms": round(batch_ms, 3), "batch_ms_per_proof": round(batch_ms / B, 3),
               "single_loop_ms": round(loop_ms, 3), "single_ms_per_proof": round(loop_ms / B, 3), "speedup": round(loop_ms / batch_ms, 2),
               "all_accepted": bool(ok_batch and all(single))}
        rows.append(row); print(json.dumps(row), flush=True)
with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "verify_batch_timing.jsonl"), "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
ctx.close()
