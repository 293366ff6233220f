"""tools/sumcheck_verify_batch_timing.py — stark_sumcheck_verify_{plain,mf}_batch against a loop of B single stark_sumcheck_verify_* calls, for
B = 1, 4, 16, 64, 256 proofs at the reference bench's sizes (plain k = 12, 14, 16; mf k = 12, 14 with q = 2).  The proofs are made on the GPU from
eight synthetic witnesses under two tree labels, repeated to fill the batch, with one tampered copy in sixteen.  Wall time on the host around each
call (every call ends in a synchronisation), after a warm-up of each path: batch and single loop run as alternating pairs, ten pairs, medians.
Every batch answer is compared with the single answers.  Also recorded: the batch under the option "sponge_one_wave" (the transcripts one wave per
instance whatever their number; median of five), and the host planning time of the B = 256 batch (the planner alone, through the host-check build of
the same header, g++ -O2) over the call's time: above 1 where that build plans slower than the product's whole call.  Writes profiles/sumcheck_verify_batch_timing.jsonl (or the path given as the first argument).  Not product code."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from stark_mlwe_amd.api import Context

Q = 2
SIZES = [("plain", 12), ("plain", 14), ("plain", 16), ("mf", 12), ("mf", 14)]
BS = (1, 4, 16, 64, 256)
PAIRS = 10
ctx = Context(0); lib = ctx.lib
one_wave = Context(0); one_wave.set_option("sponge_one_wave", 1)
hc = C.CDLL(os.path.join(ROOT, "stark_mlwe_amd", "libstark_mlwe_hostcheck.so")); hc.hc_sumcheck_verify_batch_steps.restype = C.c_size_t


def wall_ms(fn):
    t0 = time.perf_counter(); v = fn(); return (time.perf_counter() - t0) * 1e3, v


def plan_ms(mf, proofs, labels):
    n = len(proofs); bufs = [(C.c_uint8 * len(p)).from_buffer_copy(p) for p in proofs]
    ptrs = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs]); lens = (C.c_size_t * n)(*[len(p) for p in proofs])
    lab = np.ascontiguousarray(labels, dtype=np.uint64); kind, count = (C.c_int32 * 64)(), (C.c_size_t * 64)()
    f = lambda: hc.hc_sumcheck_verify_batch_steps(mf, C.c_size_t(n), ptrs, lens, lab.ctypes.data_as(C.c_void_p), kind, count, C.c_size_t(64))
    f()
    return statistics.median(wall_ms(f)[0] for _ in range(5))


rows = []
for variant, k in SIZES:
    mf = variant == "mf"; n = 1 << k
    wit = torch.empty((8, n, 4), dtype=torch.int64, device="cuda")
    for b in range(8):
        ctx._chk(lib.stark_synth_column_dev(ctx.h, 0x5C0B1000 + 64 * k + b, b % 4, 0, n, C.c_void_p(wit[b].data_ptr())))
    torch.cuda.synchronize()
    lab8 = [2025 if b % 2 == 0 else 7 for b in range(8)]; ptr8 = [wit[b].data_ptr() for b in range(8)]
    honest = ctx.prove_mf_batch_dev(k, lab8, Q, ptr8) if mf else ctx.prove_plain_batch_dev(k, lab8, ptr8)
    del wit
    proofs, labels = [], []
    for b in range(max(BS)):
        p = honest[b % 8]
        if b % 16 == 5:
            bad = bytearray(p); bad[len(p) // 2 + b] ^= 4; p = bytes(bad)
        proofs.append(p); labels.append(lab8[b % 8])
    single = (lambda b: ctx.verify_mf(k, labels[b], Q, proofs[b])) if mf else (lambda b: ctx.verify_plain(k, labels[b], proofs[b]))
    batch_on = lambda c, B: c.verify_mf_batch(k, labels[:B], Q, proofs[:B]) if mf else c.verify_plain_batch(k, None, proofs[:B])
    batch_on(ctx, 1); batch_on(one_wave, 1); single(0)                                  # warm constants and the pool
    for B in BS:
        batch_on(ctx, B); batch_on(one_wave, B)
        bm, sm, equal = [], [], True
        for _ in range(PAIRS):
            tb, vb = wall_ms(lambda: batch_on(ctx, B)); ts, vs = wall_ms(lambda: [single(b) for b in range(B)])
            bm.append(tb); sm.append(ts); equal = equal and vb == vs
        ow = statistics.median(wall_ms(lambda: batch_on(one_wave, B))[0] for _ in range(5))
        batch_ms, loop_ms = statistics.median(bm), statistics.median(sm)
        row = {"variant": variant, "k": k, "q": Q if mf else None, "B": B, "proof_bytes": len(honest[0]), "accepted": sum(batch_on(ctx, B)),
               "batch_ms": round(batch_ms, 3), "batch_min_max_ms": [round(min(bm), 3), round(max(bm), 3)], "batch_ms_per_proof": round(batch_ms / B, 4),
               "single_loop_ms": round(loop_ms, 3), "single_min_max_ms": [round(min(sm), 3), round(max(sm), 3)], "single_ms_per_proof": round(loop_ms / B, 4),
               "speedup": round(loop_ms / batch_ms, 2), "batch_one_wave_ms": round(ow, 3), "answers_equal": bool(equal)}
        if B == max(BS):
            pm = plan_ms(1 if mf else 0, proofs[:B], labels[:B])
            row.update({"host_plan_ms": round(pm, 3), "host_plan_share": round(pm / batch_ms, 3)})
        rows.append(row); print(json.dumps(row), flush=True)
with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sumcheck_verify_batch_timing.jsonl"), "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
one_wave.close(); ctx.close()
