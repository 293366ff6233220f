"""tools/sumcheck_mixed_timing.py — stark_sumcheck_prove_{plain,mf}_mixed_batch_dev against what it replaces, wall time per call (host clock around
calls that end synchronised: every prove downloads its proofs), medians and min / max over ten alternating repetitions in one process after a warm
call of each side whose outputs must be byte-equal.  Each sweep runs as ONE mixed call:
  plain  k = 10..16, one witness per size, and eight per size
  mf     k = 10..14, q = 2, one witness per size, and eight per size
against (1) the same witnesses through the same-size entry points, one stark_sumcheck_prove_*_batch_dev call per distinct k, and (2) the
witnesses of the largest k alone (one same-size call: the floor of the mixed call, whose steps are that call's rounds).
Writes profiles/sumcheck_mixed_timing.jsonl (or the path given as the first argument).  `--quick`: three repetitions.  Not product code."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from stark_mlwe_amd.api import Context

args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else os.path.join(ROOT, "profiles", "sumcheck_mixed_timing.jsonl")
REPS = 3 if "--quick" in sys.argv else 10
Q = 2
ctx = Context(0); lib = ctx.lib


def alternate(fs):
    """(median, min, max) in ms of every function of fs over REPS rounds that run them one after another (alternating), after one warm call of each"""
    ts = [[] for _ in fs]
    for f in fs:
        f()
    for _ in range(REPS):
        for i, f in enumerate(fs):
            t0 = time.perf_counter(); f(); ts[i].append(1e3 * (time.perf_counter() - t0))
    return [(round(statistics.median(t), 3), round(min(t), 3), round(max(t), 3)) for t in ts]


rows = []
for variant, k_lo, k_hi in (("plain", 10, 16), ("mf", 10, 14)):
    mf = variant == "mf"
    for per in (1, 8):
        ks = [k for k in range(k_lo, k_hi + 1) for _ in range(per)]; B = len(ks)
        wit = [torch.empty((1 << k, 4), dtype=torch.int64, device="cuda") for k in ks]
        for b, k in enumerate(ks):
            ctx._chk(lib.stark_synth_column_dev(ctx.h, 0x5C3D0000 + 64 * k + b, b % 4, 0, 1 << k, C.c_void_p(wit[b].data_ptr())))
        torch.cuda.synchronize()
        ptrs = [w.data_ptr() for w in wit]; labels = [2025 if b % 2 == 0 else 7 for b in range(B)]
        groups = {k: [b for b in range(B) if ks[b] == k] for k in sorted(set(ks))}

        def same_size(k, bs):
            return ctx.prove_mf_batch_dev(k, [labels[b] for b in bs], Q, [ptrs[b] for b in bs]) if mf else ctx.prove_plain_batch_dev(k, [labels[b] for b in bs], [ptrs[b] for b in bs])

        def mixed():
            return ctx.prove_mf_mixed_batch_dev(ks, labels, Q, ptrs) if mf else ctx.prove_plain_mixed_batch_dev(ks, labels, ptrs)

        def grouped():
            out = [None] * B
            for k, bs in groups.items():
                for b, p in zip(bs, same_size(k, bs)):
                    out[b] = p
            return out

        def largest():
            return same_size(k_hi, groups[k_hi])
        equal = mixed() == grouped()
        (mm, mlo, mhi), (gm, glo, ghi), (lm, llo, lhi) = alternate([mixed, grouped, largest])
        rows.append({"variant": variant, "q": Q if mf else None, "k": [k_lo, k_hi], "witnesses_per_k": per, "B": B, "reps": REPS, "mixed_ms": mm, "mixed_min_max_ms": [mlo, mhi],
                     "grouped_calls": len(groups), "grouped_ms": gm, "grouped_min_max_ms": [glo, ghi], "largest_k_alone_ms": lm, "largest_min_max_ms": [llo, lhi],
                     "grouped_over_mixed": round(gm / mm, 2), "mixed_over_largest": round(mm / lm, 2), "outputs_equal": bool(equal)})
        print(json.dumps(rows[-1]), flush=True)
        del wit
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
ctx.close()
