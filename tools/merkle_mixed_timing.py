"""tools/merkle_mixed_timing.py — what finding the segment costs: the SAME trees (arity 16, B trees of 2^log_n leaves, equal shapes) through
stark_merkle_build_mixed_batch_dev (DsRaggedStream: a binary search over the segment table per element read) and through
stark_merkle_build_batch_dev (DsBatchStream: a division), each followed by stark_merkle_roots_batch, in one process.  A second row builds a mixed
set (2^8 .. 2^12 leaves, B trees) in one mixed call against one same-shape call per distinct length.
Outputs are compared byte for byte first.  Then the two sides run as alternating pairs (ten pairs after a warm-up pair), wall time on the host
around each side (every side ends in a synchronisation), medians and the min / max of each side (the run-to-run spread).
Writes profiles/merkle_mixed_timing.jsonl (or the path given as the first argument).  Not product code."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from stark_mlwe_amd.api import Context

ARITY, PAIRS = 16, 10
ctx = Context(0); lib = ctx.lib; p17 = ctx.poseidon_params_for_arity(ARITY)


def wall_ms(fn):
    t0 = time.perf_counter(); v = fn(); return (time.perf_counter() - t0) * 1e3, v


def pairs(a, b):
    a(); b()
    am, bm = [], []
    for _ in range(PAIRS):
        am.append(wall_ms(a)[0]); bm.append(wall_ms(b)[0])
    return statistics.median(am), statistics.median(bm), [round(min(am), 3), round(max(am), 3)], [round(min(bm), 3), round(max(bm), 3)]


def columns(seed, ns):
    import ctypes as C
    cols = [torch.empty((n, 4), dtype=torch.int64, device="cuda") for n in ns]
    for b, n in enumerate(ns):
        ctx._chk(lib.stark_synth_column_dev(ctx.h, seed, b, 0, n, C.c_void_p(cols[b].data_ptr())))
    torch.cuda.synchronize()
    return cols


def roots_of(trees):
    roots = ctx.merkle_roots_batch(trees)
    for t in trees:
        t.free()
    return roots


rows = []
for lg, B in ((12, 64), (12, 1), (8, 64)):
    n = 1 << lg; cols = columns(0x31D0000 + lg, [n] * B)
    ptrs = [c.data_ptr() for c in cols]; labels = [1000 + b for b in range(B)]
    mixed = lambda: roots_of(ctx.merkle_build_mixed_batch_dev(ptrs, [n] * B, ARITY, labels, p17))
    same = lambda: roots_of(ctx.merkle_build_batch_dev(ptrs, n, ARITY, labels, p17))
    equal = bool((mixed() == same()).all())
    mm, sm, mmm, smm = pairs(mixed, same)
    rows.append({"op": "equal shapes, build+roots", "log_n": lg, "B": B, "mixed_ms": round(mm, 3), "same_shape_ms": round(sm, 3), "mixed_min_max_ms": mmm, "same_shape_min_max_ms": smm,
                 "mixed_minus_same_ms": round(mm - sm, 3), "outputs_equal": equal})
    print(json.dumps(rows[-1]), flush=True)

for per in (1, 8):                                                          # 2^8 .. 2^12 leaves, `per` trees each: one mixed call against five same-shape calls
    logs = [lg for lg in range(8, 13) for _ in range(per)]; ns = [1 << lg for lg in logs]; B = len(ns)
    cols = columns(0x31E0000 + per, ns); ptrs = [c.data_ptr() for c in cols]; labels = [2000 + b for b in range(B)]
    groups = {lg: [b for b in range(B) if logs[b] == lg] for lg in sorted(set(logs))}
    mixed = lambda: roots_of(ctx.merkle_build_mixed_batch_dev(ptrs, ns, ARITY, labels, p17))

    def grouped():
        out = np.zeros((B, 4), np.uint64)
        for lg, bs in groups.items():
            out[bs] = roots_of(ctx.merkle_build_batch_dev([ptrs[b] for b in bs], 1 << lg, ARITY, [labels[b] for b in bs], p17))
        return out
    largest = lambda: roots_of(ctx.merkle_build_batch_dev([ptrs[b] for b in groups[12]], 1 << 12, ARITY, [labels[b] for b in groups[12]], p17))
    equal = bool((mixed() == grouped()).all())
    mm, gm, mmm, gmm = pairs(mixed, grouped)
    _, lm, _, lmm = pairs(mixed, largest)
    rows.append({"op": "2^8..2^12 leaves, build+roots", "trees_per_size": per, "B": B, "mixed_ms": round(mm, 3), "grouped_calls_ms": round(gm, 3), "largest_group_alone_ms": round(lm, 3),
                 "mixed_min_max_ms": mmm, "grouped_min_max_ms": gmm, "largest_min_max_ms": lmm, "outputs_equal": equal})
    print(json.dumps(rows[-1]), flush=True)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "merkle_mixed_timing.jsonl")
with open(path, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
ctx.close()
