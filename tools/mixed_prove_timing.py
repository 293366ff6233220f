"""tools/mixed_prove_timing.py — stark_deep_fri_prove_mixed_batch_dev against what it replaces, wall time per call (host clock around calls that
end synchronised: every prove downloads its proof), medians over ten alternating repetitions in one process after a warm call of each side
whose outputs must be byte-equal:
  (a) the sweep k = 11..16 (schedule [16,16,8], r = 32) as six stark_deep_fri_prove_dev calls against ONE mixed call, and one k = 16 prove
      alone (the floor of the mixed call: its longest chain); stage_ms of the mixed call's k = 16 and k = 11 proofs go into the line;
  (b) 64 traces of sizes drawn (seeded) from 2^8..2^14 in one mixed call against the same traces grouped by hand into one
      stark_deep_fri_prove_batch_dev call per size.
Writes profiles/mixed_prove_timing.jsonl (or the path given as the first argument).  `--quick`: three repetitions.
`--tail`: the second arm instead — the same two workloads through the mixed call under the context option "mixed_prove_tail" = 0 (groups of equal
shape, the reference of the session) against 1 (one ragged tail per schedule), alternating, outputs byte-equal; per arm the median, the minimum and
the maximum over the repetitions (the spread a difference has to exceed) and the stage times 0/1/2 of the largest and the smallest proof, plus the
k = 16 prove alone as the floor of the sweep.  Writes profiles/mixed_prove_tail_timing.jsonl.  Not product code."""
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from stark_mlwe_amd.api import Context, DeepFriParams

args = [a for a in sys.argv[1:] if not a.startswith("--")]
TAIL = "--tail" in sys.argv
OUT = args[0] if args else os.path.join(ROOT, "profiles", "mixed_prove_tail_timing.jsonl" if TAIL else "mixed_prove_timing.jsonl")
REPS = 3 if "--quick" in sys.argv else 10
SEED_Z = 0xDEEFBAAD
vp = C.c_void_p
ctx = Context(0)


def shape(k):
    return ([16, 16, 8], 32) if k >= 11 else ([16, 8], 8)


def synth(k, seed):
    n0 = 1 << k
    cols = [torch.empty((n0, 4), dtype=torch.int64, device="cuda") for _ in range(4)]
    for c in range(4):
        ctx._chk(ctx.lib.stark_synth_column_dev(ctx.h, seed, c, 0, n0, vp(cols[c].data_ptr())))
    return cols


def single(cols, k):
    sched, r = shape(k); sch = np.ascontiguousarray(sched, dtype=np.uint64); h = vp()
    ctx._chk(ctx.lib.stark_deep_fri_prove_dev(ctx.h, *[vp(c.data_ptr()) for c in cols], None, 1 << k, sch.ctypes.data_as(vp), len(sched), r, SEED_Z, C.byref(h)))
    return ctx._proof_out(h)[0]


def mixed(traces, ks):
    return ctx.deep_fri_prove_mixed_batch_dev([[c.data_ptr() for c in tr] for tr in traces], [(1 << k,) + shape(k) for k in ks], SEED_Z)


def alternate(fs):
    """medians (ms) of every function of fs over REPS rounds that run them one after another (alternating), after one warm call of each"""
    ts = [[] for _ in fs]
    for f in fs:
        f()
    for _ in range(REPS):
        for i, f in enumerate(fs):
            t0 = time.perf_counter(); f(); ts[i].append(time.perf_counter() - t0)
    return [1e3 * statistics.median(t) for t in ts]


def alternate_spread(fs):
    """(median, min, max) in ms of every function of fs over REPS alternating rounds, after one warm call of each"""
    ts = [[] for _ in fs]
    for f in fs:
        f()
    for _ in range(REPS):
        for i, f in enumerate(fs):
            t0 = time.perf_counter(); f(); ts[i].append(time.perf_counter() - t0)
    return [(1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)) for t in ts]


def with_tail(v, f):
    ctx.set_option("mixed_prove_tail", v)
    try:
        return f()
    finally:
        ctx.set_option("mixed_prove_tail", -1)


def tail_arm(what, tr, ks, extra=()):
    """option 0 against option 1 on one workload -> one row"""
    g0 = with_tail(0, lambda: mixed(tr, ks)); g1 = with_tail(1, lambda: mixed(tr, ks))
    assert [g[:2] for g in g0] == [g[:2] for g in g1], what                         # outputs byte-equal
    res = alternate_spread([lambda: with_tail(0, lambda: mixed(tr, ks)), lambda: with_tail(1, lambda: mixed(tr, ks))] + [f for _, f in extra])
    g0 = with_tail(0, lambda: mixed(tr, ks)); g1 = with_tail(1, lambda: mixed(tr, ks))
    big, small = ks.index(max(ks)), ks.index(min(ks))
    row = {"what": what, "reps": REPS, "traces": len(ks), "classes": len({tuple(shape(k)[0]) for k in ks}), "groups": len({k for k in ks})}
    for name, (med, lo, hi) in zip(["option0", "option1"] + [n for n, _ in extra], res):
        row[name + "_ms"] = med; row[name + "_min_ms"] = lo; row[name + "_max_ms"] = hi
    row["option0_over_option1"] = res[0][0] / res[1][0]
    row["option0_stage_ms_largest"] = g0[big][2]; row["option1_stage_ms_largest"] = g1[big][2]
    row["option0_stage_ms_smallest"] = g0[small][2]; row["option1_stage_ms_smallest"] = g1[small][2]
    # the tail of a call: commit and query stages summed over its passes (every proof of a pass carries the pass's times)
    for name, g in (("option0", g0), ("option1", g1)):
        passes = {(x[2][1], x[2][2]) for x in g}
        row[name + "_tail_ms_sum_over_passes"] = sum(a + b for a, b in passes); row[name + "_passes"] = len(passes)
    print(row, flush=True)
    return row


if TAIL:
    rows = []
    ks = list(range(11, 17))
    tr = [synth(k, 0x7C000000 + k) for k in ks]
    torch.cuda.synchronize()
    rows.append(tail_arm("sweep_k11_k16", tr, ks, extra=[("k16_alone", lambda: single(tr[-1], 16))]))
    del tr
    rng = random.Random(0x51235)
    ks = [rng.randint(8, 14) for _ in range(64)]
    tr = [synth(k, 0x7D000000 + 64 * k + i) for i, k in enumerate(ks)]
    torch.cuda.synchronize()
    rows.append(tail_arm("batch64_k8_k14", tr, ks))
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    ctx.close()
    sys.exit(0)

rows = []
# (a) the reference's sweep
ks = list(range(11, 17))
tr = [synth(k, 0x7C000000 + k) for k in ks]
torch.cuda.synchronize()
got = mixed(tr, ks)
assert [g[0] for g in got] == [single(t, k) for t, k in zip(tr, ks)]
seq_ms, mix_ms, k16_ms = alternate([lambda: [single(t, k) for t, k in zip(tr, ks)], lambda: mixed(tr, ks), lambda: single(tr[-1], 16)])
got = mixed(tr, ks)
rows.append({"what": "sweep_k11_k16", "reps": REPS, "sequential_ms": seq_ms, "mixed_ms": mix_ms, "k16_alone_ms": k16_ms, "sequential_over_mixed": seq_ms / mix_ms,
             "mixed_over_k16_alone": mix_ms / k16_ms, "mixed_stage_ms_k16": got[-1][2], "mixed_stage_ms_k11": got[0][2]})
print(rows[-1], flush=True)
del tr

# (b) 64 traces of sizes 2^8..2^14
rng = random.Random(0x51235)
ks = [rng.randint(8, 14) for _ in range(64)]
tr = [synth(k, 0x7D000000 + 64 * k + i) for i, k in enumerate(ks)]
torch.cuda.synchronize()
by_k = {k: [i for i, kk in enumerate(ks) if kk == k] for k in sorted(set(ks))}


def grouped():
    out = [None] * len(ks)
    for k, idx in by_k.items():
        sched, r = shape(k)
        res = ctx.deep_fri_prove_batch_dev([[c.data_ptr() for c in tr[i]] for i in idx], 1 << k, DeepFriParams(sched, r, SEED_Z))
        for i, g in zip(idx, res):
            out[i] = g
    return out


assert [g[0] for g in mixed(tr, ks)] == [g[0] for g in grouped()]
grp_ms, mix_ms = alternate([grouped, lambda: mixed(tr, ks)])
got = mixed(tr, ks)
rows.append({"what": "batch64_k8_k14", "reps": REPS, "sizes": {str(k): len(v) for k, v in by_k.items()}, "grouped_calls": len(by_k), "grouped_ms": grp_ms, "mixed_ms": mix_ms,
             "grouped_over_mixed": grp_ms / mix_ms, "mixed_stage_ms_largest": got[ks.index(max(ks))][2]})
print(rows[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
ctx.close()
