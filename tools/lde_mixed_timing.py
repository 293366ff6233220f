"""tools/lde_mixed_timing.py — stark_lde_mixed_batch_dev against one stark_lde_batch_dev call per size (Pallas, blow-up 8, generator shift).

    python tools/lde_mixed_timing.py LIB [OUT.jsonl]     (default profiles/lde_mixed_timing.jsonl)

Rows: eight columns per size 2^8 .. 2^14 (the mixed call against the seven per-size calls, and against the 2^14 group alone: the floor); one column
per size 2^11 .. 2^16 (against the six per-size calls); 64 columns all 2^8 -> 2^11 (against stark_lde_batch_dev: on equal shapes both calls
launch the NttBatchAddr kernels, the mixed call from its plan and the batch call from its own driver).  Each row checks the outputs byte-equal, warms both sides and reports the medians of ten alternating repetitions (host wall clock
around call + synchronise: the launches are what is being compared)."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import stark_mlwe_amd._abi as abi
path = os.path.abspath(sys.argv[1]); abi.lib_path = lambda: path
from stark_mlwe_amd.api import Context, PALLAS_FR
import bench
dev = torch.device("cuda", 0)
ctx = Context(0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)); lib = ctx.lib
LB, REPS = 3, 10

def median_ms(fns):
    """medians of REPS alternating repetitions of every function in fns, in ms"""
    t = [[] for _ in fns]
    for _ in range(REPS):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter(); fn(); t[k].append(time.perf_counter() - t0)
    return [round(1e3 * statistics.median(x), 4) for x in t]

def row(name, lns, coset):
    """lns: log_n per column, grouped by size in ascending order"""
    xs = [torch.empty((1 << lg, 4), dtype=torch.int64, device=dev) for lg in lns]
    ym = [torch.empty((1 << (lg + LB), 4), dtype=torch.int64, device=dev) for lg in lns]; yg = [torch.empty_like(y) for y in ym]
    for c, (x, lg) in enumerate(zip(xs, lns)): ctx._chk(lib.stark_synth_column_dev(ctx.h, 3, c, 0, 1 << lg, C.c_void_p(x.data_ptr())))
    ip, mp, gp = [x.data_ptr() for x in xs], [y.data_ptr() for y in ym], [y.data_ptr() for y in yg]
    groups = [(lg, [i for i, l in enumerate(lns) if l == lg]) for lg in sorted(set(lns))]
    def mixed(): ctx.lde_mixed_batch_dev(PALLAS_FR, ip, lns, LB, mp, coset); ctx.sync()
    def group(lg, idx): ctx.lde_batch_dev(PALLAS_FR, [ip[i] for i in idx], lg, LB, [gp[i] for i in idx], coset)
    def grouped():
        for lg, idx in groups: group(lg, idx)
        ctx.sync()
    def largest(): group(*groups[-1]); ctx.sync()
    mixed(); grouped(); largest()
    assert all(torch.equal(a, b) for a, b in zip(ym, yg)), name
    m, g, f = median_ms([mixed, grouped, largest])
    return {"row": name, "log_n": sorted(set(lns)), "columns": len(lns), "log_blowup": LB, "mixed_ms": m, "per_size_calls": len(groups), "per_size_ms": g,
            "largest_group_alone_ms": f, "ratio_per_size_over_mixed": round(g / m, 3)}

out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lde_mixed_timing.jsonl")
coset = bench._mont_small(5); rows = []
for name, lns in (("eight columns per size, 2^8 .. 2^14", [lg for lg in range(8, 15) for _ in range(8)]),
                  ("one column per size, 2^11 .. 2^16", list(range(11, 17))),
                  ("64 columns, all 2^8", [8] * 64)):
    rows.append(row(name, lns, coset)); print(json.dumps(rows[-1]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
open(out, "w").write("".join(json.dumps(r) + "\n" for r in rows))
ctx.close()
