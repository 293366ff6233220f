"""tools/step_ab.py — A/B of the bench step (bench.make_single_gpu_step, N = 1) under option sets, in ONE process, runs alternating (diagnostic).
Each run: one warm-up step, then `steps` timed steps (wall clock, synchronised at both ends, as bench.py times them); every step's roots are checked
against the first configuration's.  Prints one JSON line per run and a summary line per configuration (mean, min, max, spread of ms/step).
Usage: python tools/step_ab.py [reps] [steps] [configs.json: a list of [name, {option: value}]]"""
import ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stark_mlwe_amd.api import Context
import bench

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
CONFIGS = [("new", {"merkle_node16_pair": 1, "fri_side_pair": 1}), ("old", {"merkle_node16_pair": 0, "fri_side_pair": 0}),
           ("node16_only", {"merkle_node16_pair": 1, "fri_side_pair": 0}), ("side_pair_only", {"merkle_node16_pair": 0, "fri_side_pair": 1})]
if len(sys.argv) > 3:
    CONFIGS = [tuple(c) for c in json.load(open(sys.argv[3]))]
dev = torch.device("cuda", 0); ts = torch.cuda.Stream(dev); torch.cuda.set_stream(ts)
ctx = Context(0, C.c_void_p(ts.cuda_stream)); lib = ctx.lib
lg = bench.LOG_TRACE; n = 1 << lg
cols = [torch.empty((n, 4), dtype=torch.int64, device=dev) for _ in range(4)]
for c in range(4):
    ctx._chk(lib.stark_synth_column_dev(ctx.h, 0x5EED0000 + lg, c, 0, n, C.c_void_p(cols[c].data_ptr())))
step = bench.make_single_gpu_step(ctx, cols, lg, dev)
ref = None; res = {name: [] for name, _ in CONFIGS}
for r in range(reps):
    for name, opts in CONFIGS:
        for k, v in opts.items():
            ctx.set_option(k, v)
        roots = step(); torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            got = bench.roots_hex(step())
            if ref is None: ref = got
            assert got == ref, (name, got, ref)
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / steps
        res[name].append(ms)
        print(json.dumps({"run": r, "config": name, "options": opts, "steps": steps, "ms_per_step": round(ms, 3)}), flush=True)
for name, opts in CONFIGS:
    v = res[name]
    print(json.dumps({"config": name, "options": opts, "runs": len(v), "mean_ms": round(sum(v) / len(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                      "spread_ms": round(max(v) - min(v), 3), "roots_equal_all_configs": True}), flush=True)
for k, v in CONFIGS[0][1].items():
    ctx.set_option(k, v)
ctx.close()
