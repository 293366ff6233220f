"""tools/fri_shard_timing.py — the sharded commit phase at one rank and on W virtual ranks, against the one-GPU build, on the 2^23-point f0 of the
bench step (2^20 rows, blow-up 8, coset 5, z = 0xC0FFEE, [16,16,8]).  HIP events on the context's stream around each call; median of 25 runs after
3 warm-up runs.  stark_fri_build_dev is timed as it is (roots left on the device) and with its L+1 roots fetched, which the sharded build always does
(the query phase and the caller need them on the host).  Not product code."""
import ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stark_mlwe_amd.api import Context, _ptr
import bench
dev = torch.device("cuda", 0)
ctx = Context(0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)); lib = ctx.lib
P = lambda t: C.c_void_p(t.data_ptr())
WARM, RUNS = 3, 25


def median_ms(fn):
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(RUNS):
        ms = C.c_float(); ctx._chk(lib.stark_timer_start(ctx.h)); fn(); ctx._chk(lib.stark_timer_stop_ms(ctx.h, C.byref(ms))); out.append(ms.value)
    return round(statistics.median(out), 3)


k = 20; N = 1 << (k + bench.LOG_BLOWUP); L = len(bench.SCHEDULE)
sch = np.ascontiguousarray(bench.SCHEDULE, dtype=np.uint64)
cols = [torch.empty((1 << k, 4), dtype=torch.int64, device=dev) for _ in range(4)]
for c in range(4):
    ctx._chk(lib.stark_synth_column_dev(ctx.h, 0x5EED0000 + k, c, 0, 1 << k, P(cols[c])))
ext = [torch.empty((N, 4), dtype=torch.int64, device=dev) for _ in range(4)]
for c in range(4):
    ctx._chk(lib.stark_lde_dev(ctx.h, 0, P(cols[c]), k, bench.LOG_BLOWUP, _ptr(bench._mont_small(bench.STEP_COSET)), P(ext[c])))
f0 = torch.empty((N, 4), dtype=torch.int64, device=dev)
ctx._chk(lib.stark_ali_merge_dev(ctx.h, *[P(e) for e in ext], None, None, _ptr(bench._root_of_unity_pallas(k + bench.LOG_BLOWUP)), _ptr(bench._mont_small(bench.STEP_Z)), N, P(f0), None))
del ext, cols


def one_gpu(fetch_roots):
    st = C.c_void_p(); ctx._chk(lib.stark_fri_build_dev(ctx.h, P(f0), N, _ptr(sch), L, bench.SEED_Z, C.byref(st)))
    if fetch_roots:
        r = np.zeros(4, np.uint64); ctx._chk(lib.stark_fri_layer_root(st, 0, _ptr(r)))
    ctx._chk(lib.stark_fri_state_free(st))


def sharded_one_rank():
    h = C.c_void_p(); ctx._chk(lib.stark_fri_build_sharded_dev(ctx.h, P(f0), N, _ptr(sch), L, bench.SEED_Z, C.byref(h))); ctx._chk(lib.stark_fri_shard_free(h))


roots = np.zeros((8, L + 1, 4), np.uint64)
row = {"log_n0": k + bench.LOG_BLOWUP, "schedule": bench.SCHEDULE, "runs": RUNS,
       "fri_build_dev_ms": median_ms(lambda: one_gpu(False)),
       "fri_build_dev_with_roots_ms": median_ms(lambda: one_gpu(True)),
       "fri_build_sharded_dev_W1_ms": median_ms(sharded_one_rank)}
for W in (2, 4, 8):
    row[f"emulated_W{W}_all_ranks_ms"] = median_ms(lambda: ctx._chk(lib.stark_diag_fri_build_sharded_emulated_dev(ctx.h, W, P(f0), N, _ptr(sch), L, bench.SEED_Z, _ptr(roots))))
print(json.dumps(row), flush=True)
ctx.close()
