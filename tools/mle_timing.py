"""tools/mle_timing.py — stark_mle_evaluate_batch_dev against single calls, the device rate of one evaluation and the "mle_log_tile" sweep.

    python tools/mle_timing.py LIB [OUT.jsonl]     (default profiles/mle_evaluate_timing.jsonl)
    python tools/mle_timing.py LIB --one K         one warmed evaluation at 2^K and nothing else (for a kernel trace: the launches of the pass kernel)

kind "grid": k in {12, 14, 16} at B in {1, 16, 64, 256} and k = 20 at B in {1, 16}.  One batch call against B calls of stark_mle_evaluate_dev and
    against B calls of the host-pointer stark_mle_evaluate, which uploads its table and synchronises once per call (that is its contract, and part
    of what a caller of it pays): medians of ten alternating triples, host wall clock around calls + one synchronise; results checked equal first.
kind "device": one evaluation at k = 20 and 24 between stark_timer_start / stop (mean of 20 after a warm-up), as GB/s of table bytes read, next to a
    device-to-device copy of the same bytes in the same process (bytes read + bytes written per second, how BASELINE.md states the copy peak).
kind "sweep": every "mle_log_tile" of the range in both lane ownerships ("mle_lane_contiguous") at k = 16, B = 64 (wall, as the grid) and at k = 24,
    B = 1 (device time)."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import stark_mlwe_amd._abi as abi
path = os.path.abspath(sys.argv[1]); abi.lib_path = lambda: path
from stark_mlwe_amd.api import Context
dev = torch.device("cuda", 0)
ctx = Context(0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)); lib = ctx.lib
rng = np.random.default_rng(0x3E1E)

def points(B, k):   # stored limbs below 2^254 < r
    p = rng.integers(0, 1 << 62, size=(B, k, 4), dtype=np.uint64); return np.ascontiguousarray(p)

def tables(B, k):
    ts = [torch.empty((1 << k, 4), dtype=torch.int64, device=dev) for _ in range(B)]
    for c, t in enumerate(ts): ctx._chk(lib.stark_synth_column_dev(ctx.h, 0x3E1E + k, c, 0, 1 << k, C.c_void_p(t.data_ptr())))
    ctx.sync(); return ts

def device_ms(fn, reps=20):
    fn(); ctx.sync(); ms = C.c_float(); ctx._chk(lib.stark_timer_start(ctx.h))
    for _ in range(reps): fn()
    ctx._chk(lib.stark_timer_stop_ms(ctx.h, C.byref(ms))); return ms.value / reps

def wall_point(k, B, host_form=True, pairs=10):
    ts = tables(B, k); r = points(B, k); tp = [t.data_ptr() for t in ts]
    ob = torch.zeros((B, 4), dtype=torch.int64, device=dev); os_ = torch.zeros_like(ob)
    def batch(): ctx.mle_evaluate_batch_dev(tp, k, r, ob.data_ptr()); ctx.sync()
    def singles():
        for b in range(B): ctx.mle_evaluate_dev(tp[b], k, r[b], os_.data_ptr() + 32 * b)
        ctx.sync()
    batch(); singles()
    assert torch.equal(ob, os_), (k, B)
    row = {"k": k, "batch": B}
    if host_form:
        hts = [t.cpu().numpy().view(np.uint64) for t in ts]
        def hosts(): return np.stack([ctx.mle_evaluate(hts[b], r[b]) for b in range(B)])
        assert (hosts() == ob.cpu().numpy().view(np.uint64)).all(), (k, B)
    tb, tsg, th = [], [], []
    for _ in range(pairs):
        t0 = time.perf_counter(); batch(); tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); singles(); tsg.append(time.perf_counter() - t0)
        if host_form: t0 = time.perf_counter(); hosts(); th.append(time.perf_counter() - t0)
    b, s_ = 1e3 * statistics.median(tb), 1e3 * statistics.median(tsg)
    row.update(batch_ms=round(b, 4), singles_dev_ms=round(s_, 4), ratio_singles_dev_over_batch=round(s_ / b, 3))
    if host_form:
        h_ = 1e3 * statistics.median(th)
        row.update(host_form_ms=round(h_, 4), ratio_host_form_over_batch=round(h_ / b, 3), host_form_note="B calls of stark_mle_evaluate: each uploads its 2^k table and synchronises")
    return row

def device_point(k):
    t = tables(1, k)[0]; r = points(1, k); o = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    ms = device_ms(lambda: ctx.mle_evaluate_dev(t.data_ptr(), k, r[0], o.data_ptr()))
    return {"k": k, "batch": 1, "device_ms": round(ms, 5), "table_gbps": round((32 << k) / ms / 1e6, 1)}

if "--one" in sys.argv:
    k = int(sys.argv[sys.argv.index("--one") + 1]); t = tables(1, k)[0]; r = points(1, k); o = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    for _ in range(2): ctx.mle_evaluate_dev(t.data_ptr(), k, r[0], o.data_ptr()); ctx.sync()
    print(json.dumps({"k": k, "evaluations": 2})); ctx.close(); sys.exit(0)

out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mle_evaluate_timing.jsonl")
rows = []
def emit(row): rows.append(row); print(json.dumps(row), flush=True)
for k, Bs in ((12, (1, 16, 64, 256)), (14, (1, 16, 64, 256)), (16, (1, 16, 64, 256)), (20, (1, 16))):
    for B in Bs: emit(dict(wall_point(k, B), kind="grid"))
for k in (20, 24):
    row = device_point(k)
    a = torch.empty((1 << k, 4), dtype=torch.int64, device=dev); b = torch.empty_like(a); a.zero_()
    cms = device_ms(lambda: b.copy_(a))
    emit(dict(row, kind="device", copy_same_bytes_ms=round(cms, 5), copy_read_plus_write_gbps=round(2 * (32 << k) / cms / 1e6, 1)))
for T in range(3, 13):
    for contig in (0, 1):
        ctx.set_option("mle_log_tile", T); ctx.set_option("mle_lane_contiguous", contig)
        try:
            emit(dict(wall_point(16, 64, host_form=False), kind="sweep", mle_log_tile=T, mle_lane_contiguous=contig))
            emit(dict(device_point(24), kind="sweep", mle_log_tile=T, mle_lane_contiguous=contig))
        finally:
            ctx.set_option("mle_log_tile", -1); ctx.set_option("mle_lane_contiguous", -1)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
open(out, "w").write("".join(json.dumps(r) + "\n" for r in rows))
ctx.close()
