"""tools/lde_timing.py — stark_lde_dev 2^20 -> 2^23 (Pallas, coset 5) of the library given by path: ms per column and a checksum of the output.

    python tools/lde_timing.py LIB                      the single-column line (any library, also one without the batch entry points)
    python tools/lde_timing.py LIB --batch [OUT.jsonl]  stark_lde_batch_dev against B single calls (default profiles/lde_batch_timing.jsonl):
        grid log_n in {8, 10, 13, 17}, blow-up 8, B in {4, 16, 64}, and log_n 8, blow-up 4, B 64 (the padded route: a pad launch between the
        transforms); each point checks the outputs byte-equal, warms both sides and reports the
        medians of seven alternating pairs (host wall clock around call + synchronise: the launches are what is being compared);
        then option ntt_batch_max_elems from 2^12 to 2^26 at B = 64 for log_n = 8 and 13."""
import ctypes as C, hashlib, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import stark_mlwe_amd._abi as abi
path = os.path.abspath(sys.argv[1]); abi.lib_path = lambda: path
if "--batch" not in sys.argv:      # a library without the batch entry points (a parent build) is measured through the rest of the table
    for k in ("stark_ntt_batch_dev", "stark_lde_batch_dev"): abi.SIGNATURES.pop(k)
from stark_mlwe_amd.api import Context, PALLAS_FR, _ptr
import bench
dev = torch.device("cuda", 0)
ctx = Context(0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)); lib = ctx.lib

def batch_point(lg, lb, B, coset):
    xs = [torch.empty((1 << lg, 4), dtype=torch.int64, device=dev) for _ in range(B)]
    yb = [torch.empty((1 << (lg + lb), 4), dtype=torch.int64, device=dev) for _ in range(B)]; ys = [torch.empty_like(y) for y in yb]
    for c, x in enumerate(xs): ctx._chk(lib.stark_synth_column_dev(ctx.h, 3, c, 0, 1 << lg, C.c_void_p(x.data_ptr())))
    ip, bp, sp, cs = [x.data_ptr() for x in xs], [y.data_ptr() for y in yb], [y.data_ptr() for y in ys], _ptr(coset)
    def batch(): ctx.lde_batch_dev(PALLAS_FR, ip, lg, lb, bp, coset); ctx.sync()
    def singles():
        for i, o in zip(ip, sp): ctx._chk(lib.stark_lde_dev(ctx.h, PALLAS_FR, C.c_void_p(i), lg, lb, cs, C.c_void_p(o)))
        ctx.sync()
    batch(); singles()
    assert all(torch.equal(a, b) for a, b in zip(yb, ys)), (lg, lb, B)
    tb, ts = [], []
    for _ in range(7):
        t0 = time.perf_counter(); batch(); tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); singles(); ts.append(time.perf_counter() - t0)
    b, s_ = 1e3 * statistics.median(tb), 1e3 * statistics.median(ts)
    return {"log_n": lg, "log_blowup": lb, "batch": B, "batch_ms": round(b, 4), "singles_ms": round(s_, 4), "ratio_singles_over_batch": round(s_ / b, 3)}

if "--batch" in sys.argv:
    i = sys.argv.index("--batch")
    out = sys.argv[i + 1] if len(sys.argv) > i + 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lde_batch_timing.jsonl")
    coset = bench._mont_small(5); rows = []
    for lg in (8, 10, 13, 17):
        for B in (4, 16, 64):
            rows.append(dict(batch_point(lg, 3, B, coset), kind="grid")); print(json.dumps(rows[-1]), flush=True)
    rows.append(dict(batch_point(8, 2, 64, coset), kind="grid")); print(json.dumps(rows[-1]), flush=True)
    for lg in (8, 13):
        for le in range(12, 27, 2):
            ctx.set_option("ntt_batch_max_elems", 1 << le)
            try: rows.append(dict(batch_point(lg, 3, 64, coset), kind="sweep", log_ntt_batch_max_elems=le))
            finally: ctx.set_option("ntt_batch_max_elems", 1 << 24)
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("".join(json.dumps(r) + "\n" for r in rows))
    ctx.close(); sys.exit(0)
res = {"lib": os.path.basename(path)}
for lg, lb in ((20, 3), (16, 4), (18, 2)):
    x = torch.empty((1 << lg, 4), dtype=torch.int64, device=dev); y = torch.empty((1 << (lg + lb), 4), dtype=torch.int64, device=dev)
    ctx._chk(lib.stark_synth_column_dev(ctx.h, 3, 1, 0, 1 << lg, C.c_void_p(x.data_ptr())))
    coset = bench._mont_small(5)
    fn = lambda: ctx._chk(lib.stark_lde_dev(ctx.h, PALLAS_FR, C.c_void_p(x.data_ptr()), lg, lb, _ptr(coset), C.c_void_p(y.data_ptr())))
    fn(); ms = C.c_float(); ctx._chk(lib.stark_timer_start(ctx.h))
    for _ in range(10): fn()
    ctx._chk(lib.stark_timer_stop_ms(ctx.h, C.byref(ms)))
    res[f"lde_2^{lg}_x{1 << lb}_ms"] = round(ms.value / 10, 4); res[f"digest_{lg}_{lb}"] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()[:12]
print(json.dumps(res)); ctx.close()
