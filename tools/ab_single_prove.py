#!/usr/bin/env python3
"""tools/ab_single_prove.py — the library of another build (the parent commit's, built in a second checkout) and this tree's in ONE process,
called alternately: stark_deep_fri_prove_dev given f0 at 2^12 / 2^14 / 2^16, r = 32, schedule [16, 16, 8]; 3 warm-ups, 15 pairs per point; host wall
ms per call; proofs compared byte for byte.  A point is accepted when the medians differ by no more than the larger min-max spread.

    python tools/ab_single_prove.py PARENT/stark_mlwe_amd/libstark_mlwe_hip.so [OUT.jsonl]     (appends one JSON line per point)

The bench.py half of such a comparison needs no tool: `python bench.py --gpus 1 --steps 10 --warmup 2` in the two checkouts, alternating."""
import ctypes as C, json, os, statistics, sys, time
import numpy as np
import torch  # first: one HIP runtime in the process
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
SEED_Z = 0xDEEFBAAD

def load(path):
    lib = C.CDLL(path)
    lib.stark_ctx_create.restype = C.c_int32; lib.stark_ctx_create.argtypes = [C.c_int32, vp, C.POINTER(vp)]
    lib.stark_ctx_destroy.argtypes = [vp]
    lib.stark_deep_fri_prove_dev.restype = C.c_int32
    lib.stark_deep_fri_prove_dev.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_uint64, C.POINTER(vp)]
    lib.stark_proof_len.restype = C.c_size_t; lib.stark_proof_len.argtypes = [vp]
    lib.stark_proof_bytes.restype = C.c_int32; lib.stark_proof_bytes.argtypes = [vp, vp]
    lib.stark_proof_free.argtypes = [vp]
    lib.stark_ref_bench_inputs.restype = C.c_int32; lib.stark_ref_bench_inputs.argtypes = [C.c_uint64, C.c_size_t, C.c_size_t, vp]
    lib.stark_last_error.restype = C.c_char_p; lib.stark_last_error.argtypes = [vp]
    h = vp(); rc = lib.stark_ctx_create(0, None, C.byref(h)); assert rc == 0, rc
    return lib, h

libs = {"parent": load(sys.argv[1]),
        "this": load(os.path.join(ROOT, "stark_mlwe_amd", "libstark_mlwe_hip.so"))}
sched = np.array([16, 16, 8], np.uint64); r = 32
out = open(sys.argv[2] if len(sys.argv) > 2 else os.devnull, "a")

def prove(which, fptr, n0):
    lib, h = libs[which]; p = vp()
    t0 = time.perf_counter()
    rc = lib.stark_deep_fri_prove_dev(h, None, None, None, None, fptr, n0, sched.ctypes.data_as(vp), 3, r, SEED_Z, C.byref(p))
    dt = time.perf_counter() - t0
    assert rc == 0, (which, rc, lib.stark_last_error(h))
    n = lib.stark_proof_len(p); buf = (C.c_uint8 * n)(); lib.stark_proof_bytes(p, buf); lib.stark_proof_free(p)
    return 1e3 * dt, bytes(buf)

for k in (12, 14, 16):
    n0 = 1 << k
    hbuf = np.zeros((n0, 4), np.uint64); assert libs["this"][0].stark_ref_bench_inputs(0xF0 + k, n0, 1, hbuf.ctypes.data_as(vp)) == 0
    f = torch.from_numpy(hbuf.view(np.int64)).cuda(); torch.cuda.synchronize(); fptr = vp(f.data_ptr())
    ref = None
    for _ in range(3):
        for w in ("parent", "this"):
            _, b = prove(w, fptr, n0); ref = ref or b; assert b == ref
    ms = {"parent": [], "this": []}; equal = True
    for _ in range(15):
        for w in ("parent", "this"):
            dt, b = prove(w, fptr, n0); ms[w].append(round(dt, 4)); equal = equal and b == ref
    med = {w: statistics.median(v) for w, v in ms.items()}; spread = {w: round(max(v) - min(v), 4) for w, v in ms.items()}
    rec = {"point": "prove_dev given f0, n0 = 2^%d, r = 32, schedule [16, 16, 8]" % k, "pairs": 15, "bytes_equal": equal,
           "parent_ms": ms["parent"], "parent_median_ms": med["parent"], "parent_spread_ms": spread["parent"],
           "this_ms": ms["this"], "this_median_ms": med["this"], "this_spread_ms": spread["this"],
           "accept": equal and abs(med["this"] - med["parent"]) <= max(spread.values())}
    print(json.dumps(rec), flush=True); out.write(json.dumps(rec) + "\n"); out.flush()
for lib, h in libs.values():
    lib.stark_ctx_destroy(h)
