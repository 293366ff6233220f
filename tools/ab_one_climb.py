#!/usr/bin/env python3
"""tools/ab_one_climb.py — the library of another build (the parent commit's, built in a second checkout) and this tree's in ONE process, called
alternately, over the batch side of every row of tools/merkle_batch_timing.py (build + roots), tools/merkle_mixed_timing.py, tools/sumcheck_batch_timing.py,
tools/sumcheck_mixed_timing.py and tools/prove_batch_timing.py (f0 batch), plus pair-leaf builds (arity 16, 4 and 2: the pair stream behind pointer
tables; the f0 batch rows run it at a pitch in their arity-2 last layer).  Two warm calls of each side, then ten alternating repetitions, host wall ms per
call (every call ends in a synchronisation); outputs compared byte for byte on every call.  A row passes when the medians differ by no more than the
larger of the two sides' own max - min.

    python tools/ab_one_climb.py PARENT/stark_mlwe_amd/libstark_mlwe_hip.so [OUT.jsonl [TOOL [THIS.so]]]     (writes one JSON line per row)

TOOL keeps the rows of one tool (a substring of its name, "" for all); THIS.so stands in for this tree's library (a build with one part of a change held back)."""
import ctypes as C, json, os, statistics, sys, time
import numpy as np
import torch  # first: one HIP runtime in the process
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stark_mlwe_amd._abi as abi
from stark_mlwe_amd.api import Context, DeepFriParams

REPS, Q, SEED_Z = 10, 2, 0xDEEFBAAD
vp = C.c_void_p


def context_of(path):
    lib = C.CDLL(path)
    for name, (res, args) in abi.SIGNATURES.items():
        fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
    abi._LIB = lib                       # Context() takes the library load_library() hands out
    return Context(0)


ONLY = sys.argv[3] if len(sys.argv) > 3 else ""
ctxs = {"parent": context_of(sys.argv[1]), "this": context_of(sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "stark_mlwe_amd", "libstark_mlwe_hip.so"))}
out = open(sys.argv[2] if len(sys.argv) > 2 else os.devnull, "w")
failed = 0


def synth(seed, col, n):
    t = torch.empty((n, 4), dtype=torch.int64, device="cuda"); c = ctxs["this"]
    c._chk(c.lib.stark_synth_column_dev(c.h, seed, col, 0, n, vp(t.data_ptr()))); torch.cuda.synchronize(); return t


def plain(v):
    return v.tobytes() if isinstance(v, np.ndarray) else v


def row(tool, what, fn):
    """fn(ctx) -> bytes / list of bytes / array"""
    global failed
    if ONLY not in tool:
        return
    ref = plain(fn(ctxs["parent"])); equal = True
    for _ in range(2):
        for w in ("parent", "this"):
            equal = equal and plain(fn(ctxs[w])) == ref
    ms = {"parent": [], "this": []}
    for _ in range(REPS):
        for w in ("parent", "this"):
            t0 = time.perf_counter(); v = fn(ctxs[w]); ms[w].append(round(1e3 * (time.perf_counter() - t0), 4)); equal = equal and plain(v) == ref
    med = {w: statistics.median(v) for w, v in ms.items()}; spread = {w: round(max(v) - min(v), 4) for w, v in ms.items()}
    rec = {"tool": tool, "row": what, "reps": REPS, "bytes_equal": bool(equal), "parent_median_ms": med["parent"], "parent_spread_ms": spread["parent"],
           "this_median_ms": med["this"], "this_spread_ms": spread["this"], "pass": bool(equal and abs(med["this"] - med["parent"]) <= max(spread.values()))}
    failed += not rec["pass"]
    print(json.dumps(rec), flush=True); out.write(json.dumps(rec) + "\n"); out.flush()


def roots_of(ctx, trees):
    r = ctx.merkle_roots_batch(trees)
    for t in trees:
        t.free()
    return r


# tools/merkle_batch_timing.py: build + roots (the open and verify rows do not build a tree), and the pair-leaf builds
for lg in (8, 12, 16):
    n = 1 << lg; cols = [synth(0x3E4C0000 + lg, b, n) for b in range(64)]
    for B in (1, 4, 16, 64):
        ptrs = [c.data_ptr() for c in cols[:B]]; labels = [1000 + b for b in range(B)]
        row("merkle_batch_timing", "build+roots, arity 16, n = 2^%d, B = %d" % (lg, B), lambda c: roots_of(c, c.merkle_build_batch_dev(ptrs, n, 16, labels, c.poseidon_params_for_arity(16))))
    if lg == 12:
        for arity in (16, 4, 2):
            ptrs = [c.data_ptr() for c in cols[:16]]; cps = [c.data_ptr() for c in cols[16:31]] + [None]; labels = [1000 + b for b in range(16)]
            row("merkle_batch_timing", "pair build+roots, arity %d, n = 2^12, B = 16, one null second column" % arity,
                lambda c: roots_of(c, c.merkle_build_batch_dev(ptrs, n, arity, labels, c.poseidon_params_for_arity(arity), cps)))
    del cols

# tools/merkle_mixed_timing.py
for lg, B in ((12, 64), (12, 1), (8, 64)):
    n = 1 << lg; cols = [synth(0x31D0000 + lg, b, n) for b in range(B)]; ptrs = [c.data_ptr() for c in cols]; labels = [1000 + b for b in range(B)]
    row("merkle_mixed_timing", "equal shapes through the mixed build, n = 2^%d, B = %d" % (lg, B), lambda c: roots_of(c, c.merkle_build_mixed_batch_dev(ptrs, [n] * B, 16, labels, c.poseidon_params_for_arity(16))))
for per in (1, 8):
    ns = [1 << lg for lg in range(8, 13) for _ in range(per)]; B = len(ns)
    cols = [synth(0x31E0000 + per, b, n) for b, n in enumerate(ns)]; ptrs = [c.data_ptr() for c in cols]; labels = [2000 + b for b in range(B)]
    row("merkle_mixed_timing", "2^8..2^12 leaves, %d trees per size" % per, lambda c: roots_of(c, c.merkle_build_mixed_batch_dev(ptrs, ns, 16, labels, c.poseidon_params_for_arity(16))))

# tools/sumcheck_batch_timing.py
for variant, k in (("plain", 12), ("plain", 14), ("plain", 16), ("mf", 12), ("mf", 14)):
    wit = [synth(0x5C0B0000 + 64 * k + b, b % 4, 1 << k) for b in range(256)]; ptrs = [w.data_ptr() for w in wit]; labels = [2025 if b % 2 == 0 else 7 for b in range(256)]
    for B in (1, 8, 64, 256):
        row("sumcheck_batch_timing", "%s, k = %d, B = %d" % (variant, k, B),
            (lambda c: c.prove_mf_batch_dev(k, labels[:B], Q, ptrs[:B])) if variant == "mf" else (lambda c: c.prove_plain_batch_dev(k, labels[:B], ptrs[:B])))
    del wit

# tools/sumcheck_mixed_timing.py
for variant, k_lo, k_hi in (("plain", 10, 16), ("mf", 10, 14)):
    for per in (1, 8):
        ks = [k for k in range(k_lo, k_hi + 1) for _ in range(per)]; B = len(ks)
        wit = [synth(0x5C3D0000 + 64 * k + b, b % 4, 1 << k) for b, k in enumerate(ks)]; ptrs = [w.data_ptr() for w in wit]; labels = [2025 if b % 2 == 0 else 7 for b in range(B)]
        row("sumcheck_mixed_timing", "%s, k = %d..%d, %d witnesses per k" % (variant, k_lo, k_hi, per),
            (lambda c: c.prove_mf_mixed_batch_dev(ks, labels, Q, ptrs)) if variant == "mf" else (lambda c: c.prove_plain_mixed_batch_dev(ks, labels, ptrs)))
        del wit

# tools/prove_batch_timing.py (a): the f0 batch
for k in (11, 12, 14, 16):
    sched, r = ([16, 16, 8], 32) if k >= 12 else ([16, 8], 8); n0 = 1 << k; prm = DeepFriParams(sched, r, SEED_Z)
    Bs = [B for B in (1, 4, 16, 64, 256) if B * n0 <= 1 << 24 and B <= 64]
    f0s = [synth(0x7B000000 + (k << 12) + p, 0, n0) for p in range(max(Bs))]; ptrs = [f.data_ptr() for f in f0s]
    for B in Bs:
        row("prove_batch_timing", "f0 batch, n0 = 2^%d, schedule %s, r = %d, B = %d" % (k, sched, r, B), lambda c: [g[0] for g in c.deep_fri_prove_f0_batch_dev(ptrs[:B], n0, prm)])
    del f0s
for c in ctxs.values():
    c.close()
print("rows that did not pass: %d" % failed)
