"""tools/merkle_batch_timing.py — the batched Merkle entry points against B single calls, arity 16 (t = 17), n = 2^8 / 2^12 / 2^16 leaves,
B = 1 / 4 / 16 / 64 trees, in one process:
  build   stark_merkle_build_batch_dev + stark_merkle_roots_batch            against  B x (stark_merkle_build_dev + stark_merkle_root)
  open    stark_merkle_open_batch, 32 random indices per tree                against  B x stark_merkle_open
  verify  stark_merkle_verify_many_ds_batch over those openings              against  B x stark_merkle_verify_many_ds
Outputs are compared byte for byte first.  Then batch and single loop run as alternating pairs (nine pairs after a warm-up pair), wall time on the
host around each side (every side ends in a synchronisation), medians.  A row says whether the batch is slower ("batch_slower": its median above
the single loop's).  The B = 1 open row is the figure for deciding whether the single open should become the batch with B = 1.
Writes profiles/merkle_batch_timing.jsonl (or the path given as the first argument).  Not product code."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from stark_mlwe_amd.api import Context, MerkleTree

ARITY, LOGS, BS, PAIRS, Q = 16, (8, 12, 16), (1, 4, 16, 64), 9, 32
ctx = Context(0); lib = ctx.lib; p17 = ctx.poseidon_params_for_arity(ARITY); cfg = ctx.merkle_cfg(ARITY)
vp = C.c_void_p


def wall_ms(fn):
    t0 = time.perf_counter(); v = fn(); return (time.perf_counter() - t0) * 1e3, v


def pairs(batch, single):
    batch(); single()
    bm, sm = [], []
    for _ in range(PAIRS):
        bm.append(wall_ms(batch)[0]); sm.append(wall_ms(single)[0])
    return statistics.median(bm), statistics.median(sm), [round(min(bm), 3), round(max(bm), 3)], [round(min(sm), 3), round(max(sm), 3)]


def single_build(ptr, n, label):
    h = vp(); ctx._chk(lib.stark_merkle_build_dev(ctx.h, p17.h, ARITY, label, vp(ptr), n, 0, None, 0, 0, 0, C.byref(h)))
    return MerkleTree(ctx, h, cfg.with_tree_label(label))


rows = []
rng = np.random.default_rng(0x3E4C1E)
for lg in LOGS:
    n = 1 << lg
    cols = torch.empty((max(BS), n, 4), dtype=torch.int64, device="cuda")
    for b in range(max(BS)):
        ctx._chk(lib.stark_synth_column_dev(ctx.h, 0x3E4C0000 + lg, b, 0, n, vp(cols[b].data_ptr())))
    torch.cuda.synchronize()
    for B in BS:
        ptrs = [cols[b].data_ptr() for b in range(B)]; labels = [1000 + b for b in range(B)]

        def build_batch():
            trees = ctx.merkle_build_batch_dev(ptrs, n, ARITY, labels, p17); roots = ctx.merkle_roots_batch(trees)
            for t in trees:
                t.free()
            return roots

        def build_single():
            out = np.zeros((B, 4), np.uint64)
            for b in range(B):
                t = single_build(ptrs[b], n, labels[b]); out[b] = t.root(); t.free()
            return out
        equal = bool((build_batch() == build_single()).all())
        bm, sm, bmm, smm = pairs(build_batch, build_single)
        rows.append({"op": "build+roots", "log_n": lg, "B": B, "batch_ms": round(bm, 3), "single_loop_ms": round(sm, 3), "batch_min_max_ms": bmm, "single_min_max_ms": smm,
                     "speedup": round(sm / bm, 2), "batch_slower": bm > sm, "outputs_equal": equal})
        print(json.dumps(rows[-1]), flush=True)

        trees = ctx.merkle_build_batch_dev(ptrs, n, ARITY, labels, p17); singles = [single_build(ptrs[b], n, labels[b]) for b in range(B)]
        ixs = [[int(i) for i in rng.integers(0, n, Q)] for _ in range(B)]
        open_batch = lambda: ctx.merkle_open_batch(trees, ixs)
        open_single = lambda: [singles[b].open_many(ixs[b]) for b in range(B)]
        proofs = open_batch(); equal = proofs == open_single()
        bm, sm, bmm, smm = pairs(open_batch, open_single)
        rows.append({"op": "open", "log_n": lg, "B": B, "queries": Q, "proof_bytes": len(proofs[0]), "batch_ms": round(bm, 3), "single_loop_ms": round(sm, 3), "batch_min_max_ms": bmm,
                     "single_min_max_ms": smm, "speedup": round(sm / bm, 2), "batch_slower": bm > sm, "outputs_equal": bool(equal)})
        print(json.dumps(rows[-1]), flush=True)

        roots = ctx.merkle_roots_batch(trees); vals = [singles[b].level(0)[ixs[b]] for b in range(B)]
        bad = B // 2                                                                    # one tampered opening per batch of two or more
        if B > 1:
            vals[bad] = vals[bad].copy(); vals[bad][-1, 0] ^= np.uint64(2)                # the last entry: where an index repeats, the later value is the one read
        verify_batch = lambda: ctx.merkle_verify_single_batch(ARITY, labels, list(roots), ixs, vals, proofs)
        verify_single = lambda: [ctx.merkle_verify_single(cfg.with_tree_label(labels[b]), roots[b], ixs[b], vals[b], proofs[b]) for b in range(B)]
        got = verify_batch(); equal = got == verify_single() and got == [not (B > 1 and b == bad) for b in range(B)]
        bm, sm, bmm, smm = pairs(verify_batch, verify_single)
        rows.append({"op": "verify", "log_n": lg, "B": B, "queries": Q, "batch_ms": round(bm, 3), "single_loop_ms": round(sm, 3), "batch_min_max_ms": bmm, "single_min_max_ms": smm,
                     "speedup": round(sm / bm, 2), "batch_slower": bm > sm, "outputs_equal": bool(equal)})
        print(json.dumps(rows[-1]), flush=True)
        for t in trees + singles:
            t.free()
    del cols
with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "merkle_batch_timing.jsonl"), "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
ctx.close()
