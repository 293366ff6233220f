"""tools/node_rate.py — per-permutation rate of the arity-16 Merkle node kernels against the pair-leaf kernel, in isolation (diagnostic).
Both sides run 2^20 permutations: a leaf layer of 2^20 pair leaves (k_leaf_pair2, one permutation per leaf) and a Merkle level of 2^19 nodes over
2^23 children (two permutations per node).  The level and the whole tree over 2^23 leaves are timed under every value of the option
"merkle_node16_pair" the library knows (1: the dedicated arity-16 node kernel, 0: the generic k_hash_ds2), with a digest of the outputs; the leaf
layer and the 2^19-node level also under every value of "poseidon_block8", alternating.
Prints JSON lines.  Not product code.
Usage: python tools/node_rate.py [path/to/libstark_variant.so]"""
import ctypes as C, hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import stark_mlwe_amd._abi as abi
if len(sys.argv) > 1:
    abi.lib_path = lambda: os.path.abspath(sys.argv[1])
from stark_mlwe_amd.api import Context, StarkError
dev = torch.device("cuda", 0)
ctx = Context(0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)); lib = ctx.lib
P = lambda t: C.c_void_p(t.data_ptr())
def dbuf(rows): return torch.empty((rows, 4), dtype=torch.int64, device=dev)
def timed(fn, reps=5):
    fn(); ms = C.c_float(); ctx._chk(lib.stark_timer_start(ctx.h))
    for _ in range(reps): fn()
    ctx._chk(lib.stark_timer_stop_ms(ctx.h, C.byref(ms))); return ms.value / reps
def digest(t): return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]
tp = ctx.transcript_params(); mp = ctx.poseidon_params_for_width(17)
n_leaf = 1 << 20
f, fn, h = dbuf(n_leaf), dbuf(n_leaf // 16), dbuf(n_leaf)
ctx._chk(lib.stark_synth_column_dev(ctx.h, 1, 0, 0, n_leaf, P(f))); ctx._chk(lib.stark_synth_column_dev(ctx.h, 1, 1, 0, n_leaf // 16, P(fn)))
n_in = 1 << 23
x = dbuf(n_in); ctx._chk(lib.stark_synth_column_dev(ctx.h, 1, 2, 0, n_in, P(x)))
# the leaf layer and the 2^19-node level under every value of "poseidon_block8" the library knows (1: partial rounds in blocks of 8 on the matrix
# cores, 0: blocks of 4 on the vector ALU), alternating, three rounds
try:
    ctx.set_option("poseidon_block8", 1); b8 = (1, 0)
except StarkError:
    b8 = (None,)
out19 = dbuf(1 << 19)
for rnd in range(3 if b8[0] is not None else 1):
    for opt in b8:
        if opt is not None: ctx.set_option("poseidon_block8", opt)
        ms = timed(lambda: ctx._chk(lib.stark_leaf_pair_hash_dev(ctx.h, tp.h, P(f), P(fn), n_leaf, 16, P(h))))
        print(json.dumps({"kernel": "k_leaf_pair2", "poseidon_block8": opt, "round": rnd, "leaves": n_leaf, "perms": n_leaf, "ms": round(ms, 3), "Mperm_s": round(n_leaf / ms / 1e3, 2), "digest": digest(h)}), flush=True)
        ms = timed(lambda: ctx._chk(lib.stark_poseidon_hash_ds_batch_dev(ctx.h, mp.h, 16, 1, 0, 0, P(x), (1 << 19) * 16, P(out19))))
        print(json.dumps({"kernel": "k_node16_pair", "poseidon_block8": opt, "round": rnd, "nodes": 1 << 19, "perms": 1 << 20, "ms": round(ms, 3), "Mperm_s": round((1 << 20) / ms / 1e3, 2), "digest": digest(out19)}), flush=True)
if b8[0] is not None: ctx.set_option("poseidon_block8", 1)
del f, fn, h, out19
try:
    ctx.set_option("merkle_node16_pair", 1); opts = (1, 0)
except StarkError:
    opts = (None,)
for opt in opts:
    if opt is not None: ctx.set_option("merkle_node16_pair", opt)
    for nodes in (1 << 19, 1 << 15, 1 << 13, 4097):
        out = dbuf(nodes)
        ms = timed(lambda: ctx._chk(lib.stark_poseidon_hash_ds_batch_dev(ctx.h, mp.h, 16, 1, 0, 0, P(x), nodes * 16, P(out))), reps=5 if nodes > 4097 else 20)
        print(json.dumps({"merkle_node16_pair": opt, "nodes": nodes, "perms": 2 * nodes, "ms": round(ms, 3), "Mperm_s": round(2 * nodes / ms / 1e3, 2), "digest": digest(out)}), flush=True)
    def tree():
        t = C.c_void_p(); ctx._chk(lib.stark_merkle_build_dev(ctx.h, mp.h, 16, 0, P(x), n_in, 0, None, 0, 0, 0, C.byref(t))); ctx.sync(); lib.stark_merkle_free(t)
    print(json.dumps({"merkle_node16_pair": opt, "tree_over_2^23_ms": round(timed(tree, reps=3), 3)}), flush=True)
if opts[0] is not None: ctx.set_option("merkle_node16_pair", 1)
ctx.close()
