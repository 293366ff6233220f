"""Host-side mirror of the reference's operator interface for the hot path, over the C-ABI.

Same names, argument meaning and error behaviour as the Rust functions in SURVEY.md §8(b)
(`permute`, `hash_with_ds_dynamic`, `MerkleTree::new/new_pairs`, `fri_fold_layer`, `compute_s_layer`,
`fri_build_transcript`, `deep_fri_prove`, `fft`/`ifft` …); a failed precondition raises StarkError where
the reference panics.  Field vectors are numpy uint64 arrays of shape (n, 4): the 4 little-endian
Montgomery limbs of ark-ff — the same bytes a Rust `&[F]` holds.

Everything here calls libstark_mlwe_hip.so; nothing is computed in Python.
"""
import ctypes as C

import numpy as np

from ._abi import StarkError, load_library

PALLAS_FR = 0
BLS12_381_FR = 1


def _arr(x, cols=4):
    a = np.ascontiguousarray(x, dtype=np.uint64)
    if a.ndim == 1 and cols == 4 and a.size == 4:
        a = a.reshape(1, 4)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Params:
    """PoseidonParams / PoseidonParamsDynamic handle (poseidon/src/lib.rs:16-21, 104-114)."""

    def __init__(self, ctx, handle, owned=True):
        self.ctx, self.h, self.owned = ctx, handle, owned
        t, rf, rp = C.c_int32(), C.c_int32(), C.c_int32()
        ctx._chk(ctx.lib.stark_poseidon_params_export(handle, C.byref(t), C.byref(rf), C.byref(rp), None, None, None))
        self.t, self.rounds_full, self.rounds_partial = t.value, rf.value, rp.value
        self.rate = self.t - 1

    def export(self):
        mds = np.zeros((self.t * self.t, 4), np.uint64)
        rcf = np.zeros((self.rounds_full * self.t, 4), np.uint64)
        rcp = np.zeros((self.rounds_partial, 4), np.uint64)
        self.ctx._chk(self.ctx.lib.stark_poseidon_params_export(self.h, None, None, None, _ptr(mds), _ptr(rcf), _ptr(rcp)))
        return mds, rcf, rcp

    def free(self):
        if self.owned and self.h:
            self.ctx.lib.stark_poseidon_params_free(self.h)
            self.h = None


class MerkleChannelCfg:
    """merkle/src/lib.rs:84-112."""

    def __init__(self, arity, params=None, tree_label=0):
        self.arity, self.params, self.tree_label = arity, params, tree_label

    def with_tree_label(self, label):
        return MerkleChannelCfg(self.arity, self.params, label)


class MerkleTree:
    """merkle/src/lib.rs:114-128: device-resident levels; `levels` materialises them lazily."""

    def __init__(self, ctx, handle, cfg, owned=True):
        self.ctx, self.h, self.cfg, self.owned = ctx, handle, cfg, owned

    @property
    def num_levels(self):
        return self.ctx.lib.stark_merkle_num_levels(self.h)

    def height(self):
        return self.num_levels - 1

    def level(self, lvl):
        n = self.ctx.lib.stark_merkle_level_len(self.h, lvl)
        out = np.zeros((n, 4), np.uint64)
        self.ctx._chk(self.ctx.lib.stark_merkle_level(self.h, lvl, _ptr(out)))
        return out

    @property
    def levels(self):
        return [self.level(i) for i in range(self.num_levels)]

    def root(self):
        out = np.zeros(4, np.uint64)
        self.ctx._chk(self.ctx.lib.stark_merkle_root(self.h, _ptr(out)))
        return out

    def gather(self, lvl, idx):
        ix = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.zeros((len(ix), 4), np.uint64)
        self.ctx._chk(self.ctx.lib.stark_merkle_gather(self.h, lvl, _ptr(ix), len(ix), _ptr(out)))
        return out

    def open_many(self, indices):
        """open_union_of_paths (merkle/src/lib.rs:246-315) -> canonical MerkleProof bytes."""
        ix = np.ascontiguousarray(indices, dtype=np.uint64)
        ln = C.c_size_t()
        self.ctx._chk(self.ctx.lib.stark_merkle_open(self.h, _ptr(ix), len(ix), None, 0, C.byref(ln)))
        buf = (C.c_uint8 * ln.value)()
        self.ctx._chk(self.ctx.lib.stark_merkle_open(self.h, _ptr(ix), len(ix), buf, ln.value, C.byref(ln)))
        return bytes(buf)

    open_many_single = open_many

    def free(self):
        if self.owned and self.h:
            self.ctx.lib.stark_merkle_free(self.h)
            self.h = None


class FriProverState:
    """fri.rs:210-216 (layers stay on the device)."""

    def __init__(self, ctx, handle, schedule):
        self.ctx, self.h, self.schedule = ctx, handle, list(schedule)

    @property
    def num_layers(self):
        return self.ctx.lib.stark_fri_num_layers(self.h)

    def f_layer(self, l):
        n = self.ctx.lib.stark_fri_layer_len(self.h, l)
        out = np.zeros((n, 4), np.uint64)
        self.ctx._chk(self.ctx.lib.stark_fri_layer_f(self.h, l, _ptr(out)))
        return out

    def root(self, l):
        out = np.zeros(4, np.uint64)
        self.ctx._chk(self.ctx.lib.stark_fri_layer_root(self.h, l, _ptr(out)))
        return out

    def z(self, l):
        out = np.zeros(4, np.uint64)
        self.ctx._chk(self.ctx.lib.stark_fri_layer_z(self.h, l, _ptr(out)))
        return out

    def tree(self, l):
        return MerkleTree(self.ctx, self.ctx.lib.stark_fri_layer_tree(self.h, l), None, owned=False)

    def free(self):
        if self.h:
            self.ctx.lib.stark_fri_state_free(self.h)
            self.h = None


class FriQueryPlan:
    """stark_fri_plan_t: the values the query phase needs, by (kind, which, level, index), and the assembler."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def requests(self):
        n = self.ctx.lib.stark_fri_plan_num_requests(self.h)
        kind = np.zeros(n, np.uint32); which = np.zeros(n, np.uint32); level = np.zeros(n, np.uint32); index = np.zeros(n, np.uint64)
        if n:
            self.ctx._chk(self.ctx.lib.stark_fri_plan_requests(self.h, _ptr(kind), _ptr(which), _ptr(level), _ptr(index)))
        return kind, which, level, index

    def assemble(self, values):
        v = _arr(values).reshape(-1, 4)
        h = C.c_void_p()
        self.ctx._chk(self.ctx.lib.stark_fri_plan_assemble(self.h, _ptr(v), v.shape[0], C.byref(h)))
        return self.ctx._proof_out(h)

    def free(self):
        if self.h:
            self.ctx.lib.stark_fri_plan_free(self.h)
            self.h = None


class FriShardState:
    """stark_fri_shard_t: this rank's part of a sharded commit phase (fri.rs:231-312); the roots are the same on every rank."""

    def __init__(self, ctx, handle, schedule):
        self.ctx, self.h, self.schedule = ctx, handle, list(schedule)

    @property
    def num_layers(self):
        return self.ctx.lib.stark_fri_shard_num_layers(self.h)

    def root(self, l):
        out = np.zeros(4, np.uint64)
        self.ctx._chk(self.ctx.lib.stark_fri_shard_root(self.h, l, _ptr(out)))
        return out

    def roots(self):
        return np.stack([self.root(l) for l in range(self.num_layers)])

    def is_sharded(self, l):
        v = self.ctx.lib.stark_fri_shard_is_sharded(self.h, l)
        if v < 0:
            raise StarkError(v, "layer out of range")
        return bool(v)

    def prove_queries(self, r):
        """Collective: the query phase (fri.rs:355-466, 613-640) -> (canonical proof bytes, size estimate), the same on every rank."""
        h = C.c_void_p()
        self.ctx._chk(self.ctx.lib.stark_fri_shard_prove_queries(self.h, r, C.byref(h)))
        return self.ctx._proof_out(h)

    def free(self):
        if self.h:
            self.ctx.lib.stark_fri_shard_free(self.h)
            self.h = None


def fri_shard_layout(n0, schedule, nranks):
    """The shard planner of the sharded commit phase (host-only): (sharded[l], stop_len[l]) for the L+1 layers; StarkError(-1) when
    nranks is not a power of two, does not divide n0, or the schedule does not divide n0."""
    lib = load_library()
    sch = np.ascontiguousarray(schedule, dtype=np.uint64)
    sharded = np.zeros(len(sch) + 1, np.int32); stop = np.zeros(len(sch) + 1, np.uint64)
    rc = lib.stark_fri_shard_layout(n0, _ptr(sch), len(sch), nranks, _ptr(sharded), _ptr(stop))
    if rc != 0:
        raise StarkError(rc, "stark_fri_shard_layout")
    return [bool(x) for x in sharded], [int(x) for x in stop]


def _dptr(x):
    """A device pointer: an int, None, or anything with data_ptr() (a torch CUDA tensor)."""
    if x is None:
        return None
    return C.c_void_p(x if isinstance(x, int) else x.data_ptr())


class Transcript:
    """transcript/src/lib.rs:48-117 (device-resident state; absorbs run with the next challenge)."""

    def __init__(self, ctx, label: bytes):
        self.ctx = ctx; self.h = C.c_void_p()
        ctx._chk(ctx.lib.stark_transcript_new(ctx.h, label, len(label), C.byref(self.h)))

    def absorb_bytes(self, b: bytes):
        self.ctx._chk(self.ctx.lib.stark_transcript_absorb_bytes(self.h, b, len(b)))

    def absorb_fields(self, xs):
        a = _arr(xs).reshape(-1, 4)
        self.ctx._chk(self.ctx.lib.stark_transcript_absorb_fields(self.h, _ptr(a), a.shape[0]))

    absorb_field = absorb_fields

    def challenge(self, label: bytes):
        out = np.zeros(4, np.uint64)
        self.ctx._chk(self.ctx.lib.stark_transcript_challenge(self.h, label, len(label), _ptr(out)))
        return out

    def challenges(self, label: bytes, n):
        out = np.zeros((n, 4), np.uint64)
        self.ctx._chk(self.ctx.lib.stark_transcript_challenges(self.h, label, len(label), n, _ptr(out)))
        return out

    def free(self):
        if self.h:
            self.ctx.lib.stark_transcript_free(self.h); self.h = None


def ref_bench_inputs(seed, n, ncols=4):
    """The reference's bench inputs (end_to_end.rs:249-253): (ncols, n, 4) uint64 Montgomery limbs.  Host-only."""
    lib = load_library(); out = np.zeros((ncols * n, 4), np.uint64)
    rc = lib.stark_ref_bench_inputs(seed, n, ncols, _ptr(out))
    if rc != 0:
        raise StarkError(rc, "stark_ref_bench_inputs")
    return out.reshape(ncols, n, 4)


def root_of_unity(log_n, field=PALLAS_FR):
    """F::get_root_of_unity(2^log_n) (host-only)."""
    lib = load_library(); out = np.zeros(4, np.uint64)
    rc = lib.stark_root_of_unity(field, log_n, _ptr(out))
    if rc != 0:
        raise StarkError(rc, "no root of unity of that order (two-adicity 32)")
    return out


class DeepFriParams:
    """fri.rs:589."""

    def __init__(self, schedule, r, seed_z):
        self.schedule, self.r, self.seed_z = list(schedule), r, seed_z


STREAM_PRIVATE = C.c_void_p(-1)      # STARK_STREAM_PRIVATE: a private non-blocking stream (the caller synchronises around its own device work)


class Context:
    """One context = one GPU = one host thread (include/stark_mlwe.h conventions).

    `stream`: a hipStream_t handle (e.g. `torch.cuda.current_stream().cuda_stream`), None for the device's legacy default
    stream (ordered against torch's default stream: safe without manual synchronisation), or STREAM_PRIVATE."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        h = C.c_void_p()
        if isinstance(stream, int):
            stream = C.c_void_p(stream) if stream else None
        rc = self.lib.stark_ctx_create(device, stream, C.byref(h))
        if rc != 0:
            raise StarkError(rc, "stark_ctx_create failed: no usable HIP device (the product path has no CPU fallback)")
        self.h = h
        v = stream.value if isinstance(stream, C.c_void_p) else None
        self.private_stream = v is not None and v == STREAM_PRIVATE.value
        self.stream_handle = -1 if self.private_stream else (v or 0)       # 0: the legacy default stream
        self._tparams = None
        self._mparams = {}

    def _chk(self, rc):
        if rc != 0:
            raise StarkError(rc, (self.lib.stark_last_error(self.h) or b"").decode())

    def close(self):
        if self.h:
            for p in list(self._mparams.values()) + ([self._tparams] if self._tparams else []):
                p.free()
            self.lib.stark_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        self._chk(self.lib.stark_ctx_sync(self.h))

    def set_option(self, key: str, value: int):
        """stark_ctx_set_option: "ntt_direct_max_log", "ntt_merged_coset", "ntt_log_tile", "ntt_min_waves", "poseidon_lane_only", "sponge_one_wave", "merkle_node16_pair", "poseidon_block8", "merkle_wave_pair", "fri_side_pair", "prove_batch_max_rows", "ntt_batch_max_elems", "mle_log_tile", "mle_lane_contiguous", "lagrange_max_partials", "lagrange_wide_acc", "lagrange_col_groups", "lagrange_shared_inverse", "lagrange_share_cosets", "mixed_prove_tail", "pool_poison" (tests only: fills the library's pooled temporaries, synchronises).  An unknown key raises StarkError (INVALID_ARG) listing the known ones."""
        self._chk(self.lib.stark_ctx_set_option(self.h, key.encode(), value))

    def trim(self):
        """Return the context's cached device blocks to the driver."""
        self._chk(self.lib.stark_ctx_trim(self.h))

    def cached_bytes(self):
        return int(self.lib.stark_ctx_cached_bytes(self.h))

    def diag_alloc_refusal(self, mode=-1, nth=0):
        """TESTS ONLY (stark_diag_alloc_refusal).  mode 1: the nth allocation request of the library from here on fails as out of memory (nth = 0: count
        only); mode 2: the first hipMalloc attempt of the nth request the pool cannot serve fails, so the pool gives its cached blocks back and retries;
        mode 3: both attempts of that request fail (the give-back runs and the call still fails); mode 0: off; mode -1: read only.  -> (requests counted
        since the last arming, refusals fired, live pooled blocks, live pooled bytes, cached bytes right after the last give-back or 2^64 - 1), read
        BEFORE the new mode is applied."""
        st = (C.c_uint64 * 5)()
        self._chk(self.lib.stark_diag_alloc_refusal(self.h, mode, nth, st))
        return tuple(int(x) for x in st)

    # ---- constants ------------------------------------------------------------------------------
    def poseidon_params_for_width(self, t):
        if t not in self._mparams:
            h = C.c_void_p()
            self._chk(self.lib.stark_poseidon_params_for_width(self.h, t, C.byref(h)))
            self._mparams[t] = Params(self, h)
        return self._mparams[t]

    def poseidon_params_for_arity(self, arity):
        t = 9 if arity <= 8 else 17 if arity <= 16 else 33 if arity <= 32 else 65 if arity <= 64 else 129
        if arity > 128:
            raise StarkError(-5, "unsupported Merkle arity; max supported = 128")
        return self.poseidon_params_for_width(t)

    def generate_params_t17_x5(self, seed: bytes):
        h = C.c_void_p()
        self._chk(self.lib.stark_poseidon_params_t17_seed(self.h, seed, len(seed), C.byref(h)))
        return Params(self, h)

    def transcript_params(self):
        if self._tparams is None:
            self._tparams = self.generate_params_t17_x5(b"POSEIDON-T17-X5-TRANSCRIPT")
        return self._tparams

    def params_upload(self, t, rf, rp, mds, rc_full, rc_partial):
        h = C.c_void_p()
        self._chk(self.lib.stark_poseidon_params_upload(self.h, t, rf, rp, _ptr(_arr(mds)), _ptr(_arr(rc_full)), _ptr(_arr(rc_partial)), C.byref(h)))
        return Params(self, h)

    # ---- poseidon -----------------------------------------------------------------------------------
    def permute(self, states, params):
        """permute / permute_dynamic over a batch: states (nstates, t, 4) -> same shape."""
        s = np.ascontiguousarray(states, dtype=np.uint64).copy()
        n = s.size // (params.t * 4)
        self._chk(self.lib.stark_poseidon_permute_batch(self.h, params.h, _ptr(s), n))
        return s

    permute_dynamic = permute

    def hash_with_ds_dynamic(self, ds_fields, inputs, params, n=1):
        ds, inp = _arr(ds_fields), _arr(inputs)
        nds, cnt = ds.shape[0] // n if ds.size else 0, inp.shape[0] // n if inp.size else 0
        out = np.zeros((n, 4), np.uint64)
        self._chk(self.lib.stark_poseidon_hash_with_ds_dynamic(self.h, params.h, _ptr(ds), nds, _ptr(inp), cnt, n, _ptr(out)))
        return out[0] if n == 1 else out

    def hash_with_ds(self, inputs, ds_tag, params):
        inp = _arr(inputs)
        out = np.zeros(4, np.uint64)
        self._chk(self.lib.stark_poseidon_hash_with_ds(self.h, params.h, _ptr(inp), inp.shape[0] if inp.size else 0, _ptr(_arr(ds_tag)), _ptr(out)))
        return out

    def hash_ds_level(self, params, arity, level, pos0, tree_label, children):
        ch = _arr(children)
        out = np.zeros(((ch.shape[0] + arity - 1) // arity, 4), np.uint64)
        self._chk(self.lib.stark_poseidon_hash_ds_batch(self.h, params.h, arity, level, pos0, tree_label, _ptr(ch), ch.shape[0], _ptr(out)))
        return out

    def leaf_pair_hash(self, f, f_next, m):
        """h[i] = hash_leaf_pair(f[i], f_next[i // m]) (f_next None => s = 0), fri.rs:283."""
        f = _arr(f)
        fn = None if f_next is None else _arr(f_next)
        out = np.zeros((f.shape[0], 4), np.uint64)
        self._chk(self.lib.stark_leaf_pair_hash(self.h, self.transcript_params().h, _ptr(f), _ptr(fn), f.shape[0], m, _ptr(out)))
        return out

    def hash_leaf_pair(self, f, s):
        return self.leaf_pair_hash(_arr(f), _arr(s), 1)[0]

    def tr_hash_fields_tagged(self, tag: bytes, fields, n=1):
        fl = _arr(fields)
        k = fl.shape[0] // n if fl.size else 0
        out = np.zeros((n, 4), np.uint64)
        self._chk(self.lib.stark_tr_hash_fields_tagged(self.h, None, tag, _ptr(fl), k, n, _ptr(out)))
        return out[0] if n == 1 else out

    def tr_hash_many_dev(self, items, out):
        """`items`: list of (tag bytes, DEVICE pointer of the fields (int; None or 0 allowed when k == 0), k); `out`: DEVICE pointer (int) of
        len(items) x 4 words.  out[i] = tr_hash_fields_tagged(tag_i, fields_i[0 .. k_i)), all items in one launch whatever their tags and lengths,
        stream-ordered (stark_tr_hash_many_dev)."""
        n = len(items)
        tags = (C.c_char_p * max(n, 1))(*[it[0] for it in items])
        flds = (C.c_void_p * max(n, 1))(*[int(it[1]) if it[1] else None for it in items])
        ks = (C.c_size_t * max(n, 1))(*[int(it[2]) for it in items])
        self._chk(self.lib.stark_tr_hash_many_dev(self.h, n, tags, flds, ks, C.c_void_p(int(out) if out else None)))

    # ---- merkle -------------------------------------------------------------------------------------
    def merkle_cfg(self, arity, tree_label=0):
        """MerkleChannelCfg::new(arity).with_tree_label(label)."""
        return MerkleChannelCfg(arity, self.poseidon_params_for_arity(arity), tree_label)

    def merkle_new(self, leaves, cfg):
        lv = _arr(leaves)
        h = C.c_void_p()
        self._chk(self.lib.stark_merkle_build(self.h, cfg.params.h, cfg.arity, cfg.tree_label, _ptr(lv), lv.shape[0] if lv.size else 0, 0, None, C.byref(h)))
        return MerkleTree(self, h, cfg)

    def merkle_new_pairs(self, f_vals, cp_vals, cfg):
        f, cp = _arr(f_vals), _arr(cp_vals)
        if f.shape != cp.shape:
            raise StarkError(-1, "f and cp length mismatch")
        h = C.c_void_p()
        self._chk(self.lib.stark_merkle_build(self.h, cfg.params.h, cfg.arity, cfg.tree_label, _ptr(f), f.shape[0] if f.size else 0, 1, _ptr(cp), C.byref(h)))
        return MerkleTree(self, h, cfg)

    def merkle_build_batch_dev(self, leaves, n, cfg_arity, tree_labels, params, cp=None):
        """MerkleTree::new / new_pairs of each of the DEVICE columns `leaves` (ints, n elements each) in one pass, one launch per level for the whole
        batch; `cp`: None, or a list of DEVICE pointers / None per tree (None = a zero column).  Stream-ordered, no synchronisation.  -> list of
        MerkleTree, each equal to the single build of that column (stark_merkle_build_batch_dev)."""
        B = len(leaves)
        if len(tree_labels) != B or (cp is not None and len(cp) != B):
            raise StarkError(-1, "one tree label (and one cp entry) per tree")
        tab = (C.c_void_p * max(B, 1))(*[None if x is None else int(x) for x in leaves])
        ctab = None if cp is None else (C.c_void_p * max(B, 1))(*[None if x is None else int(x) for x in cp])
        lab = np.ascontiguousarray(tree_labels, dtype=np.uint64)
        out = (C.c_void_p * max(B, 1))()
        self._chk(self.lib.stark_merkle_build_batch_dev(self.h, params.h, cfg_arity, B, _ptr(lab), tab, n, 0 if cp is None else 1, ctab, out))
        return [MerkleTree(self, C.c_void_p(out[b]), MerkleChannelCfg(cfg_arity, params, int(lab[b]))) for b in range(B)]

    def commitment_commit_batch_dev(self, ds_tags, leaves, n):
        """MerkleCommitment::commit of each of the DEVICE vectors `leaves` (ints, n elements) in one pass -> list of MerkleTree
        (stark_commitment_commit_batch_dev)."""
        B = len(leaves)
        if len(ds_tags) != B:
            raise StarkError(-1, "one ds_tag per vector")
        tab = (C.c_void_p * max(B, 1))(*[None if x is None else int(x) for x in leaves])
        lab = np.ascontiguousarray(ds_tags, dtype=np.uint64)
        out = (C.c_void_p * max(B, 1))()
        self._chk(self.lib.stark_commitment_commit_batch_dev(self.h, B, _ptr(lab), tab, n, out))
        return [MerkleTree(self, C.c_void_p(out[b]), MerkleChannelCfg(16, None, int(lab[b]))) for b in range(B)]

    def merkle_build_mixed_batch_dev(self, leaves, n, cfg_arity, tree_labels, params, cp=None):
        """merkle_build_batch_dev for trees of different lengths: `n` is a list, tree i has n[i] >= 1 leaves; one launch per level over the trees
        that still have that level.  Stream-ordered, no synchronisation.  -> list of MerkleTree, each equal to the single build of that column
        (stark_merkle_build_mixed_batch_dev)."""
        B = len(leaves)
        if len(tree_labels) != B or len(n) != B or (cp is not None and len(cp) != B):
            raise StarkError(-1, "one tree label, one length (and one cp entry) per tree")
        tab = (C.c_void_p * max(B, 1))(*[None if x is None else int(x) for x in leaves])
        ctab = None if cp is None else (C.c_void_p * max(B, 1))(*[None if x is None else int(x) for x in cp])
        lab = np.ascontiguousarray(tree_labels, dtype=np.uint64)
        ns = (C.c_size_t * max(B, 1))(*[int(x) for x in n])
        out = (C.c_void_p * max(B, 1))()
        self._chk(self.lib.stark_merkle_build_mixed_batch_dev(self.h, params.h, cfg_arity, B, _ptr(lab), tab, ns, 0 if cp is None else 1, ctab, out))
        return [MerkleTree(self, C.c_void_p(out[b]), MerkleChannelCfg(cfg_arity, params, int(lab[b]))) for b in range(B)]

    def commitment_commit_mixed_batch_dev(self, ds_tags, leaves, n):
        """MerkleCommitment::commit of each of the DEVICE vectors `leaves` (ints; vector i has n[i] elements) in one pass -> list of MerkleTree
        (stark_commitment_commit_mixed_batch_dev)."""
        B = len(leaves)
        if len(ds_tags) != B or len(n) != B:
            raise StarkError(-1, "one ds_tag and one length per vector")
        tab = (C.c_void_p * max(B, 1))(*[None if x is None else int(x) for x in leaves])
        lab = np.ascontiguousarray(ds_tags, dtype=np.uint64)
        ns = (C.c_size_t * max(B, 1))(*[int(x) for x in n])
        out = (C.c_void_p * max(B, 1))()
        self._chk(self.lib.stark_commitment_commit_mixed_batch_dev(self.h, B, _ptr(lab), tab, ns, out))
        return [MerkleTree(self, C.c_void_p(out[b]), MerkleChannelCfg(16, None, int(lab[b]))) for b in range(B)]

    def merkle_roots_batch(self, trees):
        """The roots of `trees` (MerkleTree, one context) as a (B, 4) array with one download (stark_merkle_roots_batch)."""
        B = len(trees)
        tab = (C.c_void_p * max(B, 1))(*[t.h for t in trees])
        out = np.zeros((B, 4), np.uint64)
        self._chk(self.lib.stark_merkle_roots_batch(tab, B, _ptr(out)))
        return out

    def merkle_open_batch(self, trees, indices):
        """open_union_of_paths of every tree of `trees` (any shapes, one context) at indices[i], all siblings in one gather -> list of canonical
        MerkleProof bytes, each equal to trees[i].open_many(indices[i]) (stark_merkle_open_batch)."""
        B = len(trees)
        if len(indices) != B:
            raise StarkError(-1, "one index list per tree")
        off = np.zeros(B + 1, np.uint64); off[1:] = np.cumsum([len(ix) for ix in indices])
        ix = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in indices]) if B else np.zeros(0), dtype=np.uint64)
        tab = (C.c_void_p * max(B, 1))(*[t.h for t in trees])
        out = (C.c_void_p * max(B, 1))()
        self._chk(self.lib.stark_merkle_open_batch(tab, B, _ptr(ix), _ptr(off), out))
        return [self._proof_out(C.c_void_p(out[b]))[0] for b in range(B)]

    def merkle_verify_single_batch(self, cfg_arity, tree_labels, roots, indices, leaves, proofs) -> list:
        """MerkleProver::verify_single on each of the openings (tree_labels[i], roots[i], indices[i], leaves[i], proofs[i]) in one device pass;
        one bool per opening, each equal to merkle_verify_single of it alone (stark_merkle_verify_many_ds_batch)."""
        B = len(proofs)
        if not (len(tree_labels) == len(roots) == len(indices) == len(leaves) == B):
            raise StarkError(-1, "one label, root, index list and value list per proof")
        if B == 0:
            return []
        off = np.zeros(B + 1, np.uint64); off[1:] = np.cumsum([len(ix) for ix in indices])
        ix = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in indices]), dtype=np.uint64)
        vals = np.ascontiguousarray(np.concatenate([_arr(v).reshape(-1, 4) for v in leaves]), dtype=np.uint64)
        if vals.shape[0] != ix.shape[0]:
            raise StarkError(-1, "one value per index")
        bufs = [(C.c_uint8 * max(1, len(p))).from_buffer_copy(bytes(p) or b"\0") for p in proofs]
        ptrs = (C.c_void_p * B)(*[C.cast(b, C.c_void_p) for b in bufs])
        lens = (C.c_size_t * B)(*[len(p) for p in proofs])
        lab = np.ascontiguousarray(tree_labels, dtype=np.uint64); rt = np.ascontiguousarray(np.stack([_arr(r).reshape(4) for r in roots]), dtype=np.uint64)
        acc = (C.c_int32 * B)()
        self._chk(self.lib.stark_merkle_verify_many_ds_batch(self.h, cfg_arity, B, _ptr(lab), _ptr(rt), _ptr(ix), _ptr(off), _ptr(vals), ptrs, lens, acc))
        return [bool(acc[i]) for i in range(B)]

    # ---- fri ---------------------------------------------------------------------------------------
    def fri_sample_z_ell(self, seed_z, level, domain_size):
        out = np.zeros(4, np.uint64)
        self._chk(self.lib.stark_fri_sample_z(self.h, None, seed_z, level, domain_size, _ptr(out)))
        return out

    def fri_fold_layer(self, f_l, z_l, m):
        f = _arr(f_l)
        n = f.shape[0] if f.size else 0
        out = np.zeros((n // m if m else 0, 4), np.uint64)
        self._chk(self.lib.stark_fri_fold(self.h, _ptr(f), n, _ptr(_arr(z_l)), m, _ptr(out)))
        return out

    def compute_s_layer(self, f_l, z_l, m):
        """fri.rs:123-143: s[i] = fold(f)[i // m] — a replicated view of the folded layer."""
        return np.repeat(self.fri_fold_layer(f_l, z_l, m), m, axis=0)

    def fri_build_transcript(self, f0, schedule, seed_z):
        f = _arr(f0)
        sch = np.ascontiguousarray(schedule, dtype=np.uint64)
        h = C.c_void_p()
        self._chk(self.lib.stark_fri_build(self.h, _ptr(f), f.shape[0], _ptr(sch), len(sch), seed_z, C.byref(h)))
        return FriProverState(self, h, schedule)

    # ---- deep-ali / prove -----------------------------------------------------------------------------
    def deep_ali_merge_evals(self, a, s, e, t, omega, z, r_eval=None, beta=None, want_c_star=True):
        a, s, e, t = _arr(a), _arr(s), _arr(e), _arr(t)
        n = a.shape[0]
        f0 = np.zeros((n, 4), np.uint64)
        cs = np.zeros(4, np.uint64) if want_c_star else None
        r = None if r_eval is None else _arr(r_eval)
        b = None if beta is None else _arr(beta)
        self._chk(self.lib.stark_ali_merge(self.h, _ptr(a), _ptr(s), _ptr(e), _ptr(t), _ptr(r), _ptr(b), _ptr(_arr(omega)), _ptr(_arr(z)), n, _ptr(f0), _ptr(cs)))
        return f0, _arr(z).reshape(4), cs

    def build_f0(self, a, s, e, t, n0):
        """DeepAliRealBuilder::default().build_f0 (fri.rs:535-569); returns (f0, aux[7])."""
        a, s, e, t = _arr(a), _arr(s), _arr(e), _arr(t)
        f0 = np.zeros((n0, 4), np.uint64)
        aux = np.zeros((7, 4), np.uint64)
        self._chk(self.lib.stark_build_f0(self.h, _ptr(a), _ptr(s), _ptr(e), _ptr(t), n0, _ptr(f0), _ptr(aux)))
        return f0, aux

    def deep_fri_prove(self, a, s, e, t, n0, params: DeepFriParams, f0=None):
        """deep_fri_prove (fri.rs:601-641) -> (canonical proof bytes, size estimate, stage ms)."""
        sch = np.ascontiguousarray(params.schedule, dtype=np.uint64)
        h = C.c_void_p()
        if f0 is None:
            a, s, e, t = _arr(a), _arr(s), _arr(e), _arr(t)
            self._chk(self.lib.stark_deep_fri_prove(self.h, _ptr(a), _ptr(s), _ptr(e), _ptr(t), None, n0, _ptr(sch), len(sch), params.r, params.seed_z, C.byref(h)))
        else:
            f = _arr(f0)
            self._chk(self.lib.stark_deep_fri_prove(self.h, None, None, None, None, _ptr(f), n0, _ptr(sch), len(sch), params.r, params.seed_z, C.byref(h)))
        try:
            ln = self.lib.stark_proof_len(h)
            buf = (C.c_uint8 * ln)()
            self._chk(self.lib.stark_proof_bytes(h, buf))
            est = self.lib.stark_proof_size_estimate(h)
            ms = [self.lib.stark_proof_stage_ms(h, i) for i in range(3)]
        finally:
            self.lib.stark_proof_free(h)
        return bytes(buf), est, ms

    def deep_fri_prove_batch_dev(self, traces, n0, params: DeepFriParams):
        """`traces`: list of (a, s, e, t) DEVICE pointers (ints) of independent n0-row traces -> list of (proof bytes, size estimate, stage ms),
        each equal to deep_fri_prove of that trace alone; the 4 * len(traces) serial column sponges run concurrently (stark_deep_fri_prove_batch_dev)."""
        B = len(traces)
        sch = np.ascontiguousarray(params.schedule, dtype=np.uint64)
        cols = [(C.c_void_p * B)(*[int(tr[c]) for tr in traces]) for c in range(4)]
        out = (C.c_void_p * B)()
        self._chk(self.lib.stark_deep_fri_prove_batch_dev(self.h, B, cols[0], cols[1], cols[2], cols[3], n0, _ptr(sch), len(sch), params.r, params.seed_z, out))
        return self._proofs_out(out, B)

    def deep_fri_prove_mixed_batch_dev(self, traces, shapes, seed_z):
        """`traces`: list of (a, s, e, t) DEVICE pointers (ints) of independent traces of ANY sizes; `shapes`: per trace (n0, schedule, r) ->
        list of (proof bytes, size estimate, stage ms), each equal to deep_fri_prove of that trace alone under its own shape.  All column sponges
        run in one launch; traces of equal shape share the batched tail — under set_option("mixed_prove_tail", 1) traces of equal schedule share one
        ragged tail whatever their n0 and r (stark_deep_fri_prove_mixed_batch_dev)."""
        B = len(traces)
        cols = [(C.c_void_p * max(B, 1))(*[int(tr[c]) if tr[c] else None for tr in traces]) for c in range(4)]
        n0 = (C.c_size_t * max(B, 1))(*[int(sh[0]) for sh in shapes])
        r = (C.c_size_t * max(B, 1))(*[int(sh[2]) for sh in shapes])
        flat, off = [], [0]
        for sh in shapes:
            flat += [int(m) for m in sh[1]]; off.append(len(flat))
        sch = (C.c_size_t * max(len(flat), 1))(*flat)
        offs = (C.c_size_t * len(off))(*off)
        out = (C.c_void_p * max(B, 1))()
        self._chk(self.lib.stark_deep_fri_prove_mixed_batch_dev(self.h, B, cols[0], cols[1], cols[2], cols[3], n0, sch, offs, r, seed_z, out))
        return self._proofs_out(out, B)

    def _proofs_out(self, out, B):
        res = []
        for p in range(B):
            h = C.c_void_p(out[p])
            try:
                ln = self.lib.stark_proof_len(h); buf = (C.c_uint8 * ln)()
                self._chk(self.lib.stark_proof_bytes(h, buf))
                res.append((bytes(buf), self.lib.stark_proof_size_estimate(h), [self.lib.stark_proof_stage_ms(h, i) for i in range(3)]))
            finally:
                self.lib.stark_proof_free(h)
        return res

    def deep_fri_prove_f0_batch_dev(self, f0s, n0, params: DeepFriParams):
        """`f0s`: DEVICE pointers (ints) of independent n0-element f0 vectors -> list of (proof bytes, size estimate, stage ms), each equal to
        deep_fri_prove(f0=...) of that vector alone; merge-free tails side by side (stark_deep_fri_prove_f0_batch_dev)."""
        B = len(f0s)
        sch = np.ascontiguousarray(params.schedule, dtype=np.uint64)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in f0s])
        out = (C.c_void_p * max(B, 1))()
        self._chk(self.lib.stark_deep_fri_prove_f0_batch_dev(self.h, B, tab, n0, _ptr(sch), len(sch), params.r, params.seed_z, out))
        return self._proofs_out(out, B)

    def fri_commit_batch_dev(self, f0s, n0, schedule, seed_z):
        """The L + 1 layer roots of fri_build_transcript for each of the DEVICE vectors `f0s` (ints), as a (B, L + 1, 4) array
        (stark_fri_commit_batch_dev)."""
        B = len(f0s)
        sch = np.ascontiguousarray(schedule, dtype=np.uint64)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in f0s])
        roots = np.zeros((B, len(sch) + 1, 4), np.uint64)
        self._chk(self.lib.stark_fri_commit_batch_dev(self.h, B, tab, n0, _ptr(sch), len(sch), seed_z, _ptr(roots)))
        return roots

    def ali_merge_batch_dev(self, traces, omega, zs, n, f0s, r_opts=None, betas=None, want_c_star=True):
        """deep_ali_merge_evals(_blinded) of B traces in one launch: `traces` = list of (a, s, e, t) DEVICE pointers, `f0s` the B DEVICE outputs,
        `zs` (B, 4) host, `r_opts` None or a list of DEVICE pointers / None per trace with `betas` (B, 4) host.  Returns c* as (B, 4) or None
        (stark_ali_merge_batch_dev)."""
        B = len(traces)
        cols = [(C.c_void_p * max(B, 1))(*[int(tr[c]) for tr in traces]) for c in range(4)]
        outs = (C.c_void_p * max(B, 1))(*[int(x) for x in f0s])
        rt = None if r_opts is None else (C.c_void_p * max(B, 1))(*[None if x is None else int(x) for x in r_opts])
        bt = None if betas is None else _arr(betas)
        z = _arr(zs)
        cs = np.zeros((B, 4), np.uint64) if want_c_star else None
        self._chk(self.lib.stark_ali_merge_batch_dev(self.h, B, cols[0], cols[1], cols[2], cols[3], rt, _ptr(bt), _ptr(_arr(omega)), _ptr(z), n, outs, _ptr(cs)))
        return cs

    def ntt_batch_dev(self, field, datas, log_n, inverse=False, coset=None):
        """stark_ntt_dev of each of the DEVICE vectors `datas` (ints, 2^log_n elements each, transformed in place) with one coset, every pass of the
        transform one launch for all of them; stream-ordered, no synchronisation (stark_ntt_batch_dev)."""
        B = len(datas)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in datas])
        self._chk(self.lib.stark_ntt_batch_dev(self.h, field, B, tab, log_n, 1 if inverse else 0, _ptr(None if coset is None else _arr(coset))))

    def lde_batch_dev(self, field, evals, log_n, log_blowup, outs, coset=None):
        """stark_lde_dev of each of the DEVICE columns `evals` (ints, 2^log_n elements) into the DEVICE vectors `outs` (2^(log_n + log_blowup) elements)
        with one coset, every step one launch for all columns; stream-ordered, no synchronisation (stark_lde_batch_dev)."""
        B = len(evals)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in evals])
        otab = (C.c_void_p * max(B, 1))(*[int(x) for x in outs])
        self._chk(self.lib.stark_lde_batch_dev(self.h, field, B, tab, log_n, log_blowup, _ptr(None if coset is None else _arr(coset)), otab))

    def ntt_mixed_batch_dev(self, field, datas, log_ns, inverse=False, coset=None):
        """stark_ntt_dev of each of the DEVICE vectors `datas` (ints; vector i has 2^log_ns[i] elements, transformed in place) with one coset: vectors
        of any lengths share the launches of a three-step schedule; stream-ordered, no synchronisation (stark_ntt_mixed_batch_dev)."""
        B = len(datas)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in datas])
        lg = (C.c_size_t * max(B, 1))(*[int(x) for x in log_ns])
        self._chk(self.lib.stark_ntt_mixed_batch_dev(self.h, field, B, tab, lg, 1 if inverse else 0, _ptr(None if coset is None else _arr(coset))))

    def lde_mixed_batch_dev(self, field, evals, log_ns, log_blowup, outs, coset=None):
        """stark_lde_dev of each of the DEVICE columns `evals` (ints; column i has 2^log_ns[i] elements) into the DEVICE vectors `outs`
        (2^(log_ns[i] + log_blowup) elements) with one blow-up and one coset, columns of any lengths in the same launches; stream-ordered, no
        synchronisation (stark_lde_mixed_batch_dev)."""
        B = len(evals)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in evals])
        otab = (C.c_void_p * max(B, 1))(*[int(x) for x in outs])
        lg = (C.c_size_t * max(B, 1))(*[int(x) for x in log_ns])
        self._chk(self.lib.stark_lde_mixed_batch_dev(self.h, field, B, tab, lg, log_blowup, _ptr(None if coset is None else _arr(coset)), otab))

    def deep_fri_verify(self, params: DeepFriParams, proof: bytes) -> bool:
        """deep_fri_verify (fri.rs:643-762) on canonical proof bytes."""
        sch = np.ascontiguousarray(params.schedule, dtype=np.uint64)
        buf = (C.c_uint8 * max(1, len(proof))).from_buffer_copy(proof or b"\0")
        ok = C.c_int32(0)
        self._chk(self.lib.stark_deep_fri_verify(self.h, buf, len(proof), _ptr(sch), len(sch), params.r, params.seed_z, C.byref(ok)))
        return bool(ok.value)

    def deep_fri_verify_batch(self, params: DeepFriParams, proofs) -> list:
        """deep_fri_verify (fri.rs:643-762) on each of `proofs` (canonical bytes, one schedule and r), in one device pass; one bool per proof."""
        n = len(proofs)
        if n == 0:
            return []
        sch = np.ascontiguousarray(params.schedule, dtype=np.uint64)
        bufs = [(C.c_uint8 * max(1, len(p))).from_buffer_copy(bytes(p) or b"\0") for p in proofs]
        ptrs = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
        lens = (C.c_size_t * n)(*[len(p) for p in proofs])
        acc = (C.c_int32 * n)()
        self._chk(self.lib.stark_deep_fri_verify_batch(self.h, n, ptrs, lens, _ptr(sch), len(sch), params.r, params.seed_z, acc))
        return [bool(acc[i]) for i in range(n)]

    def merkle_verify_single(self, cfg, root, indices, leaves, proof: bytes) -> bool:
        """MerkleProver::verify_single (merkle/src/lib.rs:800-812)."""
        ix = np.ascontiguousarray(indices, dtype=np.uint64); lv = _arr(leaves)
        buf = (C.c_uint8 * max(1, len(proof))).from_buffer_copy(proof or b"\0"); ok = C.c_int32(0)
        self._chk(self.lib.stark_merkle_verify_many_ds(self.h, cfg.arity, cfg.tree_label, _ptr(_arr(root)), _ptr(ix), len(ix), _ptr(lv), buf, len(proof), C.byref(ok)))
        return bool(ok.value)

    def merkle_verify_pairs(self, cfg, root, indices, f_vals, cp_vals, proof: bytes) -> bool:
        """MerkleProver::verify_pairs (merkle/src/lib.rs:841-855)."""
        ix = np.ascontiguousarray(indices, dtype=np.uint64); f, cp = _arr(f_vals), _arr(cp_vals)
        buf = (C.c_uint8 * max(1, len(proof))).from_buffer_copy(proof or b"\0"); ok = C.c_int32(0)
        self._chk(self.lib.stark_merkle_verify_pairs_ds(self.h, cfg.arity, cfg.tree_label, _ptr(_arr(root)), _ptr(ix), len(ix), _ptr(f), _ptr(cp), buf, len(proof), C.byref(ok)))
        return bool(ok.value)

    # ---- sum-check consumer (channel/src/lib.rs:1045-1240) ------------------------------------------------
    def commitment_commit(self, ds_tag, leaves):
        """MerkleCommitment::new(MerkleConfig::with_default_params(ds_tag)).commit(leaves) -> (root, tree) (commitment/src/lib.rs:85-90)."""
        lv = _arr(leaves); h = C.c_void_p()
        self._chk(self.lib.stark_commitment_commit(self.h, ds_tag, _ptr(lv), lv.shape[0] if lv.size else 0, C.byref(h)))
        t = MerkleTree(self, h, MerkleChannelCfg(16, None, ds_tag))
        return t.root(), t

    def commitment_verify(self, ds_tag, root, indices, values, proof: bytes) -> bool:
        """CommitmentScheme::verify (commitment/src/lib.rs:96-113)."""
        ix = np.ascontiguousarray(indices, dtype=np.uint64); v = _arr(values)
        buf = (C.c_uint8 * max(1, len(proof))).from_buffer_copy(proof or b"\0"); ok = C.c_int32(0)
        self._chk(self.lib.stark_commitment_verify(self.h, ds_tag, _ptr(_arr(root)), _ptr(ix), len(ix), _ptr(v), buf, len(proof), C.byref(ok)))
        return bool(ok.value)

    def mle_evaluate(self, table, r):
        """Mle::new(table).evaluate(r) (channel/src/lib.rs:279-295)."""
        t, rr = _arr(table), _arr(r).reshape(-1, 4); out = np.zeros(4, np.uint64)
        if t.shape[0] != 1 << rr.shape[0]:
            raise StarkError(-1, "dimension mismatch")
        self._chk(self.lib.stark_mle_evaluate(self.h, _ptr(t), rr.shape[0], _ptr(rr), _ptr(out)))
        return out

    def mle_evaluate_dev(self, table, k, r, out):
        """Mle::evaluate of the DEVICE table `table` (int, 2^k elements) at the host point r (k, 4) into the DEVICE element `out` (int);
        stream-ordered, no synchronisation (stark_mle_evaluate_dev)."""
        rr = _arr(r).reshape(-1, 4)
        if rr.shape[0] != k:
            raise StarkError(-1, "dimension mismatch")
        self._chk(self.lib.stark_mle_evaluate_dev(self.h, C.c_void_p(int(table)), k, _ptr(rr) if k else None, C.c_void_p(int(out))))

    def mle_evaluate_batch_dev(self, tables, k, r, out):
        """Mle::evaluate of each of the DEVICE tables `tables` (ints, 2^k elements each; a table may repeat) at its own host point r[i] ((B, k, 4)) into
        the DEVICE vector `out` (int, B elements), a few launches for the whole batch; stream-ordered, no synchronisation (stark_mle_evaluate_batch_dev)."""
        B = len(tables)
        rr = _arr(r).reshape(-1, 4)
        if rr.shape[0] != B * k:
            raise StarkError(-1, "dimension mismatch")
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in tables])
        self._chk(self.lib.stark_mle_evaluate_batch_dev(self.h, B, tab, k, _ptr(rr) if B * k else None, C.c_void_p(int(out))))

    def lagrange_eval_on_h(self, values, z, omega=None):
        """lagrange_eval_on_h(values, z, omega) (deep_ali/src/lib.rs:17-45): host column of n = 2^k elements, host point -> the value as 4 limbs;
        omega None = the radix-2 generator of size n."""
        v = _arr(values); out = np.zeros(4, np.uint64)
        self._chk(self.lib.stark_lagrange_eval_on_h(self.h, _ptr(v), v.shape[0], _ptr(_arr(z)), _ptr(None if omega is None else _arr(omega)), _ptr(out)))
        return out

    def lagrange_eval_on_h_dev(self, values, n, z, out, omega=None):
        """lagrange_eval_on_h of the DEVICE column `values` (int, n elements) at the host point z into the DEVICE element `out` (int);
        stream-ordered, no synchronisation (stark_lagrange_eval_on_h_dev)."""
        self._chk(self.lib.stark_lagrange_eval_on_h_dev(self.h, C.c_void_p(int(values)), n, _ptr(_arr(z)), _ptr(None if omega is None else _arr(omega)), C.c_void_p(int(out))))

    def lagrange_eval_on_h_batch_dev(self, cols, n, zs, out, omega=None):
        """lagrange_eval_on_h of each of the DEVICE columns `cols` (ints, n elements each; a column may repeat) at each of the host points zs ((P, 4)) into
        the DEVICE array `out` (int, P x len(cols) elements, point-major), one batch inversion per point for all columns; stream-ordered, no
        synchronisation (stark_lagrange_eval_on_h_batch_dev)."""
        B = len(cols); z = _arr(zs).reshape(-1, 4)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in cols])
        self._chk(self.lib.stark_lagrange_eval_on_h_batch_dev(self.h, B, tab, n, _ptr(None if omega is None else _arr(omega)), z.shape[0], _ptr(z) if z.shape[0] else None, C.c_void_p(int(out))))

    def lagrange_eval_shard_dev(self, cols, n_local, j0, n_global, zs, partials_out, omega=None):
        """The block form of lagrange_eval_on_h: `cols` (ints) are the DEVICE rows [j0, j0 + n_local) of each column of an n_global-point domain; the
        block's unscaled shares at the host points zs ((P, 4)) go into the DEVICE array `partials_out` (int, P x len(cols) elements, point-major);
        stream-ordered, no synchronisation (stark_lagrange_eval_shard_dev)."""
        B = len(cols); z = _arr(zs).reshape(-1, 4)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in cols])
        self._chk(self.lib.stark_lagrange_eval_shard_dev(self.h, B, tab, n_local, j0, n_global, _ptr(None if omega is None else _arr(omega)), z.shape[0], _ptr(z) if z.shape[0] else None,
                                                         C.c_void_p(int(partials_out))))

    def lagrange_eval_from_partials_dev(self, nparts, partials, ncols, n_global, zs, out, omega=None):
        """The combine of `nparts` block shares (DEVICE `partials`, int, nparts x P x ncols elements) into the DEVICE array `out` (int, P x ncols): the
        bytes of lagrange_eval_on_h_batch_dev on the whole columns when the blocks tile the domain; stream-ordered, no synchronisation
        (stark_lagrange_eval_from_partials_dev)."""
        z = _arr(zs).reshape(-1, 4)
        self._chk(self.lib.stark_lagrange_eval_from_partials_dev(self.h, nparts, C.c_void_p(int(partials)), ncols, n_global, _ptr(None if omega is None else _arr(omega)), z.shape[0],
                                                                 _ptr(z) if z.shape[0] else None, C.c_void_p(int(out))))

    def lagrange_eval_on_h_sharded(self, cols_block, n_global, zs, out, omega=None):
        """Collective: lagrange_eval_on_h of columns block-sharded over the context's communicator (one rank without it); cols_block (ints) = this
        rank's DEVICE rows of each column, `out` (int, DEVICE, P x len(cols_block)) = the full result on every rank
        (stark_lagrange_eval_on_h_sharded_dev)."""
        B = len(cols_block); z = _arr(zs).reshape(-1, 4)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in cols_block])
        self._chk(self.lib.stark_lagrange_eval_on_h_sharded_dev(self.h, B, tab, n_global, _ptr(None if omega is None else _arr(omega)), z.shape[0], _ptr(z) if z.shape[0] else None,
                                                                C.c_void_p(int(out))))

    def diag_lagrange_eval_sharded_emulated(self, nranks, cols_whole, n_global, zs, out, omega=None):
        """Diagnostic: the sharded lagrange_eval_on_h for `nranks` virtual ranks on this GPU (collectives as device copies) over the WHOLE DEVICE columns
        (ints); `out` (int, DEVICE, nranks x P x len(cols_whole)) = the result as every virtual rank sees it
        (stark_diag_lagrange_eval_sharded_emulated_dev)."""
        B = len(cols_whole); z = _arr(zs).reshape(-1, 4)
        tab = (C.c_void_p * max(B, 1))(*[int(x) for x in cols_whole])
        self._chk(self.lib.stark_diag_lagrange_eval_sharded_emulated_dev(self.h, nranks, B, tab, n_global, _ptr(None if omega is None else _arr(omega)), z.shape[0],
                                                                         _ptr(z) if z.shape[0] else None, C.c_void_p(int(out))))

    def prove_plain(self, k, tree_label, witness):
        """prove_plain(&build_vk_plain(k, F::from(tree_label)), witness) -> bincode-layout ProofPlain bytes."""
        w = _arr(witness); h = C.c_void_p()
        if w.shape[0] != 1 << k:
            raise StarkError(-1, "MLE length must be 2^k")
        self._chk(self.lib.stark_sumcheck_prove_plain(self.h, _ptr(w), k, tree_label, C.byref(h)))
        return self._proof_out(h)[0]

    def verify_plain(self, k, tree_label, proof: bytes) -> bool:
        buf = (C.c_uint8 * max(1, len(proof))).from_buffer_copy(proof or b"\0"); ok = C.c_int32(0)
        self._chk(self.lib.stark_sumcheck_verify_plain(self.h, k, tree_label, buf, len(proof), C.byref(ok)))
        return bool(ok.value)

    def prove_mf(self, k, tree_label, queries_per_round, witness):
        """prove_mf(&build_vk_mf(k, F::from(tree_label), q), witness) -> bincode-layout ProofMF bytes."""
        w = _arr(witness); h = C.c_void_p()
        if w.shape[0] != 1 << k:
            raise StarkError(-1, "MLE length must be 2^k")
        self._chk(self.lib.stark_sumcheck_prove_mf(self.h, _ptr(w), k, tree_label, queries_per_round, C.byref(h)))
        return self._proof_out(h)[0]

    def verify_mf(self, k, tree_label, queries_per_round, proof: bytes) -> bool:
        buf = (C.c_uint8 * max(1, len(proof))).from_buffer_copy(proof or b"\0"); ok = C.c_int32(0)
        self._chk(self.lib.stark_sumcheck_verify_mf(self.h, k, tree_label, queries_per_round, buf, len(proof), C.byref(ok)))
        return bool(ok.value)

    def verify_plain_batch(self, k, tree_labels, proofs) -> list:
        """verify_plain on each of `proofs` in one device pass (stark_sumcheck_verify_plain_batch); one bool per proof, each equal to
        verify_plain of that proof alone.  Neither k nor the labels are read (tree_labels may be None)."""
        return self._sumcheck_verify_batch(0, k, tree_labels, 0, proofs)

    def verify_mf_batch(self, k, tree_labels, queries_per_round, proofs) -> list:
        """verify_mf on each of `proofs` under tree_labels[i] in one device pass (stark_sumcheck_verify_mf_batch); one bool per proof."""
        return self._sumcheck_verify_batch(1, k, tree_labels, queries_per_round, proofs)

    def _sumcheck_verify_batch(self, mf, k, tree_labels, q, proofs):
        n = len(proofs)
        if (mf or tree_labels is not None) and len(tree_labels) != n:
            raise StarkError(-1, "one tree label per proof")
        if n == 0:
            return []
        bufs = [(C.c_uint8 * max(1, len(p))).from_buffer_copy(bytes(p) or b"\0") for p in proofs]
        ptrs = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
        lens = (C.c_size_t * n)(*[len(p) for p in proofs])
        lab = None if tree_labels is None else np.ascontiguousarray(tree_labels, dtype=np.uint64)
        acc = (C.c_int32 * n)()
        if mf:
            self._chk(self.lib.stark_sumcheck_verify_mf_batch(self.h, n, ptrs, lens, k, _ptr(lab), q, acc))
        else:
            self._chk(self.lib.stark_sumcheck_verify_plain_batch(self.h, n, ptrs, lens, k, None if lab is None else _ptr(lab), acc))
        return [bool(acc[i]) for i in range(n)]

    def prove_plain_batch_dev(self, k, tree_labels, witness_ptrs) -> list:
        """prove_plain of each witness (DEVICE pointers, ints, of 2^k elements; tree_labels[i] its VK tree label) in one pass
        (stark_sumcheck_prove_plain_batch_dev) -> list of proof bytes, each equal to prove_plain of that witness alone."""
        return self._sumcheck_batch(0, k, tree_labels, 0, witness_ptrs)

    def prove_mf_batch_dev(self, k, tree_labels, queries_per_round, witness_ptrs) -> list:
        """prove_mf of each witness in one pass (stark_sumcheck_prove_mf_batch_dev) -> list of proof bytes."""
        return self._sumcheck_batch(1, k, tree_labels, queries_per_round, witness_ptrs)

    def prove_plain_mixed_batch_dev(self, ks, tree_labels, witness_ptrs) -> list:
        """prove_plain of witnesses of different sizes (DEVICE pointers; witness i has 2^ks[i] elements) in one pass of max(ks) steps
        (stark_sumcheck_prove_plain_mixed_batch_dev) -> list of proof bytes, each equal to prove_plain of that witness alone."""
        return self._sumcheck_batch(0, list(ks), tree_labels, 0, witness_ptrs)

    def prove_mf_mixed_batch_dev(self, ks, tree_labels, queries_per_round, witness_ptrs) -> list:
        """prove_mf of witnesses of different sizes in one pass (stark_sumcheck_prove_mf_mixed_batch_dev) -> list of proof bytes."""
        return self._sumcheck_batch(1, list(ks), tree_labels, queries_per_round, witness_ptrs)

    def _sumcheck_batch(self, mf, k, tree_labels, q, witness_ptrs):
        B = len(witness_ptrs)
        if len(tree_labels) != B or (isinstance(k, list) and len(k) != B):
            raise StarkError(-1, "one tree label (and one k) per witness")
        if B == 0:
            return []
        w = (C.c_void_p * B)(*[None if p is None else int(p) for p in witness_ptrs])
        lab = np.ascontiguousarray(tree_labels, dtype=np.uint64)
        out = (C.c_void_p * B)()
        if isinstance(k, list):                                            # a k per witness: the mixed-size entry points
            kk = (C.c_size_t * B)(*[int(x) for x in k])
            if mf:
                self._chk(self.lib.stark_sumcheck_prove_mf_mixed_batch_dev(self.h, B, w, kk, _ptr(lab), q, out))
            else:
                self._chk(self.lib.stark_sumcheck_prove_plain_mixed_batch_dev(self.h, B, w, kk, _ptr(lab), out))
        elif mf:
            self._chk(self.lib.stark_sumcheck_prove_mf_batch_dev(self.h, B, w, k, _ptr(lab), q, out))
        else:
            self._chk(self.lib.stark_sumcheck_prove_plain_batch_dev(self.h, B, w, k, _ptr(lab), out))
        res = []
        for p in range(B):
            res.append(self._proof_out(C.c_void_p(out[p]))[0])
        return res

    def _proof_out(self, h):
        try:
            ln = self.lib.stark_proof_len(h)
            buf = (C.c_uint8 * ln)()
            self._chk(self.lib.stark_proof_bytes(h, buf))
            est = self.lib.stark_proof_size_estimate(h)
        finally:
            self.lib.stark_proof_free(h)
        return bytes(buf), est

    # ---- one trace sharded over several GPUs: the pieces stark_mlwe_amd.dist composes ----------------------
    def ali_challenges(self, digests, n0):
        """(seed, z, beta) of DeepAliRealBuilder::build_f0 from the four column digests (fri.rs:551-560)."""
        d = _arr(digests)
        aux = np.zeros((3, 4), np.uint64)
        self._chk(self.lib.stark_ali_challenges(self.h, _ptr(d), n0, _ptr(aux)))
        return aux

    def fri_query_plan(self, roots, n0, schedule, r):
        """Query plan of deep_fri_prove over roots only (fri.rs:355-466): FriQueryPlan with .requests()."""
        rt = _arr(roots)
        sch = np.ascontiguousarray(schedule, dtype=np.uint64)
        h = C.c_void_p()
        self._chk(self.lib.stark_fri_plan_create(self.h, _ptr(rt), n0, _ptr(sch), len(sch), r, C.byref(h)))
        return FriQueryPlan(self, h)

    def fri_build_sharded(self, f0_block, n0, schedule, seed_z):
        """Collective: the commit phase of one trace block-sharded over the context's communicator (one rank without it); f0_block =
        this rank's DEVICE block of n0 / W elements.  -> FriShardState."""
        sch = np.ascontiguousarray(schedule, dtype=np.uint64)
        h = C.c_void_p()
        self._chk(self.lib.stark_fri_build_sharded_dev(self.h, _dptr(f0_block), n0, _ptr(sch), len(sch), seed_z, C.byref(h)))
        return FriShardState(self, h, schedule)

    def deep_fri_prove_sharded(self, a, s, e, t, n0, params: DeepFriParams, f0=None):
        """Collective: deep_fri_prove (fri.rs:601-641) of one trace block-sharded over the context's communicator; a, s, e, t (or f0) =
        this rank's DEVICE blocks.  -> (canonical proof bytes, size estimate, stage ms), the same bytes on every rank."""
        sch = np.ascontiguousarray(params.schedule, dtype=np.uint64)
        h = C.c_void_p()
        self._chk(self.lib.stark_deep_fri_prove_sharded_dev(self.h, _dptr(a), _dptr(s), _dptr(e), _dptr(t), _dptr(f0), n0, _ptr(sch), len(sch),
                                                            params.r, params.seed_z, C.byref(h)))
        ms = [self.lib.stark_proof_stage_ms(h, i) for i in range(3)]
        return self._proof_out(h) + (ms,)

    def diag_fri_build_sharded_emulated(self, nranks, f0_whole, n0, schedule, seed_z):
        """Diagnostic: the sharded commit phase for `nranks` virtual ranks on this GPU (collectives as device copies) over the WHOLE f0 (device).
        -> roots as every virtual rank sees them, uint64 [nranks, L+1, 4]."""
        sch = np.ascontiguousarray(schedule, dtype=np.uint64)
        roots = np.zeros((nranks, len(sch) + 1, 4), np.uint64)
        self._chk(self.lib.stark_diag_fri_build_sharded_emulated_dev(self.h, nranks, _dptr(f0_whole), n0, _ptr(sch), len(sch), seed_z, _ptr(roots)))
        return roots

    def diag_deep_fri_prove_sharded_emulated(self, nranks, a, s, e, t, n0, params: DeepFriParams, f0=None):
        """Diagnostic: the sharded deep_fri_prove for `nranks` virtual ranks on this GPU over the WHOLE columns (device).
        -> one (proof bytes, size estimate) per virtual rank."""
        sch = np.ascontiguousarray(params.schedule, dtype=np.uint64)
        out = (C.c_void_p * nranks)()
        self._chk(self.lib.stark_diag_deep_fri_prove_sharded_emulated_dev(self.h, nranks, _dptr(a), _dptr(s), _dptr(e), _dptr(t), _dptr(f0), n0, _ptr(sch), len(sch),
                                                                          params.r, params.seed_z, out))
        return [self._proof_out(C.c_void_p(out[q])) for q in range(nranks)]

    # ---- field helpers (crates/field/src/lib.rs) ----------------------------------------------------------
    def compute_powers(self, base, n, field=PALLAS_FR):
        """compute_powers(base, n) (field/src/lib.rs:125-133)."""
        out = np.zeros((n, 4), np.uint64)
        self._chk(self.lib.stark_compute_powers(self.h, field, _ptr(_arr(base)), n, _ptr(out)))
        return out

    def domain(self, log_n, field=PALLAS_FR, precompute=False):
        """Domain::new(log_n) (field/src/lib.rs:43-53): (size, log_n, omega[, elements])."""
        w = root_of_unity(log_n, field)
        return (1 << log_n, log_n, w, self.compute_powers(w, 1 << log_n, field) if precompute else None)

    # ---- fft (crates/fft/src/lib.rs:6-32) ------------------------------------------------------------
    def fft(self, coeffs, field=BLS12_381_FR, coset=None):
        v = _arr(coeffs).copy()
        log_n = int(v.shape[0]).bit_length() - 1
        if (1 << log_n) != v.shape[0]:
            raise StarkError(-1, "radix-2 domain size must be a power of two")
        self._chk(self.lib.stark_ntt(self.h, field, _ptr(v), log_n, 0, _ptr(None if coset is None else _arr(coset))))
        return v

    def ifft(self, evals, field=BLS12_381_FR, coset=None):
        v = _arr(evals).copy()
        log_n = int(v.shape[0]).bit_length() - 1
        if (1 << log_n) != v.shape[0]:
            raise StarkError(-1, "radix-2 domain size must be a power of two")
        self._chk(self.lib.stark_ntt(self.h, field, _ptr(v), log_n, 1, _ptr(None if coset is None else _arr(coset))))
        return v

    fft_in_place, ifft_in_place = fft, ifft

    def lde(self, evals, log_blowup, field=PALLAS_FR, coset=None):
        v = _arr(evals)
        log_n = int(v.shape[0]).bit_length() - 1
        if log_n < 0 or (1 << log_n) != v.shape[0]:
            raise StarkError(-1, "radix-2 domain size must be a power of two")
        out = np.zeros((v.shape[0] << log_blowup, 4), np.uint64)
        self._chk(self.lib.stark_lde(self.h, field, _ptr(v), log_n, log_blowup, _ptr(None if coset is None else _arr(coset)), _ptr(out)))
        return out
