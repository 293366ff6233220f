/* include/stark_mlwe.h — C-ABI of libstark_mlwe_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for the proving hot path of saholmes/stark-mlwe.  The reference has no FFI
 * seam of its own (100 % safe Rust); these entry points sit BENEATH the Rust signatures listed in
 * SURVEY.md §8(b), which stay unchanged.  Each declaration cites the reference item it replaces
 * (paths relative to the reference checkout).  INTEGRATION.md shows the Rust `extern "C"` block and
 * the wrappers a maintainer adds.
 *
 * Conventions
 *   - A field element is 4 little-endian uint64_t limbs in Montgomery form (R = 2^256): exactly the
 *     in-memory layout of ark-ff `Fp<MontBackend<_,4>,4>`, so `&[F]` <-> `const uint64_t*` is zero-copy.
 *   - Plain-named functions take HOST pointers (what a Rust slice hands over) and return when the
 *     result is in the caller's buffer.  A plain-named function returns, with any status, only after the
 *     device has finished reading the caller's arrays.  `*_dev` variants take DEVICE pointers obtained from
 *     stark_malloc (or any hipMalloc'd / torch CUDA memory) and are stream-ordered on the context's
 *     stream; call stark_ctx_sync before reading results on the host.
 *   - Every function returns a status: 0 = OK, negative = error class.  stark_last_error() gives text.
 *     The Rust wrappers turn non-zero into panic!, matching the reference's assert!/panic! behaviour
 *     (fri.rs:86-87, merkle/src/lib.rs:148,161).
 *   - One context may be used by one host thread at a time; distinct contexts are independent (every
 *     entry point makes its context's device current, so one process may hold contexts on several GPUs).
 *   - Stream rule: all work of a context is enqueued on ONE stream, chosen at stark_ctx_create.  A caller
 *     that produces inputs or consumes outputs with its own kernels (torch, hipMemcpyAsync, ...) must do
 *     so on that same stream, or on a stream that is ordered against it.  Passing NULL selects the
 *     device's legacy default stream, which HIP orders against every blocking stream — including the
 *     default stream torch uses — so the NULL context is safe next to default-stream callers without
 *     manual synchronisation.  STARK_STREAM_PRIVATE asks for a private non-blocking stream instead:
 *     fastest in isolation, but then the CALLER brackets its own device work with stark_ctx_sync.
 *   - There is NO CPU fallback: without a usable HIP device every compute entry point fails with
 *     STARK_ERR_HIP.
 */
#ifndef STARK_MLWE_H
#define STARK_MLWE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STARK_OK               0
#define STARK_ERR_INVALID_ARG (-1)
#define STARK_ERR_HIP         (-2)
#define STARK_ERR_RCCL        (-3)
#define STARK_ERR_OOM         (-4)
#define STARK_ERR_UNSUPPORTED (-5)

#define STARK_FIELD_PALLAS_FR    0   /* crates/field/src/lib.rs:13  (the prover field)        */
#define STARK_FIELD_BLS12_381_FR 1   /* crates/fft/src/lib.rs:1     (the `fft` crate's field) */

typedef struct stark_ctx stark_ctx_t;
typedef struct stark_params stark_params_t;
typedef struct stark_tree stark_tree_t;
typedef struct stark_fri_state stark_fri_state_t;
typedef struct stark_proof stark_proof_t;
typedef struct stark_fri_plan stark_fri_plan_t;
typedef struct stark_transcript stark_transcript_t;
typedef struct stark_fri_shard stark_fri_shard_t;

/* ---- context / memory ------------------------------------------------------------------------- */
int32_t stark_version(void);
/* device: HIP device ordinal.  stream: the hipStream_t to run on (e.g. torch's current stream);
 * NULL = the legacy default stream; STARK_STREAM_PRIVATE = a private non-blocking stream (see "Stream rule").
 * (SURVEY.md §8(b) sketched `stark_ctx_create(devices, ndev)`: this build runs one process per GPU, so a
 * context is one device; the communicator that spans the GPUs is stark_comm_* below.) */
#define STARK_STREAM_PRIVATE ((void*)(intptr_t)-1)
int32_t stark_ctx_create(int32_t device, void* stream, stark_ctx_t** out);
/* Lifetime: every handle made from a context (stark_tree_t, stark_fri_state_t, stark_fri_plan_t, stark_transcript_t, a stark_params_t returned
 * to the caller) keeps the context alive.  stark_ctx_destroy with such handles outstanding synchronises, marks the context and returns
 * STARK_OK; the handles stay fully usable and the last one freed releases the context's resources.  Device pointers obtained FROM a handle
 * (stark_merkle_level_dev, layers of a FRI state) are valid for work ordered on the context's stream until the handle is freed: freeing
 * returns the block to the context's pool without a device synchronisation, so a caller that read it on ANOTHER stream synchronises first. */
int32_t stark_ctx_destroy(stark_ctx_t* ctx);
int32_t stark_ctx_sync(stark_ctx_t* ctx);
/* The library keeps released temporaries / layers / tree levels in a per-context cache (no hipMalloc /
 * hipFree on the hot path).  trim hands the cached blocks back to the driver. */
int32_t stark_ctx_trim(stark_ctx_t* ctx);     /* also drops the NTT plans (direct twiddle tables) and the NTT scratch vector */
/* Tuning / diagnostic options — explicit state of the context, never read from the environment:
 *   "ntt_direct_max_log" (default 24: one-product twiddle tables up to 2^24 points; 0 = always the two-level lookup),
 *   "ntt_merged_coset" (default 1: a coset transform's pre-scale is folded into its first pass's twiddle table; 0 = separate tables),
 *   "ntt_log_tile" (8..12, default 11; -1 restores the default), "ntt_min_waves" (2 | 4), "poseidon_lane_only" (0 | 1).
 *   "sponge_one_wave" (0 | 1: long serial sponges, small Merkle levels / leaf layers and short transcript hashes on the one-wave / wave-pair kernels
 *   instead of the five-wave latency kernel; comparison), "sponge_debug" (timing experiments on the five-wave kernel; digests are WRONG when set).
 *   "prove_batch_max_rows" (1..2^28, default 2^22: the rows of one pass of the batched DEEP-FRI provers).
 *   "ntt_batch_max_elems" (1..2^28, default 2^24: the output elements of one pass of stark_ntt_batch_dev / stark_lde_batch_dev).
 *   "mle_log_tile" (3..12, default 12; -1 restores the default: the rounds one launch of stark_mle_evaluate_dev / _batch_dev folds),
 *   "mle_lane_contiguous" (0 | 1, default 0; -1 restores the default: a lane of those launches owns consecutive elements instead of interleaved ones; comparison).
 *   "lagrange_max_partials" (1..2^28, default 2^21 elements = 64 MiB; -1 restores the default: the block partials one pass of
 *   stark_lagrange_eval_on_h_batch_dev may hold; a pass of one point is always allowed),
 *   "lagrange_wide_acc" (0 | 1, default 1; -1 restores the default: a lane's products of a column go through the lazy accumulator; comparison),
 *   "lagrange_col_groups" (1..65535, default -1 = automatic; -1 restores the default: the column groups of a launch of the lagrange_eval kernel;
 *   1 = one group, g > 1 = min(g, ncols) groups; every value gives the same bytes).
 *   "lagrange_shared_inverse" (0 | 1, default 0; -1 restores the default: 1 = a pass of the lagrange_eval driver multiplies the workgroups' products,
 *   inverts those of a point together with ONE Fermat inversion and hands every workgroup its inverse, instead of one inversion per workgroup; two
 *   more launches, two pooled tables of pass points x workgroups elements, still stream-ordered and without a host synchronisation; every value
 *   gives the same bytes, errors and refusals on every stark_lagrange_eval_* entry point),
 *   "lagrange_share_cosets" (0 | 1, default 0; -1 restores the default: 1 = points of one coset of H — z and z w^s, such as the DEEP pair (z, z w), in
 *   any order, duplicates included — share the weights of the first of them and read the columns at their shift; the whole-domain calls only: the
 *   block forms (stark_lagrange_eval_shard_dev, the sharded and emulated calls) ignore it, because a rotation leaves the block; every value gives
 *   the same bytes).
 *   "mixed_prove_tail" (0 | 1, default 0; -1 restores the default: stark_deep_fri_prove_mixed_batch_dev runs the tail — merge, commit phase, query phase —
 *   once per group of equal (n0, schedule, r) (0) or once per class of equal schedule, whatever the n0 and r in it (1: the ragged tail); every value gives
 *   the same bytes).
 *   "pool_poison" (0..255, default -1 = off; FOR TESTS ONLY: every pooled block the library hands to itself, recycled or fresh, and the NTT scratch vector are
 *   filled with this byte first, so a result that depends on a temporary nobody wrote changes with the byte.  Each fill synchronises the stream: the
 *   calls that promise "no synchronisation" do synchronise while it is set.  The long-lived tables are not filled).
 * An unknown key is STARK_ERR_INVALID_ARG; stark_last_error then lists the known keys.
 * Changing an option synchronises the stream and drops the cached NTT plans. */
int32_t stark_ctx_set_option(stark_ctx_t* ctx, const char* key, int64_t value);
size_t  stark_ctx_cached_bytes(stark_ctx_t* ctx);
/* The text of the context's last error.  One kind of SUCCESSFUL call also writes here: an NTT / LDE call that could not allocate one of its optional
 * direct tables returns STARK_OK, runs on the two-level lookup, and leaves a note that starts with "optional NTT table " (it replaces an older error
 * text).  Read the text right after the call whose status it explains. */
const char* stark_last_error(stark_ctx_t* ctx);
int32_t stark_malloc(stark_ctx_t* ctx, size_t bytes, void** dptr);
int32_t stark_free(stark_ctx_t* ctx, void* dptr);
int32_t stark_memcpy_h2d(stark_ctx_t* ctx, void* dst_dev, const void* src_host, size_t bytes);
int32_t stark_memcpy_d2h(stark_ctx_t* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* Diagnostic: lane-level v_mad_u64_u32 (32x32+64 multiply-accumulate) issue rate of this device, measured live with every
 * SIMD saturated — the roofline `peak` of the integer-VALU-bound Poseidon kernels (bench.py "poseidon.roofline"). */
int32_t stark_diag_mac_rate(stark_ctx_t* ctx, double* lane_macs_per_s);
/* Diagnostic, FOR TESTS ONLY: refuse one device allocation of the library's own, so that the error paths behind every allocation can be run
 * without exhausting a device.  An allocation REQUEST is every request for a pooled block (temporaries, layers, tree levels: served from the
 * context's cache or by hipMalloc) and every allocation of a long-lived table (NTT plans and their tables, parameter sets, transcript frames, the
 * NTT scratch vector); stark_malloc is the caller's own and is not counted.
 *   mode 1: requests are counted from 1 and request number nth fails as a real out-of-memory condition does (the call returns STARK_ERR_OOM with
 *           every output handle NULL, or degrades where a table is optional); nth = 0 counts without refusing.
 *   mode 2: the requests the cache could not serve are counted, and for number nth the FIRST hipMalloc attempt is refused: the library hands its
 *           cached blocks back to the driver, tries again and the call succeeds.
 *   mode 3: as mode 2 with the second attempt refused as well: the cached blocks are handed back and the request still fails (STARK_ERR_OOM).
 *   mode 0: off, the default (counting stops).   mode -1: read the numbers, change nothing.
 * A hook that fired disarms itself and goes on counting.  stats (NULL, or FIVE words) receives, BEFORE the new mode is applied: the requests counted
 * since the last arming, the refusals fired since then, the pooled blocks currently held by handles and calls, their bytes, and the cached bytes the
 * library's accounting showed right after its last hand-back of the cache since the arming (all ones: none happened).  Neither
 * synchronises nor drops the NTT plans (stark_ctx_set_option does both). */
int32_t stark_diag_alloc_refusal(stark_ctx_t* ctx, int32_t mode, uint64_t nth, uint64_t* stats);
/* HIP-event timing on the context's stream (bench.py measures kernels with these). */
int32_t stark_timer_start(stark_ctx_t* ctx);
int32_t stark_timer_stop_ms(stark_ctx_t* ctx, float* ms);

/* ---- Poseidon constants -------------------------------------------------------------------------
 * PoseidonParams / PoseidonParamsDynamic (poseidon/src/lib.rs:16-21, 104-114).  Constants are passed
 * in as the Rust side derived them (row-major mds[i][j], rc_full[r][i], rc_partial[r]); the library
 * turns them into kernel form (LU factors, sparse partial-round matrices).  t in {9,17,33,65,129}. */
int32_t stark_poseidon_params_upload(stark_ctx_t* ctx, int32_t t, int32_t rf, int32_t rp, const uint64_t* mds,
                                     const uint64_t* rc_full, const uint64_t* rc_partial, stark_params_t** out);
/* Same derivations done inside the library (BLAKE3, utils/src/lib.rs:16-22):
 *   for_width:  poseidon_params_for_width(t)                        poseidon/src/lib.rs:120-146
 *   t17_seed :  params::generate_params_t17_x5(seed)                poseidon/src/lib.rs:318-356
 *               (seed "POSEIDON-T17-X5-TRANSCRIPT" = transcript::default_params, transcript/src/lib.rs:44-46) */
int32_t stark_poseidon_params_for_width(stark_ctx_t* ctx, int32_t t, stark_params_t** out);
int32_t stark_poseidon_params_t17_seed(stark_ctx_t* ctx, const uint8_t* seed, size_t seed_len, stark_params_t** out);
int32_t stark_poseidon_params_export(stark_params_t* p, int32_t* t, int32_t* rf, int32_t* rp, uint64_t* mds, uint64_t* rc_full, uint64_t* rc_partial);
int32_t stark_poseidon_params_free(stark_params_t* p);

/* ---- Poseidon ------------------------------------------------------------------------------------ */
/* permute / permute_dynamic (poseidon/src/lib.rs:31, 219): nstates states of t elements, in place. */
int32_t stark_poseidon_permute_batch(stark_ctx_t* ctx, stark_params_t* p, uint64_t* states, size_t nstates);
int32_t stark_poseidon_permute_batch_dev(stark_ctx_t* ctx, stark_params_t* p, uint64_t* states, size_t nstates);
/* hash_with_ds_dynamic (poseidon/src/lib.rs:288-312) over a batch: hash k absorbs
 * ds_fields[k*nds .. +nds] then inputs[k*cnt .. +cnt], pad 1||0*, squeezes state[0]. */
int32_t stark_poseidon_hash_with_ds_dynamic(stark_ctx_t* ctx, stark_params_t* p, const uint64_t* ds_fields, size_t nds,
                                            const uint64_t* inputs, size_t cnt, size_t n, uint64_t* out);
/* hash_with_ds (legacy, poseidon/src/lib.rs:85-100): t = 17, ds_tag in the capacity lane, no padding. */
int32_t stark_poseidon_hash_with_ds(stark_ctx_t* ctx, stark_params_t* p, const uint64_t* inputs, size_t cnt, const uint64_t* ds_tag, uint64_t* out);
/* One Merkle level: out[k] = hash_with_ds_dynamic([arity, level, pos0+k, tree_label], in[k*arity ..])
 * (merkle/src/lib.rs:167-176); the last chunk may be short. */
int32_t stark_poseidon_hash_ds_batch(stark_ctx_t* ctx, stark_params_t* p, size_t arity, uint32_t level, uint64_t pos0, uint64_t tree_label,
                                     const uint64_t* in, size_t n_in, uint64_t* out);
int32_t stark_poseidon_hash_ds_batch_dev(stark_ctx_t* ctx, stark_params_t* p, size_t arity, uint32_t level, uint64_t pos0, uint64_t tree_label,
                                         const uint64_t* in, size_t n_in, uint64_t* out);
/* hash_leaf_pair over a layer (fri.rs:38-44 as used at fri.rs:283): h[i] = hash_leaf_pair(f[i], s_i),
 * s_i = f_next[i / m], or zero when f_next == NULL (fri.rs:266).  tparams = transcript params (t=17). */
int32_t stark_leaf_pair_hash(stark_ctx_t* ctx, stark_params_t* tparams, const uint64_t* f, const uint64_t* f_next, size_t n, size_t m, uint64_t* h);
int32_t stark_leaf_pair_hash_dev(stark_ctx_t* ctx, stark_params_t* tparams, const uint64_t* f, const uint64_t* f_next, size_t n, size_t m, uint64_t* h);
/* tr_hash_fields_tagged (fri.rs:28-35): n_hashes independent transcript hashes of k fields each. */
int32_t stark_tr_hash_fields_tagged(stark_ctx_t* ctx, stark_params_t* tparams, const char* tag, const uint64_t* fields, size_t k, size_t n_hashes, uint64_t* out);
int32_t stark_tr_hash_fields_tagged_dev(stark_ctx_t* ctx, stark_params_t* tparams, const char* tag, const uint64_t* fields, size_t k, size_t n_hashes, uint64_t* out);
/* n transcript hashes of ANY tags and lengths in one launch: out[i] = tr_hash_fields_tagged(tags[i], fields[i][0 .. k[i])) (fri.rs:28-35), byte-equal
 * to stark_tr_hash_fields_tagged_dev on item i alone.  tags: HOST array of n C strings; fields: HOST array of n DEVICE pointers (a NULL entry is
 * allowed iff k[i] == 0: such an item hashes its tag's frame alone; the table itself may be NULL when every k[i] is 0); k: HOST, n; out: DEVICE,
 * n x 4.  The sponges are independent chains and run side by side, the longest first, each digest written to its caller's slot: the call costs what
 * its longest item costs.  Stream-ordered, no host synchronisation (the first use of a tag uploads its frame and synchronises, as in every
 * transcript hash).  Pointers may repeat; inputs are left intact.  n == 0 returns STARK_OK.
 * STARK_ERR_INVALID_ARG, before any launch: a null ctx, tags, k or out; a null tags[i]; a null fields table or entry with k[i] > 0; an out range
 * that overlaps an input. */
int32_t stark_tr_hash_many_dev(stark_ctx_t* ctx, size_t n, const char* const* tags, const uint64_t* const* fields, const size_t* k, uint64_t* out);

/* ---- Merkle ---------------------------------------------------------------------------------------
 * MerkleTree::new / new_pairs (merkle/src/lib.rs:147-193, 392-445): level-by-level build, all levels
 * kept resident on the device (openings read them, :261-291).  pairs != 0 => leaves are (f, cp) pairs
 * hashed with the leaf DS level 2^32-1 (:380-388).  `first_pos` / `level0` let a shard build its part
 * of a larger tree (DS positions are global): pass 0 / 0 for a whole tree. */
int32_t stark_merkle_build(stark_ctx_t* ctx, stark_params_t* p, size_t arity, uint64_t tree_label, const uint64_t* leaves, size_t n,
                           int32_t pairs, const uint64_t* cp, stark_tree_t** out);
int32_t stark_merkle_build_dev(stark_ctx_t* ctx, stark_params_t* p, size_t arity, uint64_t tree_label, const uint64_t* leaves, size_t n,
                               int32_t pairs, const uint64_t* cp, uint64_t first_pos, uint32_t level0, int32_t stop_at_len, stark_tree_t** out);
int32_t stark_merkle_num_levels(stark_tree_t* t);
size_t  stark_merkle_level_len(stark_tree_t* t, int32_t lvl);
int32_t stark_merkle_root(stark_tree_t* t, uint64_t* out4);
int32_t stark_merkle_level(stark_tree_t* t, int32_t lvl, uint64_t* out);                         /* host copy of a level */
const uint64_t* stark_merkle_level_dev(stark_tree_t* t, int32_t lvl);                           /* device pointer     */
int32_t stark_merkle_gather(stark_tree_t* t, int32_t lvl, const size_t* idx, size_t k, uint64_t* out);
/* open_union_of_paths (merkle/src/lib.rs:246-315) → canonical MerkleProof encoding (DESIGN.md
 * "Proof encoding"): call with buf == NULL to get the length. */
int32_t stark_merkle_open(stark_tree_t* t, const size_t* idx, size_t k, uint8_t* buf, size_t cap, size_t* len);
int32_t stark_merkle_free(stark_tree_t* t);

/* Many trees in one device pass.  Element i of every result equals what the single call returns for item i alone, byte for byte, and the handles
 * are ordinary stark_tree_t: every accessor above (and stark_merkle_open, stark_merkle_free) takes them, they may be freed in any order, and like
 * every handle they keep their context alive.
 *  - build: MerkleTree::new / new_pairs (merkle/src/lib.rs:147-193, 392-445) of `batch` trees of one shape (arity, n, pairs, params) — every arity
 *    and width of the single build, ragged last nodes, n = 1 (no hash: root = leaf).  Stream-ordered with no host synchronisation (the labels and
 *    pointer tables are copied before the call returns).  Level v of all trees is ONE pooled block of batch x len_v elements (tree i's level the
 *    slice at i * len_v) that goes back to the pool when the last tree of the batch is freed; level 0 is one launch (a copy, or the pair leaves read
 *    through the pointer tables) and every level above one launch whose kernel form is chosen for batch x nodes hashes.  The same pointer may appear
 *    twice; inputs are left intact.  Shard builds (first_pos / level0 / stop_at_len) have no batch form.
 *  - roots: the batch's roots with ONE download and one synchronisation (any complete trees of one context).
 *  - open: open_union_of_paths (:246-315) of every tree: tree i opens idx[idx_off[i] .. idx_off[i+1]); out[i] is a stark_proof_t whose bytes are
 *    exactly stark_merkle_open's (stark_proof_len / stark_proof_bytes).  The trees need not share a shape or come from a batch build; they share a
 *    context.  Every tree is planned on the host and all siblings come back with one gather launch, one download and one synchronisation.
 *  - verify: verify_many_ds (:587-722) over `batch` openings under one cfg_arity: item i has tree_labels[i], roots[4 i ..], the indices and values
 *    (stored form, as the single call takes them) at [idx_off[i], idx_off[i+1]) and proofs[i] / lens[i]; accepted[i] == stark_merkle_verify_many_ds on
 *    item i alone.  The host parses and plans every opening, the device runs one launch per (width, tree depth) and compares the roots: one upload,
 *    one download, one synchronisation (a plan is cut at 2^25 pool slots, so a huge batch runs as several).  An item that does not decode, fails a
 *    structural check or has no index is a rejection, never an error.  verify_pairs_ds has no batch form.
 * batch == 0 returns STARK_OK.  STARK_ERR_INVALID_ARG, before any launch: a null ctx, params, table or out / accepted; a null leaves[i] or trees[i];
 * pairs without a cp table; n == 0; an arity incompatible with the parameter width; a non-monotone idx_off; (open) an empty index list for a tree, as
 * open_many, or a leaf index out of range; trees of different contexts or a partial tree; batch x n above 2^31 - 1.  Arity 1 with n > 1 and (verify) a
 * cfg_arity above 128 are STARK_ERR_UNSUPPORTED, as in the single calls.  On any error every out[i] is NULL and every accepted[i] is 0. */
/* MerkleTree::new / new_pairs (merkle/src/lib.rs:147-193, 392-445) of `batch` trees of one shape (arity, n, pairs, params). */
int32_t stark_merkle_build_batch_dev(stark_ctx_t* ctx, stark_params_t* p, size_t arity, size_t batch, const uint64_t* tree_labels /* host, batch */,
                                     const uint64_t* const* leaves /* host array of batch DEVICE pointers */, size_t n, int32_t pairs,
                                     const uint64_t* const* cp /* as leaves; NULL iff !pairs; a NULL entry = zeros */, stark_tree_t** out /* host, batch handles */);
/* The same of `batch` trees of DIFFERENT lengths: tree i has n[i] >= 1 leaves (one arity, one parameter set, pairs or not for all).  out[i] equals
 * stark_merkle_build_dev of tree i alone, level by level and byte for byte.  Level v of the call is ONE pooled block, the slices of the trees that
 * have more than v levels back to back in tree order (a tree of one leaf has its one level and no hash; trees drop out as they reach their root);
 * level 0 is one launch (a ragged copy, or the pair leaves) and every level above one launch over the trees that still have it, its kernel form
 * chosen for the launch's total number of hashes.  The handles are ordinary trees that may be freed in any order; the blocks go back to the pool with
 * the last one.  Stream-ordered with no host synchronisation: n, the labels and the pointer tables may die on return.  batch == 0 returns STARK_OK.
 * STARK_ERR_INVALID_ARG, before any launch: a null ctx, params, table, n or out; a null leaves[i]; an n[i] == 0; pairs without a cp table; an arity
 * incompatible with the parameter width; a sum of n above 2^31 - 1.  Arity 1 with some n[i] > 1 is STARK_ERR_UNSUPPORTED.  On any error every out[i]
 * is NULL and stark_ctx_cached_bytes is what it was. */
int32_t stark_merkle_build_mixed_batch_dev(stark_ctx_t* ctx, stark_params_t* p, size_t arity, size_t batch, const uint64_t* tree_labels /* host, batch */,
                                           const uint64_t* const* leaves /* host array of batch DEVICE pointers */, const size_t* n /* host, batch */, int32_t pairs,
                                           const uint64_t* const* cp /* as leaves; NULL iff !pairs; a NULL entry = zeros */, stark_tree_t** out /* host, batch handles */);
/* the batch roots with ONE download (MerkleTree::root, merkle/src/lib.rs:195-197) */
int32_t stark_merkle_roots_batch(stark_tree_t* const* trees, size_t batch, uint64_t* roots /* host, batch x 4 */);
/* open_union_of_paths (merkle/src/lib.rs:246-315) of every tree: tree i opens idx[idx_off[i] .. idx_off[i+1]) */
int32_t stark_merkle_open_batch(stark_tree_t* const* trees, size_t batch, const size_t* idx, const size_t* idx_off /* batch + 1 */, stark_proof_t** out);
/* verify_many_ds (merkle/src/lib.rs:587-722) over `batch` openings; accepted[i] == stark_merkle_verify_many_ds on item i alone. */
int32_t stark_merkle_verify_many_ds_batch(stark_ctx_t* ctx, size_t cfg_arity, size_t batch, const uint64_t* tree_labels, const uint64_t* roots /* batch x 4 */,
                                          const size_t* indices, const size_t* idx_off, const uint64_t* values /* concatenated, idx_off-indexed */,
                                          const uint8_t* const* proofs, const size_t* lens, int32_t* accepted);

/* ---- FRI ------------------------------------------------------------------------------------------ */
/* fri_sample_z_ell (fri.rs:59-82). */
int32_t stark_fri_sample_z(stark_ctx_t* ctx, stark_params_t* tparams, uint64_t seed_z, size_t level, size_t domain_size, uint64_t* z4);
/* fri_fold_layer (fri.rs:85-102): out[b] = sum_{t<m} f[b*m+t] z^t, n % m == 0, m >= 2. */
int32_t stark_fri_fold(stark_ctx_t* ctx, const uint64_t* f, size_t n, const uint64_t* z4, size_t m, uint64_t* out);
int32_t stark_fri_fold_dev(stark_ctx_t* ctx, const uint64_t* f, size_t n, const uint64_t* z4, size_t m, uint64_t* out);
/* fri_build_transcript (fri.rs:231-312): all folds, per-layer leaf hashes and the L+1 trees.
 * z_l are derived inside (they depend only on (seed_z, l, size), fri.rs:250). */
int32_t stark_fri_build(stark_ctx_t* ctx, const uint64_t* f0, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, stark_fri_state_t** out);
int32_t stark_fri_build_dev(stark_ctx_t* ctx, const uint64_t* f0, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, stark_fri_state_t** out);
int32_t stark_fri_num_layers(stark_fri_state_t* s);                 /* L + 1 */
size_t  stark_fri_layer_len(stark_fri_state_t* s, int32_t layer);
int32_t stark_fri_layer_f(stark_fri_state_t* s, int32_t layer, uint64_t* out);
int32_t stark_fri_layer_root(stark_fri_state_t* s, int32_t layer, uint64_t* out4);
int32_t stark_fri_layer_z(stark_fri_state_t* s, int32_t layer, uint64_t* out4);
stark_tree_t* stark_fri_layer_tree(stark_fri_state_t* s, int32_t layer);
int32_t stark_fri_state_free(stark_fri_state_t* s);

/* ---- DEEP-ALI (next row N1) ---------------------------------------------------------------------- */
/* deep_ali_merge_evals(_blinded) (deep_ali/src/lib.rs:48-105).  r_opt / beta may be NULL.  c_star may be NULL. */
int32_t stark_ali_merge(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* r_opt,
                        const uint64_t* beta4, const uint64_t* omega4, const uint64_t* z4, size_t n, uint64_t* f0, uint64_t* c_star4);
int32_t stark_ali_merge_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* r_opt,
                            const uint64_t* beta4, const uint64_t* omega4, const uint64_t* z4, size_t n, uint64_t* f0, uint64_t* c_star4);
/* lagrange_eval_on_h(values, z, omega) (deep_ali/src/lib.rs:17-45): the value at z of the polynomial of degree < n whose evaluations on
 * H = <omega> are `values`; host pointers, the reference's signature (uploads the column, synchronises, out4 on the host). */
int32_t stark_lagrange_eval_on_h(stark_ctx_t* ctx, const uint64_t* values, size_t n, const uint64_t* z4, const uint64_t* omega4, uint64_t* out4);
/* lagrange_eval_on_h (deep_ali/src/lib.rs:17-45) of a DEVICE-resident column of n elements at the point z4 (HOST) into out4 (DEVICE, one element);
 * omega4: HOST.  The batch form below with one column and one point. */
int32_t stark_lagrange_eval_on_h_dev(stark_ctx_t* ctx, const uint64_t* values, size_t n, const uint64_t* z4, const uint64_t* omega4, uint64_t* out4);
/* lagrange_eval_on_h (deep_ali/src/lib.rs:17-45) of ncols columns at npoints points over one domain: cols is a HOST array of ncols DEVICE pointers
 * (n elements each), z the HOST array of the npoints x 4 points, out npoints x ncols elements in DEVICE memory:
 * out[p * ncols + c] = lagrange_eval_on_h(cols[c], z[p], omega), the reference's field element in stored (Montgomery, fully reduced) form and
 * byte-equal to the single call on that column and point alone.  Outside H (z^n != 1) it is (z^n - 1)/n * sum_j v[j] omega^j / (z - omega^j);
 * inside H (z = omega^j) it is v[j] itself, copied; points inside and outside H may share a call.  The weights omega^j / (z - omega^j) depend on
 * the point only: the columns of a call share one batch inversion per point.  Stream-ordered, no host synchronisation: z and the pointer table are
 * copied before the call returns.  The scratch (block partials) is bounded by cutting the points into passes ("lagrange_max_partials").
 * n is a power of two, 1 <= n <= 2^30; n = 1 gives v[0] for every z.  omega4 == NULL means the radix-2 generator of size n, as in
 * stark_ali_merge_shard_dev; a caller's omega must be a primitive n-th root of unity: the host checks omega^n = 1 and, for n >= 2,
 * omega^(n/2) = -1, so the reference's "z in domain but not matching a power of omega" panic cannot arise.  Columns may repeat and are left
 * intact.  ncols == 0 or npoints == 0 returns STARK_OK and writes nothing.  STARK_ERR_INVALID_ARG, checked on the host before anything is
 * launched: a null ctx, cols, cols[c] or out; a null z with npoints > 0; n zero, not a power of two or above 2^30; an omega that fails the
 * check above; an out range that overlaps a column.  (More than 2^24 columns in one call: STARK_ERR_UNSUPPORTED.) */
int32_t stark_lagrange_eval_on_h_batch_dev(stark_ctx_t* ctx, size_t ncols, const uint64_t* const* cols, size_t n, const uint64_t* omega4, size_t npoints,
                                           const uint64_t* z, uint64_t* out);
/* lagrange_eval_on_h (deep_ali/src/lib.rs:17-45) of columns that live as blocks: the share of the rows [j0, j0 + n_local) of an n_global-point
 * domain.  cols is a HOST array of ncols DEVICE pointers to this block's n_local rows, z the HOST array of the npoints x 4 points, partials_out
 * npoints x ncols elements in DEVICE memory, point-major.  Outside H: partials_out[p * ncols + c] = sum over the block's rows j of
 * cols[c][j] omega^(j0 + j) / (z[p] - omega^(j0 + j)), unscaled, omega the generator of the GLOBAL domain.  Inside H (z[p] = omega^(j*), classified
 * against the global domain): the row cols[c][j* - j0] when j0 <= j* < j0 + n_local, zero otherwise.  The shares of the blocks of any partition of
 * [0, n_global) go through stark_lagrange_eval_from_partials_dev.  Any block with 1 <= n_local and j0 + n_local <= n_global is accepted; n_local
 * need not be a power of two.  n_global and omega4 follow the batch call's rules (omega4 == NULL: the radix-2 generator of size n_global).
 * Stream-ordered, no host synchronisation: z and the pointer table are copied before the call returns; passes are bounded by
 * "lagrange_max_partials".  ncols == 0 or npoints == 0 returns STARK_OK and writes nothing.  STARK_ERR_INVALID_ARG, before anything is launched:
 * the batch call's causes, n_local == 0, j0 + n_local > n_global, a partials_out range that overlaps a column block. */
int32_t stark_lagrange_eval_shard_dev(stark_ctx_t* ctx, size_t ncols, const uint64_t* const* cols, size_t n_local, uint64_t j0, size_t n_global, const uint64_t* omega4,
                                      size_t npoints, const uint64_t* z, uint64_t* partials_out);
/* The combine of the block shares of lagrange_eval_on_h (deep_ali/src/lib.rs:17-45): partials is DEVICE, nparts x npoints x ncols (the
 * partials_out of nparts calls of stark_lagrange_eval_shard_dev, one after the other), out DEVICE, npoints x ncols:
 * out[p * ncols + c] = scale[p] * sum_q partials[(q * npoints + p) * ncols + c], scale = (z^n - 1)/n outside H and one inside H, computed on the
 * host from z (HOST).  When the parts tile [0, n_global), out equals stark_lagrange_eval_on_h_batch_dev on the whole columns byte for byte.
 * Stream-ordered, no host synchronisation.  STARK_ERR_INVALID_ARG: nparts == 0 with results requested, a null partials, z or out, a refused
 * (n_global, omega4), out overlapping partials. */
int32_t stark_lagrange_eval_from_partials_dev(stark_ctx_t* ctx, size_t nparts, const uint64_t* partials, size_t ncols, size_t n_global, const uint64_t* omega4, size_t npoints,
                                              const uint64_t* z, uint64_t* out);
/* lagrange_eval_on_h (deep_ali/src/lib.rs:17-45) of columns block-sharded over the context's communicator as ONE collective call (W = 1 without a
 * communicator): rank q passes its rows [q*n/W, (q+1)*n/W) of every column (cols_block: a HOST array of ncols DEVICE pointers) and EVERY rank
 * receives the full out (DEVICE, npoints x ncols), the bytes of stark_lagrange_eval_on_h_batch_dev on the whole columns.  Steps: the block
 * partials, one all-gather of the W tables of npoints x ncols elements, the combine.  All argument checks come before the first collective; the
 * first collective all-gathers a small header (n_global, ncols, npoints, a 64-bit digest of the omega and z bytes) and, when any two headers
 * differ, EVERY rank returns STARK_ERR_INVALID_ARG (the rule of stark_fri_build_sharded_dev).  W must be a power of two that divides n_global.
 *  - stark_diag_lagrange_eval_sharded_emulated_dev: the diagnostic twin (deep_ali/src/lib.rs:17-45): the same phase code for `nranks` VIRTUAL
 *    ranks on this one GPU, every collective as device copies.  cols_whole: the WHOLE columns; out: nranks x npoints x ncols, the result as every
 *    virtual rank sees it.  nranks must be a power of two that divides n_global, else STARK_ERR_INVALID_ARG.
 * STATUS: W > 1 over a real communicator has run only as the emulation, like the sharded LDE, commit and prove (no multi-GPU node was available
 * to the build). */
int32_t stark_lagrange_eval_on_h_sharded_dev(stark_ctx_t* ctx, size_t ncols, const uint64_t* const* cols_block, size_t n_global, const uint64_t* omega4, size_t npoints,
                                             const uint64_t* z, uint64_t* out);
int32_t stark_diag_lagrange_eval_sharded_emulated_dev(stark_ctx_t* ctx, int32_t nranks, size_t ncols, const uint64_t* const* cols_whole, size_t n_global, const uint64_t* omega4,
                                                      size_t npoints, const uint64_t* z, uint64_t* out);
/* DeepAliRealBuilder::build_f0 (fri.rs:535-569): 4 column sponges, (z, beta) sampling, merge.
 * aux7 (optional, host): col digests A,S,E,T, seed_f, z, beta. */
int32_t stark_build_f0(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, size_t n0, uint64_t* f0, uint64_t* aux7);
int32_t stark_build_f0_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, size_t n0, uint64_t* f0, uint64_t* aux7_host);

/* ---- end-to-end prove (next row N2) -------------------------------------------------------------- */
/* deep_fri_prove (fri.rs:601-641) with DeepAliRealBuilder::default().  If f0 != NULL the builder is
 * skipped and a,s,e,t are ignored ("prove given f0").  The proof is returned in the canonical byte
 * encoding (DESIGN.md "Proof encoding"). */
int32_t stark_deep_fri_prove(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* f0,
                             size_t n0, const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out);
int32_t stark_deep_fri_prove_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* f0,
                                 size_t n0, const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out);
/* `batch` independent traces of n0 rows each, one proof per trace (the reference's bench proves one trace after another,
 * channel/benches/end_to_end.rs:229-309).  a, s, e, t: HOST arrays of `batch` DEVICE pointers; out: host array of `batch` proof handles
 * (all NULL on failure).  The serial column sponges of build_f0 (fri.rs:548-557) bound a single prove and keep four waves of the chip
 * busy; the 4 * batch chains of a batch are independent and run in ONE launch, so the stage costs what it costs for one trace.
 * The tails (merge, commit phase, query phase) of the traces then run side by side: the batch is cut into passes of at most
 * "prove_batch_max_rows" rows (option, default 2^22; a pass of one trace is the single tail), and every step of a pass is one launch
 * for all its traces.  (The earlier tail, trace after trace on four worker contexts, has been removed together with the option that selected
 * it: stark_ctx_set_option now refuses that key as it refuses any unknown one, with STARK_ERR_INVALID_ARG.)
 * Every proof is byte-identical to stark_deep_fri_prove_dev on that trace alone.  stage_ms 0 / 1 / 2 of a proof are its pass's shared
 * stage times: the sponge stage of the whole batch + the pass's merge, the pass's commit phase, the pass's query phase.  They are HOST times
 * between the steps: in a pass of two or more traces merge and commit phase only enqueue their launches, so stages 0 and 1 count enqueueing
 * and stage 2, which holds the pass's first synchronisation, absorbs the device time of all three. */
int32_t stark_deep_fri_prove_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* a, const uint64_t* const* s, const uint64_t* const* e, const uint64_t* const* t,
                                       size_t n0, const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out);
/* `batch` independent traces of ANY shapes in one call: trace i has n0[i] rows, folds by schedule[sched_off[i] .. sched_off[i + 1]) and answers r[i]
 * queries (the reference's bench proves k = 11, 12, .. 18 one after another, channel/benches/end_to_end.rs:229-309).  a, s, e, t: HOST arrays of
 * `batch` DEVICE pointers; n0, r: HOST, batch; sched_off: HOST, batch + 1, non-decreasing; out: host array of `batch` proof handles.
 * The 4 * batch column sponges of build_f0 run in ONE launch whatever their lengths (longest first), so the stage that bounds a prove costs what
 * the largest trace's costs instead of the sum over the traces.  Traces of equal (n0, schedule, r) then form a group — groups in order of first
 * appearance, traces in the caller's order — and each group takes the tail of stark_deep_fri_prove_batch_dev: passes of at most
 * "prove_batch_max_rows" rows, a pass of one trace the single tail.
 * Under the option "mixed_prove_tail" = 1 the traces of equal SCHEDULE (same L, same entries; n0 and r free) form a class instead — classes in order of
 * first appearance, traces in the caller's order — and a class is cut into passes of consecutive traces whose n0 sum to at most "prove_batch_max_rows"
 * (at least one trace a pass; a pass of one trace is the single tail).  A pass runs ONE merge launch, one commit phase (one fold launch per layer over
 * all its traces, one leaf launch and one launch per tree level per layer) and one query phase with four host synchronisations, whatever the sizes
 * and query counts in it.  Results, stage times, errors and everything below are the same under either value.
 * Proof i is byte-identical to stark_deep_fri_prove_dev on trace i alone under (n0[i], its schedule, r[i]).  stage_ms 0 of a proof is the sponge
 * stage of the whole batch + its pass's merge; 1 and 2 are its pass's, as in stark_deep_fri_prove_batch_dev.  batch == 0 returns STARK_OK.
 * STARK_ERR_INVALID_ARG, before any launch: a null ctx, table, entry, n0, r, sched_off or out; a decreasing sched_off; a null schedule with a
 * fold; an n0[i] that is not a power of two or is <= 1; a schedule that does not divide its n0.  Shapes the single call refuses with
 * STARK_ERR_UNSUPPORTED are refused with it here.  On any error every out[i] is NULL. */
int32_t stark_deep_fri_prove_mixed_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* a, const uint64_t* const* s, const uint64_t* const* e, const uint64_t* const* t,
                                             const size_t* n0, const size_t* schedule, const size_t* sched_off, const size_t* r, uint64_t seed_z, stark_proof_t** out);
/* The batch forms of "prove given f0", of the commit phase and of the merge.  Tables (f0, a, s, e, t, r_opt) are HOST arrays of `batch`
 * DEVICE pointers.  Element i of every result equals what the single call returns for trace i alone, byte for byte:
 * stark_deep_fri_prove_dev with f0; the L + 1 roots of stark_fri_build_dev (roots[(i (L + 1) + l) * 4 ..]); stark_ali_merge_dev (one omega4
 * for the batch, z and beta per trace on the host, r_opt NULL or per trace with NULL entries allowed, c_star NULL or batch x 4 on the host).
 * The traces of a pass (see stark_deep_fri_prove_batch_dev) run every step in one launch.  batch == 0 returns STARK_OK.
 * STARK_ERR_INVALID_ARG, before any launch: a null ctx, table or entry; a z[i] inside H; n0 not a power of two or <= 1 (the prove); a null
 * schedule with L > 0 or a schedule that does not divide n0.  On any error every out[i] is NULL. */
int32_t stark_deep_fri_prove_f0_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* f0, size_t n0, const size_t* schedule, size_t L, size_t r, uint64_t seed_z,
                                          stark_proof_t** out);
int32_t stark_fri_commit_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* f0, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z,
                                   uint64_t* roots /* host, batch x (L+1) x 4 */);
int32_t stark_ali_merge_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* a, const uint64_t* const* s, const uint64_t* const* e, const uint64_t* const* t,
                                  const uint64_t* const* r_opt, const uint64_t* beta /* batch x 4, host */, const uint64_t* omega4, const uint64_t* z /* batch x 4, host */,
                                  size_t n, uint64_t* const* f0, uint64_t* c_star /* batch x 4, host, may be NULL */);
size_t  stark_proof_len(stark_proof_t* p);
int32_t stark_proof_bytes(stark_proof_t* p, uint8_t* out);
size_t  stark_proof_size_estimate(stark_proof_t* p);                /* deep_fri_proof_size_bytes, fri.rs:764-805 */
double  stark_proof_stage_ms(stark_proof_t* p, int32_t stage);     /* 0 build_f0, 1 fri_build, 2 queries+encode */
int32_t stark_proof_free(stark_proof_t* p);

/* ---- verification (next row N3) --------------------------------------------------------------------
 * deep_fri_verify (fri.rs:643-762) over the canonical proof bytes stark_proof_bytes returns; *accepted = 1 / 0 (the reference
 * returns bool; bytes that do not decode are rejected, inputs on which the reference would panic are rejected).  seed_z is
 * DeepFriParams.seed_z, carried for signature parity (the reference's verifier does not read it).  Host index logic in the
 * library, every hash (leaf pairs, DS nodes) batched onto the GPU kernels of the prover: a single call is the batch call with one proof
 * (one upload, one synchronisation).  Every single verifier of this header leaves *accepted 0 on a reject and on an error. */
int32_t stark_deep_fri_verify(stark_ctx_t* ctx, const uint8_t* proof, size_t len, const size_t* schedule, size_t L, size_t r, uint64_t seed_z, int32_t* accepted);
/* deep_fri_verify (fri.rs:643-762) over `batch` canonical proofs at once; accepted[i] == what stark_deep_fri_verify answers for proofs[i]
 * alone, for every input (honest, tampered, truncated, empty, other n0).  The proofs share one schedule and r; each proof's n0 is read from
 * its own bytes.  The host plans every hash of every proof (they depend on the indices inside the proofs, never on hash values); the
 * device runs the openings of all proofs that sit at the same tree depth in one launch per Poseidon width, then compares the roots, and
 * the decisions come back with one synchronisation.  A proof that does not decode or fails a structural check is a rejection, never an
 * error.  batch == 0 returns STARK_OK.  STARK_ERR_INVALID_ARG: a null ctx or accepted (batch > 0), null proofs or lens, a null proofs[i]
 * with lens[i] != 0, a null schedule with L > 0.  On any error every accepted[i] is 0.  seed_z is carried but unused, as above. */
int32_t stark_deep_fri_verify_batch(stark_ctx_t* ctx, size_t batch, const uint8_t* const* proofs, const size_t* lens, const size_t* schedule, size_t L, size_t r,
                                    uint64_t seed_z, int32_t* accepted);
/* MerkleProver::new(MerkleChannelCfg::new(cfg_arity).with_tree_label(tree_label)).verify_single / .verify_pairs
 * (merkle/src/lib.rs:800-812, 841-855 over verify_many_ds :587-722 and verify_pairs_ds :723-773); `proof` = the canonical
 * MerkleProof encoding stark_merkle_open returns. */
int32_t stark_merkle_verify_many_ds(stark_ctx_t* ctx, size_t cfg_arity, uint64_t tree_label, const uint64_t* root4, const size_t* indices, size_t k, const uint64_t* values,
                                    const uint8_t* proof, size_t len, int32_t* accepted);
int32_t stark_merkle_verify_pairs_ds(stark_ctx_t* ctx, size_t cfg_arity, uint64_t tree_label, const uint64_t* root4, const size_t* indices, size_t k, const uint64_t* f_vals, const uint64_t* cp_vals,
                                     const uint8_t* proof, size_t len, int32_t* accepted);

/* ---- sum-check consumer (next row N4) ----------------------------------------------------------------
 * prove_plain / verify_plain and the Merkle-folded prove_mf / verify_mf (channel/src/lib.rs:1045-1240) over a witness of 2^k field
 * elements; vk = (k, tree_label[, queries_per_round]) (build_vk_plain / build_vk_mf, :1025-1043).  The witness and every folded
 * layer are committed with MerkleCommitment (commitment/src/lib.rs:60-114: arity 16, parameters "POSEIDON-T17-X5-SEED") on the GPU;
 * the Fiat-Shamir channel (:7-117) is a device-resident transcript.  The proof comes back as a stark_proof_t whose bytes are the
 * bincode 1.x layout of the reference's serde structs ProofPlain / ProofMF (:925-979) — read them with stark_proof_len /
 * stark_proof_bytes.  verify_*: *accepted = 1 / 0; a failed round check (an assert_eq! panic in the reference) is a rejection. */
/* trait CommitmentScheme for MerkleCommitment (commitment/src/lib.rs:13-27, 80-114): commit (arity 16, tree_label = ds_tag, parameters
 * "POSEIDON-T17-X5-SEED") -> a tree handle (root: stark_merkle_root; open: stark_merkle_open); verify over the bytes of stark_merkle_open. */
int32_t stark_commitment_commit(stark_ctx_t* ctx, uint64_t ds_tag, const uint64_t* leaves, size_t n, stark_tree_t** out);
/* MerkleCommitment::commit (commitment/src/lib.rs:80-90) of `batch` DEVICE vectors of n leaves: arity 16, "POSEIDON-T17-X5-SEED", tree_label = ds_tags[i];
 * stark_merkle_build_batch_dev with those parameters (same contract; out[i] equals stark_commitment_commit's tree on vector i). */
int32_t stark_commitment_commit_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* ds_tags, const uint64_t* const* leaves, size_t n, stark_tree_t** out);
/* The same of `batch` DEVICE vectors of n[i] leaves each: stark_merkle_build_mixed_batch_dev with those parameters (same contract). */
int32_t stark_commitment_commit_mixed_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* ds_tags, const uint64_t* const* leaves, const size_t* n /* host, batch */,
                                                stark_tree_t** out);
int32_t stark_commitment_verify(stark_ctx_t* ctx, uint64_t ds_tag, const uint64_t* root4, const size_t* indices, size_t k, const uint64_t* values,
                                const uint8_t* proof, size_t len, int32_t* accepted);
/* Mle::evaluate (channel/src/lib.rs:279-295): the multilinear extension of a 2^k table at r (k elements); host pointers. */
int32_t stark_mle_evaluate(stark_ctx_t* ctx, const uint64_t* table, size_t k, const uint64_t* r, uint64_t* out4);
/* Mle::evaluate (channel/src/lib.rs:279-295) of a DEVICE-resident table of 2^k elements at the point r (HOST, k elements) into out4 (DEVICE, one
 * element): the batch form below with batch = 1. */
int32_t stark_mle_evaluate_dev(stark_ctx_t* ctx, const uint64_t* table, size_t k, const uint64_t* r, uint64_t* out4);
/* Mle::evaluate (channel/src/lib.rs:279-295) of `batch` tables of 2^k elements each: tables is a HOST array of DEVICE pointers, r the HOST array of
 * the batch x k challenges (point i at r + 4 * k * i), out the batch results in DEVICE memory.  out[i] == stark_mle_evaluate on table i and point i,
 * byte for byte.  Every challenge is known up front, so one launch folds "mle_log_tile" rounds of all tables and an evaluation is
 * ceil(k / mle_log_tile) launches that read each table once.  Stream-ordered, no host synchronisation: r and the pointer table are copied before
 * the call returns.  Tables may repeat (one table at many points) and are left intact.  batch == 0 returns STARK_OK; k = 0 gives out[i] = table i's
 * only element.  STARK_ERR_INVALID_ARG, checked on the host before anything is launched: a null ctx, tables, tables[i] or out; a null r with
 * k > 0; k > 40; an out range that overlaps a table. */
int32_t stark_mle_evaluate_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* tables, size_t k, const uint64_t* r, uint64_t* out);
int32_t stark_sumcheck_prove_plain(stark_ctx_t* ctx, const uint64_t* witness, size_t k, uint64_t tree_label, stark_proof_t** out);
int32_t stark_sumcheck_prove_plain_dev(stark_ctx_t* ctx, const uint64_t* witness, size_t k, uint64_t tree_label, stark_proof_t** out);
int32_t stark_sumcheck_verify_plain(stark_ctx_t* ctx, size_t k, uint64_t tree_label, const uint8_t* proof, size_t len, int32_t* accepted);
int32_t stark_sumcheck_prove_mf(stark_ctx_t* ctx, const uint64_t* witness, size_t k, uint64_t tree_label, size_t queries_per_round, stark_proof_t** out);
int32_t stark_sumcheck_prove_mf_dev(stark_ctx_t* ctx, const uint64_t* witness, size_t k, uint64_t tree_label, size_t queries_per_round, stark_proof_t** out);
int32_t stark_sumcheck_verify_mf(stark_ctx_t* ctx, size_t k, uint64_t tree_label, size_t queries_per_round, const uint8_t* proof, size_t len, int32_t* accepted);
/* prove_plain (channel/src/lib.rs:1045-1076) of `batch` independent witnesses of 2^k elements each: witnesses[i] is a DEVICE pointer,
 * tree_labels[i] the instance's VK tree label (host array).  out[i] = what stark_sumcheck_prove_plain_dev returns for instance i alone,
 * byte for byte.  The batch runs side by side: one Merkle level of all witnesses per launch, the B transcripts in one launch per round,
 * and no host round trip inside the round loop.  batch == 0 returns STARK_OK.  STARK_ERR_INVALID_ARG (batch > 0): a null ctx, out,
 * witnesses or tree_labels, a null witnesses[i], k > 40.  On any error every out[i] is NULL.  k = 0: claim = witness[0], no rounds. */
int32_t stark_sumcheck_prove_plain_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* witnesses, size_t k,
                                             const uint64_t* tree_labels, stark_proof_t** out);
/* prove_mf (:1130-1172), same contract, one queries_per_round for the batch; one host synchronisation per round (the query indices). */
int32_t stark_sumcheck_prove_mf_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* witnesses, size_t k,
                                          const uint64_t* tree_labels, size_t queries_per_round, stark_proof_t** out);
/* The same of witnesses of DIFFERENT sizes in one pass: witnesses[i] has 2^k[i] elements (k: host array).  out[i] = what
 * stark_sumcheck_prove_{plain,mf}_dev returns for witness i under k[i] alone, byte for byte.  The rounds are aligned at the end: with
 * K = max k, instance i joins at step K - k[i], so every step runs one launch of each kind over the instances active in it and the whole batch
 * takes K steps, not the sum over the distinct sizes; only the commit of the witnesses is ragged (as stark_merkle_build_mixed_batch_dev).
 * plain: no host round trip inside the loop; mf: one host synchronisation per step, K in all.  k[i] = 0: claim = final = witnesses[i][0].
 * Errors as the batch forms, plus a null k and any k[i] > 40.  On any error every out[i] is NULL. */
int32_t stark_sumcheck_prove_plain_mixed_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* witnesses, const size_t* k /* host, batch */,
                                                   const uint64_t* tree_labels, stark_proof_t** out);
int32_t stark_sumcheck_prove_mf_mixed_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* witnesses, const size_t* k /* host, batch */,
                                                const uint64_t* tree_labels, size_t queries_per_round, stark_proof_t** out);
/* verify_plain (:1080-1128) over `batch` proofs at once; accepted[i] == what stark_sumcheck_verify_plain answers for proofs[i] alone, for
 * every input (honest, tampered, truncated, extended, empty, a proof of another k).  Like the single verifier this reads neither k nor the
 * labels: both are carried for signature parity, tree_labels may be NULL, and proofs of different round counts may share a batch.  The
 * host only parses the structure of each proof; its field elements are decoded on the device (range check, Montgomery form), the
 * transcripts of all proofs advance side by side and the round relations are checked one lane per (proof, round): one upload, a number of
 * device steps that does not depend on the batch, one download of the decisions, one synchronisation.  A proof that does not decode or
 * fails a check is a rejection, never an error.  batch == 0 returns STARK_OK.  STARK_ERR_INVALID_ARG: a null ctx or accepted (batch > 0),
 * null proofs or lens, a null proofs[i] with lens[i] != 0.  On any error every accepted[i] is 0.  Device memory is bounded: a large batch
 * runs as several plans (option "sumcheck_verify_batch_max_slots", default 2^25 field elements). */
int32_t stark_sumcheck_verify_plain_batch(stark_ctx_t* ctx, size_t batch, const uint8_t* const* proofs, const size_t* lens, size_t k, const uint64_t* tree_labels, int32_t* accepted);
/* verify_mf (:1176-1240), same contract: accepted[i] == stark_sumcheck_verify_mf on proofs[i] alone under tree_labels[i] (a null
 * tree_labels is STARK_ERR_INVALID_ARG); k and queries_per_round are carried but unread, so proofs of different round and query counts
 * may share a batch.  Every round challenge is one transcript of the batch, every Merkle opening of every round of every proof runs in
 * one launch per tree depth (MerkleCommitment's parameters), and the fold relations and root comparisons are checked one lane each. */
int32_t stark_sumcheck_verify_mf_batch(stark_ctx_t* ctx, size_t batch, const uint8_t* const* proofs, const size_t* lens, size_t k, const uint64_t* tree_labels, size_t queries_per_round,
                                       int32_t* accepted);

/* ---- Transcript (transcript/src/lib.rs:48-117) -------------------------------------------------------
 * Transcript::new(label, transcript::default_params()) / absorb_bytes / absorb_field(s) / challenge / challenges as an object:
 * the 17-lane state and the rate cursor live on the device; absorbs are queued on the host and executed (lazy permute-on-full,
 * :79-88) by one launch when the next challenge is drawn. */
int32_t stark_transcript_new(stark_ctx_t* ctx, const uint8_t* label, size_t label_len, stark_transcript_t** out);
int32_t stark_transcript_absorb_bytes(stark_transcript_t* t, const uint8_t* bytes, size_t n);
int32_t stark_transcript_absorb_fields(stark_transcript_t* t, const uint64_t* fields, size_t n);
int32_t stark_transcript_challenge(stark_transcript_t* t, const uint8_t* label, size_t label_len, uint64_t* out4);
int32_t stark_transcript_challenges(stark_transcript_t* t, const uint8_t* label, size_t label_len, size_t n, uint64_t* out);
int32_t stark_transcript_free(stark_transcript_t* t);

/* ---- One trace sharded over several GPUs ------------------------------------------
 * The commit phase shards by contiguous blocks (folds, leaf hashes and lower Merkle levels are
 * block-local: stark_fri_fold_dev, stark_leaf_pair_hash_dev, stark_merkle_build_dev with first_pos /
 * level0 / stop_at_len).  The pieces below complete the path without callbacks across the ABI:
 *  - stark_ali_merge_shard_dev: deep_ali_merge_evals(_blinded) (deep_ali/src/lib.rs:48-105) on the local
 *    block [j0, j0+n_local) of an n_global-point domain (omega4 NULL => the radix-2 domain generator); *partial4 (host, may be NULL) receives the
 *    block's share of sum_j phi_j w^j/(z - w^j); stark_ali_cstar_from_partials combines the ranks' shares
 *    (c* = (1/n) * sum, lib.rs:44,94).
 *  - stark_ali_challenges: (seed, z, beta) of DeepAliRealBuilder::build_f0 from the four column digests
 *    (fri.rs:551-560, ali_sample_z_beta_fs :511-533); digests16 = H(a),H(s),H(e),H(t) (host), aux12 = seed,z,beta (host).
 *    The column digests themselves are stark_tr_hash_fields_tagged_dev(tag "ALI/A|S|E|T", k = n0, n_hashes = 1).
 *  - query phase of deep_fri_prove (fri.rs:355-466, 613-640) over values that live on other ranks:
 *    plan_create derives every query index from the L+1 roots and lists the values the proof needs
 *    (kind 0: element `index` of layer `which`; kind 1: node `index` at `level` of tree `which`);
 *    the caller collects them (each from its owner) and plan_assemble returns the canonical proof bytes. */
int32_t stark_ali_merge_shard_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* r_opt,
                                  const uint64_t* beta4, const uint64_t* omega4, const uint64_t* z4, size_t n_local, uint64_t j0, size_t n_global,
                                  uint64_t* f0, uint64_t* partial4);
int32_t stark_ali_cstar_from_partials(stark_ctx_t* ctx, const uint64_t* partials, size_t k, size_t n_global, uint64_t* c_star4);
int32_t stark_ali_challenges(stark_ctx_t* ctx, const uint64_t* digests16, size_t n0, uint64_t* aux12);
int32_t stark_fri_plan_create(stark_ctx_t* ctx, const uint64_t* roots, size_t n0, const size_t* schedule, size_t L, size_t r, stark_fri_plan_t** out);
size_t  stark_fri_plan_num_requests(stark_fri_plan_t* p);
int32_t stark_fri_plan_requests(stark_fri_plan_t* p, uint32_t* kind, uint32_t* which, uint32_t* level, uint64_t* index);
int32_t stark_fri_plan_assemble(stark_fri_plan_t* p, const uint64_t* values, size_t n_values, stark_proof_t** out);
int32_t stark_fri_plan_free(stark_fri_plan_t* p);
/* The commit and query phases of a sharded deep_fri_prove as ONE collective call each (stark_mlwe_amd/dist.py's DistProver behind the boundary), so
 * that a host without Python drives a multi-GPU prove with one call per prove.  W = stark_comm_size of the context's communicator, or 1 when
 * stark_comm_init was never called; rank q holds the natural-order rows [q*n0/W, (q+1)*n0/W).  Collective calls must be made by every rank with
 * the same (n0, schedule, r, seed_z): every argument check happens before the first collective, and the first collective all-gathers a small
 * header of those values — when any two ranks' headers differ, EVERY rank returns STARK_ERR_INVALID_ARG (nobody is left waiting).  Every rank
 * issues the same sequence of collectives whatever its local data.
 *  - stark_fri_build_sharded_dev: fri_build_transcript (fri.rs:231-312) over the ranks.  Layers are folded block-locally while they stay
 *    shardable (hashed arity, whole Merkle and fold groups per block: stark_fri_shard_layout); the first layer that is not is all-gathered once and
 *    every later layer is replicated and committed as on one GPU (commit_pairs for arities that are not hashed).  A sharded layer's leaf
 *    hashes and lower Merkle levels are block-local with global DS positions (merkle/src/lib.rs:164-179, first_pos = q*n_l/W); the one level
 *    that crosses rank boundaries is all-gathered and every rank finishes the top identically.  Returns a handle whose L+1 roots are the same
 *    on every rank and equal stark_fri_build_dev's on the whole f0.
 *  - stark_fri_shard_prove_queries: fri_prove_queries + encoding (fri.rs:355-466, 613-640).  Every rank derives the plan from the roots; each
 *    fills the values it owns into a device table (zeros elsewhere), one stark_comm_all_reduce_u64_dev completes it, one download, and every
 *    rank receives the same canonical proof bytes.
 *  - stark_deep_fri_prove_sharded_dev: deep_fri_prove (fri.rs:601-641) from this rank's blocks of a, s, e, t: build_f0 (fri.rs:535-569; column c
 *    is gathered to rank c mod W for its serial sponge, the four digests are all-reduced, the merge is block-local), the commit, the queries.
 *    f0_opt (this rank's block of f0) skips build_f0 as in stark_deep_fri_prove_dev.  stark_proof_stage_ms 0/1/2 are filled.  At W = 1 the bytes
 *    equal stark_deep_fri_prove_dev's.
 *  - stark_diag_*_emulated_dev: diagnostic twins that run the same phase code for `nranks` VIRTUAL ranks on this one GPU, every collective as
 *    device copies (as stark_diag_lde_sharded_emulated_dev).  Inputs are the WHOLE vectors.  roots_out: nranks x (L+1) x 4 words, the roots as
 *    every virtual rank sees them; out: a host array of nranks proof handles, one per virtual rank.
 *  - stark_fri_shard_layout: the planner the calls above use (host-only, no context): sharded[l] = 1 when layer l stays block-local over nranks
 *    ranks, stop_len[l] = the local length of the level at which its lower tree stops (1 for a replicated layer, whose tree is built to its
 *    root on every rank); STARK_ERR_INVALID_ARG when nranks is not a power of two, does not divide n0, or the schedule does not divide n0.
 * STATUS: W > 1 has run only as the emulation (no multi-GPU node was available to the build). */
int32_t stark_fri_build_sharded_dev(stark_ctx_t* ctx, const uint64_t* f0_block, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, stark_fri_shard_t** out);
int32_t stark_fri_shard_num_layers(stark_fri_shard_t* h);
int32_t stark_fri_shard_root(stark_fri_shard_t* h, int32_t l, uint64_t* out4);
int32_t stark_fri_shard_is_sharded(stark_fri_shard_t* h, int32_t l);
int32_t stark_fri_shard_free(stark_fri_shard_t* h);
int32_t stark_fri_shard_prove_queries(stark_fri_shard_t* h, size_t r, stark_proof_t** out);
int32_t stark_deep_fri_prove_sharded_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* f0_opt, size_t n0,
                                         const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out);
int32_t stark_diag_fri_build_sharded_emulated_dev(stark_ctx_t* ctx, int32_t nranks, const uint64_t* f0_whole, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z,
                                                  uint64_t* roots_out);
int32_t stark_diag_deep_fri_prove_sharded_emulated_dev(stark_ctx_t* ctx, int32_t nranks, const uint64_t* a_whole, const uint64_t* s_whole, const uint64_t* e_whole,
                                                       const uint64_t* t_whole, const uint64_t* f0_opt_whole, size_t n0, const size_t* schedule, size_t L, size_t r,
                                                       uint64_t seed_z, stark_proof_t** out);
int32_t stark_fri_shard_layout(size_t n0, const size_t* schedule, size_t L, int32_t nranks, int32_t* sharded, size_t* stop_len);

/* ---- field helpers (crates/field/src/lib.rs) ------------------------------------------------------ */
/* F::get_root_of_unity(2^log_n) — Domain::new's omega (field/src/lib.rs:43-53), FriDomain::new_radix2 (fri.rs:53-56).  Host-only. */
int32_t stark_root_of_unity(int32_t field_id, size_t log_n, uint64_t* out4);
/* compute_powers(base, n) = [1, base, ..., base^(n-1)] (field/src/lib.rs:125-133; Domain::precompute_elements with base = omega). */
int32_t stark_compute_powers(stark_ctx_t* ctx, int32_t field_id, const uint64_t* base4, size_t n, uint64_t* out);
int32_t stark_compute_powers_dev(stark_ctx_t* ctx, int32_t field_id, const uint64_t* base4, size_t n, uint64_t* out);

/* ---- NTT (crates/fft/src/lib.rs:6-32) ------------------------------------------------------------- */
/* fft_in_place / ifft_in_place: natural order in and out; inverse != 0 includes the n^-1 scaling.
 * coset4 (optional): evaluate on coset4 * <w> (forward) / interpolate from it (inverse). */
int32_t stark_ntt(stark_ctx_t* ctx, int32_t field_id, uint64_t* data, size_t log_n, int32_t inverse, const uint64_t* coset4);
int32_t stark_ntt_dev(stark_ctx_t* ctx, int32_t field_id, uint64_t* data, size_t log_n, int32_t inverse, const uint64_t* coset4);
/* LDE: 2^log_n evaluations on <w_n> -> 2^(log_n+log_blowup) evaluations on coset4 * <w_N> (coset4 NULL => 1). */
int32_t stark_lde(stark_ctx_t* ctx, int32_t field_id, const uint64_t* evals, size_t log_n, size_t log_blowup, const uint64_t* coset4, uint64_t* out);
int32_t stark_lde_dev(stark_ctx_t* ctx, int32_t field_id, const uint64_t* evals, size_t log_n, size_t log_blowup, const uint64_t* coset4, uint64_t* out);
/* `batch` transforms / extensions of one shape and one coset; tables are HOST arrays of `batch` DEVICE pointers.
 * Element i equals what stark_ntt_dev / stark_lde_dev returns for column i alone, byte for byte.
 * Stream-ordered with no host synchronisation, like the single calls (the tables are copied before the call returns).  batch == 0 is STARK_OK.
 * STARK_ERR_INVALID_ARG, checked on the host before anything is launched: a null ctx, table or entry; log_n (or log_n + log_blowup) outside
 * the single call's range (0..30); an unknown field; two `out` ranges (two `data` ranges) that overlap.
 * Inputs may repeat, and evals[i] may be out[i]: a column is read completely before its output is written.  Inputs are otherwise left intact; an
 * input that overlaps ANOTHER column's output is not supported (columns of different passes are not ordered against each other).
 * The batch is cut into passes of at most "ntt_batch_max_elems" output elements (option, default 2^24: 512 MiB of outputs and as much scratch);
 * inside a pass every step of the single call is ONE launch for all columns and the columns are read and written in place through pointer
 * tables (no gather copy).  A pass of one column — every column larger than the limit — is the single call itself. */
int32_t stark_ntt_batch_dev(stark_ctx_t* ctx, int32_t field_id, size_t batch, uint64_t* const* data, size_t log_n, int32_t inverse, const uint64_t* coset4);
int32_t stark_lde_batch_dev(stark_ctx_t* ctx, int32_t field_id, size_t batch, const uint64_t* const* evals, size_t log_n, size_t log_blowup,
                            const uint64_t* coset4, uint64_t* const* out);
/* The same with a length per column: log_n is a HOST array of `batch` entries, column i has 2^log_n[i] elements and is extended onto
 * coset4 * <w_{N_i}>, N_i = 2^(log_n[i] + log_blowup); one log_blowup and one coset for the call.  Column i equals what stark_ntt_dev /
 * stark_lde_dev returns for it alone under log_n[i], byte for byte.
 * Stream-ordered with no host synchronisation; log_n, both tables and coset4 may be overwritten or freed the moment the call returns.  Inputs may
 * repeat, and evals[i] may be out[i]; inputs are otherwise left intact; an input that overlaps ANOTHER column's output is not supported.
 * batch == 0 is STARK_OK.  A column with log_n[i] == 0 takes no part in the transform; its extension is 2^log_blowup copies of its point.
 * STARK_ERR_INVALID_ARG, checked on the host before anything is launched or allocated (the outputs stay untouched): a null ctx, table, entry or
 * log_n; any log_n[i] or log_n[i] + log_blowup above 30; an unknown field; two `out` ranges (two `data` ranges), now of different lengths, that overlap.
 * The batch is cut into consecutive passes of at most "ntt_batch_max_elems" output elements, in the caller's order (a greedy run over the sum of
 * N_i); a pass of one column is the single call itself.  Inside a pass the passes of all transforms are aligned at the end of a three-step
 * schedule and every step is one launch per kernel form for all columns, whatever their sizes: at most 5 launches for the transforms and
 * 3 + 1 + 5 for the extensions (inverse transforms, one pad launch, forward transforms), independent of `batch` and of the sizes that occur.
 * Scratch of a pass: the sum of N_i + 2^log_n[i] elements. */
int32_t stark_ntt_mixed_batch_dev(stark_ctx_t* ctx, int32_t field_id, size_t batch, uint64_t* const* data, const size_t* log_n, int32_t inverse,
                                  const uint64_t* coset4);
int32_t stark_lde_mixed_batch_dev(stark_ctx_t* ctx, int32_t field_id, size_t batch, const uint64_t* const* evals, const size_t* log_n, size_t log_blowup,
                                  const uint64_t* coset4, uint64_t* const* out);
/* Building blocks of the multi-GPU six-step NTT (one process per GPU; the exchange between the two
 * is an all-to-all done by the caller, see stark_mlwe_amd/dist.py):
 *   phase A: `ncols` column NTTs of size 2^log_rows on a row-major [2^log_rows][ncols] slab, then the
 *            twiddle w_N^(col_global * k) (N = 2^log_n, col_global = col0 + local column).
 *   phase B: `nrows` contiguous NTTs of size 2^log_cols (plain stark_ntt batched over rows). */
int32_t stark_ntt_columns_dev(stark_ctx_t* ctx, int32_t field_id, uint64_t* slab, size_t log_rows, size_t ncols, size_t col0, size_t log_n, int32_t inverse);
int32_t stark_ntt_rows_dev(stark_ctx_t* ctx, int32_t field_id, uint64_t* slab, size_t nrows, size_t log_cols, int32_t inverse, const uint64_t* scale4);
/*   phase A of a COSET transform: as stark_ntt_columns_dev (forward), with x[j] *= shift4^j on load, j = the element's natural
 *            index in the whole vector (row * 2^(log_n-log_rows) + col0 + local column) — one of the 2^log_blowup cosets of an LDE.
 *   stark_permute3_dev: dst (contiguous) = the [d0][d1][d2] array src with its axes permuted to (p0, p1, p2) — the layout
 *            changes on either side of an all-to-all (32-byte elements).
 *   stark_interleave_dev: dst[k*stride + offset] = src[k], k < n — the coset transforms of an LDE into natural order. */
/*   stark_ntt_rows_coset_dev: first local phase of a forward COSET transform on the layout the inverse six-step transform leaves behind
 *            (rows k1 = row0 .. row0+nrows of the [R][C] view c[k1 + R k'], C = 2^log_cols contiguous, R = 2^(log_n-log_cols)):
 *            dst[i][m] = w_n^(k1 m) * sum_k' src[i][k'] shift^(k' R + k1) w_C^(k' m).  src is not modified (all cosets of an LDE start from it);
 *            the second phase is a plain size-R transform over k1 after ONE exchange — no exchange between inverse and forward. */
int32_t stark_ntt_rows_coset_dev(stark_ctx_t* ctx, int32_t field_id, const uint64_t* src, uint64_t* dst, size_t nrows, size_t log_cols, size_t row0, size_t log_n, const uint64_t* shift4);
/*   stark_lde_sharded_dev: the whole LDE of ONE column block-sharded over the ranks of the context's communicator (stark_comm_init; one rank without a
 *            communicator is allowed): rank q passes its natural-order block of 2^log_n / W evaluations and receives its block of the 2^(log_n+log_blowup)
 *            evaluations on shift * <w_N> — the composition of the building blocks above with FOUR all-to-alls, inside the library, so that a host
 *            without Python (the reference's Rust process) drives a multi-GPU LDE with one call per column.  (dist.py's ShardedLde is the same
 *            composition in Python and stays the form the CPU gloo tests exercise.) */
int32_t stark_lde_sharded_dev(stark_ctx_t* ctx, int32_t field_id, const uint64_t* block, size_t log_n, size_t log_blowup, const uint64_t* shift4, uint64_t* out);
/* Diagnostic: the same phases for `nranks` VIRTUAL ranks on this one GPU, every exchange done as device copies — what checks the index arithmetic of
 * stark_lde_sharded_dev for W > 1 without a second GPU.  evals: the whole 2^log_n vector; out: the whole extended vector (= stark_lde_dev's). */
int32_t stark_diag_lde_sharded_emulated_dev(stark_ctx_t* ctx, int32_t field_id, int32_t nranks, const uint64_t* evals, size_t log_n, size_t log_blowup, const uint64_t* shift4, uint64_t* out);
int32_t stark_ntt_columns_coset_dev(stark_ctx_t* ctx, int32_t field_id, uint64_t* slab, size_t log_rows, size_t ncols, size_t col0, size_t log_n, const uint64_t* shift4);
int32_t stark_permute3_dev(stark_ctx_t* ctx, const uint64_t* src, uint64_t* dst, size_t d0, size_t d1, size_t d2, int32_t p0, int32_t p1, int32_t p2);
int32_t stark_interleave_dev(stark_ctx_t* ctx, const uint64_t* src, uint64_t* dst, size_t n, size_t stride, size_t offset);

/* ---- the communicator (RCCL over xGMI; one process per GPU) ------------------------------------------------------------
 * The exchanges of the path behind the boundary, so that a host without torch can drive several GPUs:
 * rank 0 calls stark_comm_unique_id and passes the 128 bytes to its peers by its own means; every rank then calls
 * stark_comm_init on its context (collective: returns when all ranks have joined).  The data-path calls below are enqueued on
 * the context's stream (no host synchronisation) and must be made by all ranks in the same order.  Without a usable RCCL the
 * calls fail with STARK_ERR_RCCL; nothing else in the library depends on it. */
#define STARK_COMM_ID_BYTES 128
/* Local probe (dlopen + ncclGetVersion, no communication): STARK_OK when RCCL can be bound and reports the major version whose ABI this
 * library was checked against, else STARK_ERR_RCCL; *version_code (may be NULL) = its NCCL_VERSION_CODE.  Ranks agree on the answer BEFORE any
 * of them enters the collective stark_comm_init (a rank that cannot load RCCL must not leave its peers blocked in ncclCommInitRank).
 * STATUS: the N > 1 paths of this section have not run on hardware yet (no multi-GPU node was available to the build). */
int32_t stark_comm_available(int32_t* version_code);
int32_t stark_comm_unique_id(uint8_t* id128);
int32_t stark_comm_init(stark_ctx_t* ctx, int32_t nranks, int32_t rank, const uint8_t* id128);
int32_t stark_comm_destroy(stark_ctx_t* ctx);
int32_t stark_comm_size(stark_ctx_t* ctx);
int32_t stark_comm_rank(stark_ctx_t* ctx);
/* all-to-all: chunk q (bytes_per_peer) of `send` goes to rank q; chunk p of `recv` is what rank p sent here — the row/column
 * transpose of the six-step NTT, one message per peer link.  send != recv. */
int32_t stark_comm_all_to_all_dev(stark_ctx_t* ctx, const void* send, void* recv, size_t bytes_per_peer);
int32_t stark_comm_all_gather_dev(stark_ctx_t* ctx, const void* send, void* recv, size_t bytes);
int32_t stark_comm_all_reduce_u64_dev(stark_ctx_t* ctx, const void* send, void* recv, size_t count);   /* SUM of uint64 words (send == recv allowed) */
int32_t stark_comm_gather_dev(stark_ctx_t* ctx, const void* send, void* recv, size_t bytes, int32_t root);

/* ---- synthetic inputs for benchmarks (DESIGN.md "Synthetic inputs") ------------------------------- */
/* The reference's OWN bench inputs (channel/benches/end_to_end.rs:249-253): ncols vectors of n elements from one
 * StdRng::seed_from_u64(seed) through ark-ff's Fp::rand, written to HOST memory (host-only, no context): with the seed chain of
 * end_to_end.rs:214-253 the prover's size estimate must equal the `proof_bytes` the reference published (benchmarkdata.csv). */
int32_t stark_ref_bench_inputs(uint64_t seed, size_t n, size_t ncols, uint64_t* out);
int32_t stark_synth_column_dev(stark_ctx_t* ctx, uint64_t seed, uint64_t col, size_t i0, size_t n, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* STARK_MLWE_H */
