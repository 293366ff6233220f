// stark_mlwe_amd/csrc/ctx.hpp — internal objects behind the opaque C-ABI handles (product code).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../include/stark_mlwe.h"
#include "fr.hpp"
#include "host_util.hpp"
#include "poseidon_params.hpp"
#include "ntt_dev.hpp"
#include "fri_plan.hpp"

namespace stark { struct NttPlan; struct PowCache; }
struct stark_ctx;

// Handles (trees, FRI states, plans, transcripts, caller-made parameter sets) keep their context alive: stark_ctx_destroy with live handles
// only marks the context; the LAST handle freed tears it down.  `CtxRef` is the FIRST member of every handle type and members are destroyed in
// reverse order, so it is destroyed last — after the handle's owners (DevBuf, unique_ptr<stark_tree>, the shared TreeBlocks) have returned
// their blocks to the context's pool.  No handle has a destructor of its own.  (A Rust host drops its thread-local context at thread exit
// while Tree / ProverState values owned by the caller may outlive it — ADVICE r2.)
namespace stark { void ctx_ref(stark_ctx* c); void ctx_unref(stark_ctx* c); }
struct CtxRef {
    stark_ctx* c = nullptr;
    CtxRef() = default; CtxRef(const CtxRef&) = delete; CtxRef& operator=(const CtxRef&) = delete;
    void bind(stark_ctx* x) { if (x) stark::ctx_ref(x); if (c) stark::ctx_unref(c); c = x; }
    ~CtxRef() { if (c) stark::ctx_unref(c); }
};

namespace stark {
// THE device allocation of the library proper (capi_core.hip): hipMalloc for the unpooled tables (DevMem::alloc, a request of its own) and for the two
// attempts of a pool miss (ctx_alloc, which counts its request itself).  A failure leaves *out NULL and the runtime's last error CLEARED: the
// launches are checked with hipGetLastError, which reports the last error any earlier call on the thread returned, so an out-of-memory status left
// behind would be reported by the next, innocent call.  The refusal hook (stark_ctx::alloc_hook) lives here.
enum DevMallocKind { kDevTable, kDevPoolFirst, kDevPoolRetry };
hipError_t dev_malloc(stark_ctx* ctx, void** out, size_t bytes, DevMallocKind kind);
// Owner of ONE unpooled device allocation (dev_malloc on alloc, hipFree on reset / destruction; move-only): the long-lived tables and constants.
// They stay outside the context's pool, so stark_ctx_trim and the out-of-memory retry of ctx_alloc never touch them.  An owner is destroyed
// with its context's device current (see ctx_teardown); DevBuf below is the pooled, per-call counterpart.
struct DevMem {
    void* p = nullptr;
    DevMem() = default; DevMem(const DevMem&) = delete; DevMem& operator=(const DevMem&) = delete;
    DevMem(DevMem&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem& operator=(DevMem&& o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~DevMem() { reset(); }
    hipError_t alloc(stark_ctx* ctx, size_t bytes) { reset(); return dev_malloc(ctx, &p, bytes, kDevTable); }
    // THE one-off fill of a long-lived table: alloc(bytes), the copy from host memory on the context's stream, and the synchronisation right behind it
    // (src may die on return).  The static form copies into device memory somebody else owns.  Defined below stark_ctx.
    int32_t fill_sync(stark_ctx* ctx, const void* src, size_t bytes);
    static int32_t fill_sync(stark_ctx* ctx, void* dst, const void* src, size_t bytes);
    void reset() { if (p) { (void)hipFree(p); p = nullptr; } }
    explicit operator bool() const { return p != nullptr; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
    fr_t* fr() const { return as<fr_t>(); }
};
}  // namespace stark

struct stark_params {
    CtxRef ref_;                         // bound only for parameter sets handed to the caller (the context's own cached sets do not pin it)
    stark_ctx* ctx = nullptr;
    stark::host::PoseidonConsts ref;     // reference-form constants (as uploaded / derived)
    stark::host::KernelConsts kc;        // kernel-form constants
    stark::DevMem blob;                  // one device allocation holding all tables
    stark::PoseidonDev dev{};            // device pointers into `blob`
};

struct stark_comm;
struct stark_ctx {
    int device = 0;
    int num_cus = 256;                               // compute units of the device (persistent NTT grids)
    stark_comm* comm = nullptr;                      // RCCL communicator spanning the ranks (capi_comm.hip); nullptr until stark_comm_init
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t side_stream = nullptr;               // lazily created: small independent jobs that run underneath a big one (fri_build)
    std::string err;
    int live_handles = 0; bool destroy_pending = false;   // see CtxRef
    hipEvent_t ev0 = nullptr, ev1 = nullptr;         // stark_timer_start / stop
    hipEvent_t ev_fork = nullptr;                    // orders the side stream after the main one and back (ctx_fork / ctx_join)
    // lazily created constants
    std::unique_ptr<stark_params> tparams;           // transcript params (t=17, "POSEIDON-T17-X5-TRANSCRIPT")
    std::map<int, std::unique_ptr<stark_params>> merkle_params;   // poseidon_params_for_width(t)
    stark::DevMem leaf_init;                         // one LeafConsts: the 17-lane template of hash_leaf_pair and round 0 in closed form (device)
    std::map<std::string, stark::DevMem> tr_frames;  // per-tag transcript prefix/suffix frames (device): [prefix.., suffix..]
    std::map<std::string, std::pair<int, int>> tr_frame_dims;
    // scratch
    stark::DevMem scratch; size_t scratch_bytes = 0;
    // NTT plans
    std::map<uint64_t, stark::NttPlan*> plans;
    // Caching device allocator for the library's own temporaries, layers and tree levels: a block released here is reused by a
    // later request of the same (rounded) size WITHOUT hipFree / hipMalloc, so the hot path neither synchronises the device nor
    // pays allocation latency.  Safe because every use of such a block is ordered on this context's stream (the side stream
    // joins the main one before anything it touched is released).  stark_ctx_trim() returns the cached blocks to the driver.
    std::map<size_t, std::vector<void*>> pool_free;
    std::map<void*, size_t> pool_live;
    size_t pool_cached_bytes = 0;
    // host-side caches of values that depend only on their key
    struct ZKey { uint64_t seed; size_t level, size; bool operator<(const ZKey& o) const { return seed != o.seed ? seed < o.seed : (level != o.level ? level < o.level : size < o.size); } };
    std::map<ZKey, stark::fr_t> z_cache;                                // fri_sample_z_ell(seed_z, level, size)  (fri.rs:59-82)
    std::unique_ptr<stark::PowCache> omega_tabs;                       // two-level power tables of a domain generator (DomainH, deep_ali/src/lib.rs:109-125); pow_table.hpp, made on first use
    void* pinned = nullptr; size_t pinned_bytes = 0;                   // small pinned staging area for async uploads / downloads
    // Host sources of the uploads of everything the library built on the host (ctx_upload_staged: pointer tables, transcript inputs, headers).
    // Each copy lives until the event recorded behind its upload has passed; later calls reap the finished ones, teardown the rest.
    struct StagedUpload { hipEvent_t done; std::unique_ptr<uint8_t[]> host; };
    std::vector<StagedUpload> staged;

    // tuning / diagnostic options (stark_ctx_set_option): explicit API state, never the environment
    struct Options {
        int ntt_direct_max_log = 24;     // direct (one-product) twiddle / coset tables for transforms up to 2^this (0 disables)
        bool ntt_merged_coset = true;    // coset transforms: the pre-scale folded into the first pass's twiddle table (one table read instead of two); 0 = separate tables (comparison)
        int ntt_log_tile = 11;           // log2 of the elements of an NTT tile (8..12); -1 would mean "auto" (the default also shrinks for small launches)
        bool ntt_log_tile_forced = false;
        int ntt_min_waves = 2;           // occupancy hint of the NTT kernels (2 or 4 waves per SIMD)
        int sponge_debug = 0;            // timing experiments on the five-wave sponge (bit 0: A does not wait, 1: B idle, 2: C idle, 3: no full rounds, 4: no partial rounds); digests are WRONG when set
        bool sponge_one_wave = false;    // long serial sponges on ONE wave (poseidon_coop.hpp, round 2) instead of three (poseidon_chain.hpp) (diagnostic / comparison)
        bool poseidon_lane_only = false; // one-lane-per-sponge kernels instead of the wave-pair / one-wave forms (diagnostic)
        bool merkle_node16_pair = true;  // t = 17 Merkle levels of > 4096 nodes with exactly 16 children each: the fixed two-permutation kernel k_node16_pair; 0 = the generic k_hash_ds2 (comparison)
        bool poseidon_block8 = true;     // t = 17 wave-pair kernels (k_leaf_pair2, k_hash_ds2<17>, k_node16_pair), parameter sets with rp % 8 == 0: partial rounds in blocks of 8 with the E-product and the lane product on the matrix cores; 0 = blocks of 4 on the vector ALU (comparison)
        bool merkle_wave_pair = false;   // Merkle levels of t = 9, 17 in the wave-pair form at EVERY size, as under side_commit (diagnostic: the wave-pair kernels at their smallest shapes)
        bool fri_side_pair = true;       // fri_build: the small layers' commitments on the side stream in the wave-pair form at every size (see side_commit); 0 = the latency forms (comparison)
        size_t sumcheck_verify_batch_max_slots = (size_t)1 << 25;   // a plan of the batched sum-check verifiers is run once it holds this many pool slots (1 GiB of field elements): device memory stays bounded whatever the batch
        size_t ntt_batch_max_elems = (size_t)1 << 24;    // the batched NTT / LDE calls cut a batch into passes of at most this many output elements (ntt_mixed_passes, ntt_mixed_plan.hpp): 512 MiB of outputs and as much scratch per pass
        size_t prove_batch_max_rows = (size_t)1 << 22;   // the batched DEEP-FRI provers cut a batch into passes of at most this many rows (traces x n0) whose tails run side by side (fri_batch.hpp); device memory per pass stays near 70 B per row
        int mle_log_tile = -1;           // log2 of the elements one workgroup of k_mle_fold_pass folds to one (3..12); -1 = the default of mle_dev.hpp
        int mle_lane_contiguous = -1;    // a lane of k_mle_fold_pass owns consecutive (1) or interleaved (0) elements; -1 = the default of mle_dev.hpp (comparison)
        size_t lagrange_max_partials = (size_t)1 << 21;  // stark_lagrange_eval_on_h_batch_dev cuts the points of a call into passes of at most this many block partials (points x columns x workgroups per column; lagrange_dev.hpp): 64 MiB of scratch per pass; a pass of one point is always allowed
        int lagrange_wide_acc = -1;      // k_lagrange_partials: a lane's K products of a column in the lazy accumulator (1) or as K products and additions (0); -1 = the default of lagrange_dev.hpp (comparison)
        int lagrange_col_groups = -1;    // k_lagrange_partials: the column groups of a launch (blockIdx.z): 1 = one group, g > 1 = min(g, ncols) groups; -1 = automatic (lag_col_groups, lagrange_dev.hpp).  Every value gives the same bytes
        int lagrange_shared_inverse = 0; // lagrange_eval_batch: 1 = one Fermat inversion per point and pass (k_lagrange_totals, k_lagrange_invert, the shared form of k_lagrange_partials) instead of one per workgroup; 0 = the default.  Every value gives the same bytes
        int lagrange_share_cosets = 0;   // lagrange_eval_batch, whole-domain form: 1 = points of one coset of H (z, z w^s) share the weights of the first of them, the columns read at the shift; 0 = the default; the block form ignores it.  Every value gives the same bytes
        bool mixed_prove_tail = false;   // stark_deep_fri_prove_mixed_batch_dev: 0 = traces of equal (n0, schedule, r) share a tail (mixed_prove_groups); 1 = traces of equal schedule share ONE ragged tail whatever their n0 and r (mixed_prove_classes, fri_mixed.hpp).  Every value gives the same bytes
        int pool_poison = -1;            // TESTS ONLY: 0..255 = ctx_alloc fills every block it hands out (the whole rounded block, recycled or fresh) and ctx_scratch the scratch vector
                                         // with this byte, so a read of a temporary nobody wrote shows; each fill synchronises the stream.  -1 = off (one branch per allocation, no HIP call)
    } opt;
    // TESTS ONLY (stark_diag_alloc_refusal): refuses one chosen allocation request, so that the error paths behind every allocation can be run.
    // mode 0 = off (one branch per request, no HIP call).  mode 1: requests are counted — every ctx_alloc call, pool hit or miss, and every
    // DevMem::alloc — and request number `at` (from 1; 0 = count only) is refused as a failed allocation is: STARK_ERR_OOM from ctx_alloc,
    // hipErrorOutOfMemory from DevMem::alloc.  mode 2: pool misses are counted and the FIRST hipMalloc attempt of miss number `at` is refused, so
    // ctx_alloc gives its cached blocks back and tries again.  A hook that fired disarms itself (counting goes on).
    // mode 3: as mode 2 with the SECOND attempt refused as well: the give-back runs and the request still fails, the last branch of a real failure.
    // cached_after_give_back: pool_cached_bytes as the give-back's own accounting left it (~0 until a give-back ran while the hook was on).
    struct AllocHook { int mode = 0; uint64_t at = 0, requests = 0, fired = 0, cached_after_give_back = ~(uint64_t)0; bool refuse_retry = false; } alloc_hook;
    bool side_commit = false;            // set while fri_build enqueues work that runs underneath the 2^n-leaf launch: Merkle levels and leaf layers of t = 9, 17 take the
                                         // wave-pair form (64 sponges per two waves) instead of one wave or five waves per sponge, which would hold many wave slots at lone-wave speed

    int32_t fail(int32_t code, const std::string& msg) { err = msg; return code; }
};

namespace stark {
// The pooled allocator's two functions (capi_core.hip; see stark_ctx::pool_free).  Only DevBuf calls them.
int32_t ctx_alloc(stark_ctx* ctx, size_t bytes, void** out);
void ctx_release(stark_ctx* ctx, void* p);

// THE owner of one pooled block (move-only): the block returns to its context's pool on reset() or destruction, exactly once, by whoever holds
// the owner at that point.  Temporaries of an entry point, the layers and tree levels of the handles and adopted blocks (merkle_build_on) are all this.
struct DevBuf {
    stark_ctx* ctx = nullptr; void* p = nullptr;
    DevBuf() = default; DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : ctx(o.ctx), p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); ctx = o.ctx; p = o.p; o.p = nullptr; } return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p) { ctx_release(ctx, p); p = nullptr; } }      // releases now; idempotent
    int32_t take(stark_ctx* c, size_t bytes) { reset(); ctx = c; return ctx_alloc(c, bytes, &p); }     // the allocator's own code and message
    hipError_t alloc(stark_ctx* c, size_t bytes) { return take(c, bytes) == STARK_OK ? hipSuccess : hipErrorOutOfMemory; }
    // (no upload member: host memory reaches a block through ctx_upload_staged or a CallerUploads guard, below)
    // the first `bytes` to host memory, then one synchronisation of the context's stream
    hipError_t download_sync(void* dst, size_t bytes) const { const hipError_t e = bytes ? hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess; return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream); }
    fr_t* fr() const { return reinterpret_cast<fr_t*>(p); }
};
// The pooled blocks the trees of one batched build share (merkle_batch.hpp: level v of all trees is one block): every tree of the batch holds a
// reference, and the blocks go back to the context's pool when the last of them is freed.  Each holding tree pins the context (its CtxRef outlives
// this member), so the context is alive whenever the blocks are released.
struct TreeBlocks { std::vector<DevBuf> blocks; };
}
struct stark_tree {
    CtxRef ref_;
    stark_ctx* ctx = nullptr; stark_params* p = nullptr;
    size_t arity = 0; uint64_t label = 0;
    std::vector<stark::fr_t*> levels; std::vector<size_t> lens;   // the raw views MerkleTreeView and the kernels read
    std::vector<stark::DevBuf> blocks;                             // the blocks this tree owns (a tree of its own: one per level)
    std::shared_ptr<stark::TreeBlocks> shared;                     // a tree of a batched build: its levels are slices of these blocks
    stark_tree(stark_ctx* c, stark_params* p_, size_t arity_, uint64_t label_) : ctx(c), p(p_), arity(arity_), label(label_) { ref_.bind(c); }
};
struct stark_proof { std::vector<uint8_t> bytes; size_t size_estimate = 0; double ms[3] = {0, 0, 0}; };   // a finished proof (capi_fri.hip, capi_sumcheck.hip): bytes, size estimate, stage times
// the single success point of a call that returns proofs: the caller owns out[0 .. v.size()) from here on
inline void hand_out(std::vector<std::unique_ptr<stark_proof>>& v, stark_proof** out) { for (size_t i = 0; i < v.size(); ++i) out[i] = v[i].release(); }

#define STARK_HIP(ctx, call)                                                                                     \
    do {                                                                                                         \
        hipError_t e__ = (call);                                                                                 \
        if (e__ != hipSuccess) return (ctx)->fail(e__ == hipErrorOutOfMemory ? STARK_ERR_OOM : STARK_ERR_HIP,     \
                                                  std::string(#call) + ": " + hipGetErrorString(e__));           \
    } while (0)
#define STARK_TRY(expr) do { int32_t rc__ = (expr); if (rc__ != STARK_OK) return rc__; } while (0)

namespace stark {

inline int32_t DevMem::fill_sync(stark_ctx* ctx, void* dst, const void* src, size_t bytes) {
    STARK_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream)); return STARK_OK;
}
inline int32_t DevMem::fill_sync(stark_ctx* ctx, const void* src, size_t bytes) { STARK_HIP(ctx, alloc(ctx, bytes)); return fill_sync(ctx, p, src, bytes); }

inline const fr_t* as_fr(const uint64_t* p) { return reinterpret_cast<const fr_t*>(p); }
inline fr_t* as_fr(uint64_t* p) { return reinterpret_cast<fr_t*>(p); }
inline fr_t load_fr(const uint64_t* p) { fr_t x; for (int i = 0; i < 4; ++i) { x.v[2 * i] = (uint32_t)p[i]; x.v[2 * i + 1] = (uint32_t)(p[i] >> 32); } return x; }
inline void store_fr(uint64_t* p, const fr_t& x) { for (int i = 0; i < 4; ++i) p[i] = (uint64_t)x.v[2 * i] | ((uint64_t)x.v[2 * i + 1] << 32); }

// THE row gather on the device (capi_poseidon.hip; the list: merkle_batch.hpp): the four tables go up as ONE packed ctx_upload_staged block (the list
// may die on return), then ONE k_gather_rows launch into out_dev (nullptr: a pooled table of G.size() rows).  out_host (optional, host memory of any
// alignment): the first G.size() rows of the table are downloaded and the context's stream synchronised.  Index bounds are the caller's to check.
struct MerkleGatherList;
int32_t gather_rows(stark_ctx* ctx, const MerkleGatherList& G, fr_t* out_dev, void* out_host);

// shared internal entry points (defined in capi_core.hip / capi_ntt.hip / capi_comm.hip; the Poseidon ones: poseidon_launch.hpp)
int32_t ctx_transcript_params(stark_ctx* ctx, stark_params** out);
int32_t ctx_merkle_params(stark_ctx* ctx, int t, stark_params** out);
int32_t ctx_commit_params(stark_ctx* ctx, stark_params** out);      // MerkleCommitment's set (the sum-check openings)
int32_t ctx_scratch(stark_ctx* ctx, size_t bytes, void** out);
// Host memory reaches the device in three functions and nowhere else ("Uploads"): DevMem::fill_sync above and the two below.
// THE upload of what the library itself built on the host: `bytes` of host memory to device memory on the context's stream, out of a copy the
// context owns (stark_ctx::staged).  The source may die on return, on every path, and the host is not synchronised.
int32_t ctx_upload_staged(stark_ctx* ctx, void* dst, const void* src, size_t bytes);
// THE upload of memory the library does not own and will not copy a second time: the caller's arrays of the host-pointer entry points (and a large
// staging vector of the same scope).  copy() / up() enqueue the direct copy; a scope left before the stream was synchronised behind them (an error,
// or a success path that only enqueues) synchronises it here, so a plain-named entry point returns, with any status, only after the device has
// finished reading the caller's arrays.  Declared AFTER the DevBufs it fills and after the host memory it reads (as StreamFork below: destroyed
// first, the fence runs before the blocks return to the pool).  A success path ends in download_sync() or sync(): one synchronisation, none here;
// a path whose callee synchronised on its way (a prove) just returns and pays one more on an idle stream.
struct CallerUploads {
    stark_ctx* ctx; bool pending = false;
    explicit CallerUploads(stark_ctx* c) : ctx(c) {}
    CallerUploads(const CallerUploads&) = delete; CallerUploads& operator=(const CallerUploads&) = delete;
    ~CallerUploads() { if (pending) (void)hipStreamSynchronize(ctx->stream); }
    hipError_t copy(void* dst, const void* src, size_t bytes) { if (!bytes) return hipSuccess; pending = true; return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream); }
    // a pooled block of `bytes` into d, then its copy() from src
    hipError_t up(DevBuf& d, const void* src, size_t bytes) { const hipError_t e = d.alloc(ctx, bytes); return e != hipSuccess ? e : copy(d.p, src, bytes); }
    hipError_t sync() { const hipError_t e = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) pending = false; return e; }
    // the finish of a call: `bytes` of device memory to host memory, then the one synchronisation
    hipError_t download_sync(void* dst, const void* src, size_t bytes) { const hipError_t e = bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess; return e != hipSuccess ? e : sync(); }
};
// THE memory of an executor of the templated drivers (fri_batch.hpp, sumcheck_batch.hpp, lagrange_dev.hpp, merkle_batch.hpp): pooled blocks that
// return to the pool with it, host tables through upload / put (the source may die on return), download = copy + synchronisation.  The device
// executors derive from it and add their launches; hostcheck.cpp's HostArena is its twin.
// Where the host copy of an upload lives: in the context (ctx_upload_staged, an event per upload: the executors whose calls return without a
// synchronisation), or — hold_until_download, for a driver that downloads after every few uploads (the sum-check rounds, where the event per upload
// measured 2 - 4 %: profiles/sumcheck_batch_parent_vs_upload_discipline.jsonl) — in the arena until its next download() has synchronised; an
// arena left with such copies outstanding synchronises first (`fence` is the last member: it runs before `held` and `blocks` go).
struct DevArena {
    stark_ctx* ctx; std::vector<DevBuf> blocks; const bool hold; std::vector<std::unique_ptr<uint8_t[]>> held; CallerUploads fence;
    explicit DevArena(stark_ctx* c, bool hold_until_download = false) : ctx(c), hold(hold_until_download), fence(c) {}
    int32_t alloc(size_t bytes, void** out) { DevBuf b; STARK_TRY(b.take(ctx, bytes)); *out = b.p; blocks.push_back(std::move(b)); return STARK_OK; }
    int32_t upload(void* dst, const void* src, size_t bytes) {
        if (!hold || !bytes) return ctx_upload_staged(ctx, dst, src, bytes);
        held.emplace_back(new uint8_t[bytes]); memcpy(held.back().get(), src, bytes);
        STARK_HIP(ctx, fence.copy(dst, held.back().get(), bytes)); return STARK_OK;
    }
    template <class T> int32_t put(const std::vector<T>& h, T** out) {
        void* p = nullptr; STARK_TRY(alloc(std::max<size_t>(h.size(), 1) * sizeof(T), &p));
        if (!h.empty()) STARK_TRY(upload(p, h.data(), h.size() * sizeof(T)));
        *out = (T*)p; return STARK_OK;
    }
    int32_t download(void* dst, const void* src, size_t bytes) {
        STARK_HIP(ctx, fence.download_sync(dst, src, bytes)); held.clear(); return STARK_OK;
    }
};
int32_t ctx_side_stream(stark_ctx* ctx, hipStream_t* out);
// Fork: what is enqueued on *side from here on runs after everything enqueued on the context's stream so far, and concurrently with what that stream
// receives next.  Join: the context's stream continues after everything enqueued on the side stream.  Events only; the host is not synchronised.
int32_t ctx_fork(stark_ctx* ctx, hipStream_t* side);
int32_t ctx_join(stark_ctx* ctx);
// THE fork guard: whoever forks holds one, declared AFTER the owners of what the two streams use.  A scope left while still forked (an error
// between fork() and join(), or a failed join) drains the side stream and then the context's stream before those owners release anything;
// a joined guard does nothing, so no success path synchronises.
struct StreamFork {
    stark_ctx* ctx; hipStream_t side = nullptr; bool forked = false;
    explicit StreamFork(stark_ctx* c) : ctx(c) {}
    StreamFork(const StreamFork&) = delete; StreamFork& operator=(const StreamFork&) = delete;
    ~StreamFork() { if (forked) { (void)hipStreamSynchronize(side); (void)hipStreamSynchronize(ctx->stream); } }
    int32_t fork() { STARK_TRY(ctx_fork(ctx, &side)); forked = true; return STARK_OK; }
    int32_t join() { if (forked) { STARK_TRY(ctx_join(ctx)); forked = false; } return STARK_OK; }
};
int32_t ctx_enter(stark_ctx* ctx);                                   // makes the context's device current (every entry point)
void comm_destroy(stark_ctx* ctx);
void ntt_set_attrs();                                                // per-device kernel attributes of the NTT kernels (capi_ntt.hip)
void ntt_plans_free(stark_ctx* ctx);

}  // namespace stark
