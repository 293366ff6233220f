// stark_mlwe_amd/csrc/capi_core.hip — context lifetime, the pooled allocator, options, memcpy / timers, the Poseidon parameter sets.
// C-ABI declared in include/stark_mlwe.h.  The Poseidon / Merkle entry points and their kernels: capi_poseidon.hip.
#include <algorithm>
#include <cstring>
#include "poseidon_launch.hpp"
#include "pow_table.hpp"   // stark_ctx::omega_tabs is destroyed with the context

using namespace stark;

namespace stark {

// Option "pool_poison" (tests only): `bytes` at p become the fill byte before the allocator hands p out.  The fill is enqueued on the context's stream
// and the host waits for it: a block allocated between ctx_fork and ctx_join is first touched on the SIDE stream, which is not ordered after a memset
// enqueued later on the main one — because the allocator returns only once the fill has landed, every later launch on either stream sees it.
static int32_t pool_poison_fill(stark_ctx* ctx, void* p, size_t bytes) {
    STARK_HIP(ctx, hipMemsetAsync(p, ctx->opt.pool_poison, bytes, ctx->stream));
    STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return STARK_OK;
}

int32_t ctx_scratch(stark_ctx* ctx, size_t bytes, void** out) {
    if (bytes > ctx->scratch_bytes) {
        if (ctx->scratch) STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->scratch_bytes = 0; STARK_HIP(ctx, ctx->scratch.alloc(ctx, bytes)); ctx->scratch_bytes = bytes;      // alloc frees the smaller block first
    }
    if (ctx->opt.pool_poison >= 0 && ctx->scratch_bytes) STARK_TRY(pool_poison_fill(ctx, ctx->scratch.p, ctx->scratch_bytes));
    *out = ctx->scratch.p; return STARK_OK;
}

int32_t ctx_upload_staged(stark_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!bytes) return STARK_OK;
    auto& q = ctx->staged;
    for (size_t i = 0; i < q.size();) {                                     // uploads the stream has passed: their host copies go
        if (hipEventQuery(q[i].done) == hipSuccess) { (void)hipEventDestroy(q[i].done); q[i] = std::move(q.back()); q.pop_back(); } else ++i;
    }
    (void)hipGetLastError();                                                // hipErrorNotReady of the queries is not an error
    stark_ctx::StagedUpload u; u.host.reset(new uint8_t[bytes]); memcpy(u.host.get(), src, bytes);
    STARK_HIP(ctx, hipEventCreateWithFlags(&u.done, hipEventDisableTiming));
    const uint8_t* from = u.host.get();
    q.push_back(std::move(u));                                              // owned from here on, whatever fails below (teardown synchronises first)
    STARK_HIP(ctx, hipMemcpyAsync(dst, from, bytes, hipMemcpyHostToDevice, ctx->stream));
    STARK_HIP(ctx, hipEventRecord(q.back().done, ctx->stream));
    return STARK_OK;
}

// ---- caching device allocator (stark_ctx::pool_free) ----------------------------------------------------------
static inline size_t pool_round(size_t bytes) {
    if (bytes < 256) return 256;
    if (bytes <= (1u << 20)) { size_t r = 256; while (r < bytes) r <<= 1; return r; }       // small: powers of two
    return (bytes + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);                             // large: whole MiB (layer / level sizes repeat exactly)
}
// The refusal hook (TESTS ONLY, stark_ctx::alloc_hook; called only while it is on).  `counted`: this event is one the current mode counts.
// True: the event is the armed one and is refused; the hook disarms itself and goes on counting.
static bool alloc_hook_fires(stark_ctx* ctx, bool counted) {
    stark_ctx::AllocHook& h = ctx->alloc_hook;
    if (!counted || ++h.requests != h.at) return false;
    h.at = 0; ++h.fired; return true;
}
hipError_t dev_malloc(stark_ctx* ctx, void** out, size_t bytes, DevMallocKind kind) {
    *out = nullptr;
    if (ctx->alloc_hook.mode) {
        stark_ctx::AllocHook& h = ctx->alloc_hook;
        if (kind == kDevPoolRetry) { if (h.refuse_retry) { h.refuse_retry = false; return hipErrorOutOfMemory; } }      // mode 3: the second attempt of the refused miss
        else if (alloc_hook_fires(ctx, h.mode == 1 ? kind == kDevTable : kind == kDevPoolFirst)) { h.refuse_retry = h.mode == 3; return hipErrorOutOfMemory; }
    }
    const hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) { *out = nullptr; (void)hipGetLastError(); }      // nothing stays behind for the hipGetLastError of a later launch
    return e;
}
int32_t ctx_alloc(stark_ctx* ctx, size_t bytes, void** out) {
    const size_t sz = pool_round(bytes);
    // a refused request fails as the second attempt below does, without the give-back (which synchronises the stream: the refusal is also used behind a busy one)
    if (ctx->alloc_hook.mode == 1 && alloc_hook_fires(ctx, true)) return ctx->fail(STARK_ERR_OOM, "device allocation of " + std::to_string(sz) + " bytes failed");
    auto it = ctx->pool_free.find(sz);
    if (it != ctx->pool_free.end() && !it->second.empty()) {
        void* p = it->second.back(); it->second.pop_back(); ctx->pool_cached_bytes -= sz;
        ctx->pool_live[p] = sz; *out = p;
        return ctx->opt.pool_poison >= 0 ? pool_poison_fill(ctx, p, sz) : STARK_OK;       // the whole rounded block, not only `bytes`
    }
    void* p = nullptr; hipError_t e = dev_malloc(ctx, &p, sz, kDevPoolFirst);
    if (e != hipSuccess) {                                       // out of memory: give the cached blocks back and retry once
        (void)hipStreamSynchronize(ctx->stream);
        for (auto& kv : ctx->pool_free) { for (void* q : kv.second) { (void)hipFree(q); ctx->pool_cached_bytes -= kv.first; } kv.second.clear(); }
        if (ctx->alloc_hook.mode) ctx->alloc_hook.cached_after_give_back = ctx->pool_cached_bytes;       // the accounting's own result: 0 when every cached block was counted once
        e = dev_malloc(ctx, &p, sz, kDevPoolRetry);
        if (e != hipSuccess) return ctx->fail(STARK_ERR_OOM, "device allocation of " + std::to_string(sz) + " bytes failed");
    }
    ctx->pool_live[p] = sz; *out = p;
    return ctx->opt.pool_poison >= 0 ? pool_poison_fill(ctx, p, sz) : STARK_OK;
}
void ctx_release(stark_ctx* ctx, void* p) {
    if (!p || !ctx) return;
    auto it = ctx->pool_live.find(p);
    if (it == ctx->pool_live.end()) { ctx->err = "ctx_release: the pointer is not a live block of this context's pool (left alone)"; return; }   // never hipFree: the pool may still list it
    const size_t sz = it->second; ctx->pool_live.erase(it);
    ctx->pool_free[sz].push_back(p); ctx->pool_cached_bytes += sz;
}
int32_t ctx_enter(stark_ctx* ctx) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != ctx->device) STARK_HIP(ctx, hipSetDevice(ctx->device));
    return STARK_OK;
}

int32_t ctx_side_stream(stark_ctx* ctx, hipStream_t* out) {
    if (!ctx->side_stream) { STARK_HIP(ctx, hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking)); STARK_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming)); }
    *out = ctx->side_stream; return STARK_OK;
}
int32_t ctx_fork(stark_ctx* ctx, hipStream_t* side) {
    STARK_TRY(ctx_side_stream(ctx, side));
    if (hipEventRecord(ctx->ev_fork, ctx->stream) != hipSuccess || hipStreamWaitEvent(*side, ctx->ev_fork, 0) != hipSuccess) return ctx->fail(STARK_ERR_HIP, "fork");
    return STARK_OK;
}
int32_t ctx_join(stark_ctx* ctx) {
    if (hipEventRecord(ctx->ev_fork, ctx->side_stream) != hipSuccess || hipStreamWaitEvent(ctx->stream, ctx->ev_fork, 0) != hipSuccess) return ctx->fail(STARK_ERR_HIP, "join");
    return STARK_OK;
}

static int32_t params_finish(stark_ctx* ctx, stark_params* P) {
    if (host::rp_for_width(P->ref.t) < 0) return ctx->fail(STARK_ERR_UNSUPPORTED, "Poseidon width must be one of 9,17,33,65,129");
    P->kc = host::make_kernel_consts(P->ref);
    if (!P->kc.ok) return ctx->fail(STARK_ERR_UNSUPPORTED, "MDS matrix has a singular leading minor: LU/sparse kernel form unavailable");
    const host::KernelConsts& k = P->kc;
    std::vector<fr_t> blob; auto put = [&](const std::vector<fr_t>& v) { size_t off = blob.size(); blob.insert(blob.end(), v.begin(), v.end()); return off; };
    size_t o_rcf = put(k.rc_full), o_rcp = put(k.rc_partial), o_lu = put(k.lu), o_pre = put(k.lu_pre), o_row0 = put(k.row0), o_sp = put(k.sparse), o_mds = put(k.mds), o_mpre = put(k.mds_pre), o_gam = put(k.gamma);
    // radix-2^29 multiplier tables (fr29.hpp), appended to the same device blob as raw words
    const size_t o_29 = blob.size();
    { std::vector<uint32_t> w29; for (auto* v : {&k.lu29, &k.lu_pre29, &k.row0_29, &k.sparse29, &k.gamma29, &k.mds29, &k.mds_pre29, &k.chain_a, &k.chain_g, &k.chain_w, &k.rc_full29}) w29.insert(w29.end(), v->begin(), v->end());
      while (w29.size() % 8) w29.push_back(0);
      blob.resize(o_29 + w29.size() / 8); memcpy((void*)(blob.data() + o_29), w29.data(), w29.size() * 4); }
    // int8 MFMA fragments of the dense matrices (t = 17), raw bytes in the same blob
    const size_t o_frag = blob.size(), frag_elems = (k.mds_frag.size() + sizeof(fr_t) - 1) / sizeof(fr_t);
    if (!k.mds_frag.empty()) { blob.resize(o_frag + 2 * frag_elems); memcpy((void*)(blob.data() + o_frag), k.mds_frag.data(), k.mds_frag.size()); memcpy((void*)(blob.data() + o_frag + frag_elems), k.mds_pre_frag.data(), k.mds_pre_frag.size()); }
    // The 8-round partial blocks (t = 17, rp % 8 == 0, M[0][0] != 0), the SCALED family (host_util.hpp blk8s_*): int8 MFMA fragments of the E-product, of the lane
    // product followed by the shared unit fragment, of the Gamma terms; then the scaled round constants as nine limbs each (rc_partial_scaled29) with the unscale multiplier right behind them (PoseidonDev::blk8_unscale29).  The unscaled family stays on the
    // host.  Owned and freed with the set.
    const size_t o_b8 = blob.size(), ef_elems = (k.blk8s_efrag.size() + sizeof(fr_t) - 1) / sizeof(fr_t), lf_bytes = k.blk8s_lfrag.size() + 1024, lf_elems = (lf_bytes + sizeof(fr_t) - 1) / sizeof(fr_t),
                 gf_elems = (k.blk8s_gfrag.size() + sizeof(fr_t) - 1) / sizeof(fr_t), rcs_words = k.rc_partial_scaled29.size(), un_elems = ((rcs_words + k.blk8_unscale29.size()) * 4 + sizeof(fr_t) - 1) / sizeof(fr_t);      // the constants' limbs and the unscale multiplier, contiguous words
    const bool have_b8 = !k.blk8s_efrag.empty();
    if (have_b8) { blob.resize(o_b8 + ef_elems + lf_elems + gf_elems + un_elems);
                   int8_t* const b8 = (int8_t*)(blob.data() + o_b8);
                   memcpy(b8, k.blk8s_efrag.data(), k.blk8s_efrag.size());
                   memcpy(b8 + ef_elems * sizeof(fr_t), k.blk8s_lfrag.data(), k.blk8s_lfrag.size()); memcpy(b8 + ef_elems * sizeof(fr_t) + k.blk8s_lfrag.size(), k.blk8_lfrag.data() + k.blk8_lfrag.size() - 1024, 1024);
                   memcpy(b8 + (ef_elems + lf_elems) * sizeof(fr_t), k.blk8s_gfrag.data(), k.blk8s_gfrag.size());
                   memcpy(b8 + (ef_elems + lf_elems + gf_elems) * sizeof(fr_t), k.rc_partial_scaled29.data(), rcs_words * 4);
                   memcpy(b8 + (ef_elems + lf_elems + gf_elems) * sizeof(fr_t) + rcs_words * 4, k.blk8_unscale29.data(), k.blk8_unscale29.size() * 4); }
    STARK_TRY(P->blob.fill_sync(ctx, blob.data(), blob.size() * sizeof(fr_t)));
    fr_t* const dev = P->blob.fr();
    P->dev.t = k.t; P->dev.rf = k.rf; P->dev.rp = k.rp;
    P->dev.rc_full = dev + o_rcf; P->dev.rc_partial = dev + o_rcp; P->dev.lu = dev + o_lu; P->dev.lu_pre = dev + o_pre;
    P->dev.row0 = dev + o_row0; P->dev.sparse = dev + o_sp; P->dev.mds = dev + o_mds; P->dev.mds_pre = dev + o_mpre; P->dev.gamma = dev + o_gam;
    { const uint32_t* b29 = reinterpret_cast<const uint32_t*>(dev + o_29);
      P->dev.lu29 = b29; P->dev.lu_pre29 = b29 + k.lu29.size(); P->dev.row0_29 = P->dev.lu_pre29 + k.lu_pre29.size();
      P->dev.sparse29 = P->dev.row0_29 + k.row0_29.size(); P->dev.gamma29 = P->dev.sparse29 + k.sparse29.size();
      P->dev.mds29 = P->dev.gamma29 + k.gamma29.size(); P->dev.mds_pre29 = P->dev.mds29 + k.mds29.size();
      const uint32_t* ch = P->dev.mds_pre29 + k.mds_pre29.size();
      P->dev.chain_a = k.chain_a.empty() ? nullptr : ch; P->dev.chain_g = k.chain_a.empty() ? nullptr : ch + k.chain_a.size(); P->dev.chain_w = k.chain_a.empty() ? nullptr : ch + k.chain_a.size() + k.chain_g.size();
      P->dev.rc_full29 = ch + k.chain_a.size() + k.chain_g.size() + k.chain_w.size(); }
    P->dev.blk8_efrag = have_b8 ? (const void*)(dev + o_b8) : nullptr; P->dev.blk8_lfrag = have_b8 ? (const void*)(dev + o_b8 + ef_elems) : nullptr;
    P->dev.blk8_gfrag = have_b8 ? (const void*)(dev + o_b8 + ef_elems + lf_elems) : nullptr;
    P->dev.blk8_unit_frag = have_b8 ? (const void*)((const int8_t*)P->dev.blk8_lfrag + k.blk8s_lfrag.size()) : nullptr;
    P->dev.rc_partial_scaled29 = have_b8 ? reinterpret_cast<const uint32_t*>(dev + o_b8 + ef_elems + lf_elems + gf_elems) : nullptr;
    P->dev.mds_frag = k.mds_frag.empty() ? nullptr : (const void*)(dev + o_frag); P->dev.mds_pre_frag = k.mds_frag.empty() ? nullptr : (const void*)(dev + o_frag + frag_elems);
    return STARK_OK;
}
static int32_t params_from_consts(stark_ctx* ctx, const host::PoseidonConsts& c, std::unique_ptr<stark_params>& out) {
    std::unique_ptr<stark_params> P(new stark_params()); P->ctx = ctx; P->ref = c;
    STARK_TRY(params_finish(ctx, P.get()));
    out = std::move(P); return STARK_OK;
}
// a set handed to the caller keeps the context alive
static int32_t params_for_caller(stark_ctx* ctx, const host::PoseidonConsts& c, stark_params** out) {
    std::unique_ptr<stark_params> P; STARK_TRY(params_from_consts(ctx, c, P));
    P->ref_.bind(ctx); *out = P.release(); return STARK_OK;
}
int32_t ctx_transcript_params(stark_ctx* ctx, stark_params** out) {
    if (!ctx->tparams) STARK_TRY(params_from_consts(ctx, host::consts_transcript(), ctx->tparams));
    if (out) *out = ctx->tparams.get();
    return STARK_OK;
}
int32_t ctx_merkle_params(stark_ctx* ctx, int t, stark_params** out) {
    auto it = ctx->merkle_params.find(t);
    if (it == ctx->merkle_params.end()) {
        if (host::rp_for_width(t) < 0) return ctx->fail(STARK_ERR_UNSUPPORTED, "unsupported Poseidon width");
        std::unique_ptr<stark_params> P; STARK_TRY(params_from_consts(ctx, host::consts_for_width(t), P));
        *out = P.get(); ctx->merkle_params[t] = std::move(P); return STARK_OK;
    }
    *out = it->second.get(); return STARK_OK;
}
// MerkleCommitment's parameters (commitment/src/lib.rs:48-51: generate_params_t17_x5 of "POSEIDON-T17-X5-SEED"), cached next to the other sets
// under key -17; like them it does not pin the context
int32_t ctx_commit_params(stark_ctx* ctx, stark_params** out) {
    std::unique_ptr<stark_params>& slot = ctx->merkle_params[-17];
    if (!slot) STARK_TRY(params_from_consts(ctx, host::derive_consts("POSEIDON-T17-X5-SEED", 17, 8, 64), slot));
    *out = slot.get(); return STARK_OK;
}

}  // namespace stark

extern "C" {

int32_t stark_version(void) { return 1; }

int32_t stark_ctx_create(int32_t device, void* stream, stark_ctx_t** out) {
    if (!out) return STARK_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return STARK_ERR_HIP;   // no device => no product path
    if (hipSetDevice(device) != hipSuccess) return STARK_ERR_HIP;
    std::unique_ptr<stark_ctx> c(new stark_ctx()); c->device = device;
    if (stream == STARK_STREAM_PRIVATE) { if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return STARK_ERR_HIP; c->own_stream = true; }
    else { c->stream = (hipStream_t)stream; c->own_stream = false; }         // NULL = the device's legacy default stream (ordered against torch's default stream and every blocking stream)
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) return STARK_ERR_HIP;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->num_cus = cus; }
    stark::ntt_set_attrs();
    stark::poseidon_set_attrs();
    *out = c.release(); return STARK_OK;
}
}  // extern "C"
// everything the context owns; runs when the context has been destroyed AND its last handle is gone
static void ctx_teardown(stark_ctx* ctx) {
    (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream);
    stark::comm_destroy(ctx);
    stark::ntt_plans_free(ctx);
    for (auto& kv : ctx->pool_free) for (void* q : kv.second) (void)hipFree(q);
    for (auto& kv : ctx->pool_live) (void)hipFree(kv.first);                 // blocks whose owner leaked (every handle is gone by now)
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    for (auto& u : ctx->staged) (void)hipEventDestroy(u.done);               // the stream was synchronised above: every staged upload is done
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0); if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;                                                               // the DevMem members, the cached parameter sets and the power-table cache free themselves here, the device still current
}
namespace stark {
void ctx_ref(stark_ctx* c) { ++c->live_handles; }
void ctx_unref(stark_ctx* c) { if (--c->live_handles == 0 && c->destroy_pending) ctx_teardown(c); }
}
extern "C" {
// With handles still alive (trees, FRI states, plans, transcripts, parameter sets made for the caller) the context is only MARKED here: it stops
// accepting new work through stark_ctx_* but stays valid for those handles, and the last of them to be freed tears it down.
int32_t stark_ctx_destroy(stark_ctx_t* ctx) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (ctx->destroy_pending) return STARK_ERR_INVALID_ARG;                  // destroyed twice
    STARK_TRY(ctx_enter(ctx));
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->live_handles > 0) { ctx->destroy_pending = true; return STARK_OK; }
    ctx_teardown(ctx); return STARK_OK;
}
int32_t stark_ctx_sync(stark_ctx_t* ctx) { if (!ctx) return STARK_ERR_INVALID_ARG; STARK_TRY(ctx_enter(ctx)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream)); return STARK_OK; }
int32_t stark_ctx_trim(stark_ctx_t* ctx) {
    if (!ctx) return STARK_ERR_INVALID_ARG; STARK_TRY(ctx_enter(ctx));
    STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& kv : ctx->pool_free) { for (void* q : kv.second) (void)hipFree(q); kv.second.clear(); }
    ctx->pool_cached_bytes = 0;
    stark::ntt_plans_free(ctx);                  // NTT plans with their direct twiddle / coset tables (up to 3*n*32 B per plan) are rebuilt on demand
    ctx->scratch.reset(); ctx->scratch_bytes = 0;
    return STARK_OK;
}
size_t stark_ctx_cached_bytes(stark_ctx_t* ctx) { return ctx ? ctx->pool_cached_bytes : 0; }
}  // extern "C"
// The options of stark_ctx_set_option: the key, and what a value does to the context's options (the accepted range when it is refused).
struct OptionDef { const char* key; const char* (*set)(stark_ctx::Options&, int64_t); };
static const OptionDef kOptions[] = {
    {"ntt_direct_max_log", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < 0 || v > 30) return "0..30"; o.ntt_direct_max_log = (int)v; return nullptr; }},
    {"ntt_merged_coset", [](stark_ctx::Options& o, int64_t v) -> const char* { o.ntt_merged_coset = v != 0; return nullptr; }},
    {"ntt_log_tile", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v != -1 && (v < 8 || v > 12)) return "8..12, or -1 for the default"; o.ntt_log_tile_forced = v != -1; o.ntt_log_tile = v == -1 ? 11 : (int)v; return nullptr; }},
    {"ntt_min_waves", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v != 2 && v != 4) return "2 or 4"; o.ntt_min_waves = (int)v; return nullptr; }},
    {"poseidon_lane_only", [](stark_ctx::Options& o, int64_t v) -> const char* { o.poseidon_lane_only = v != 0; return nullptr; }},
    {"sponge_one_wave", [](stark_ctx::Options& o, int64_t v) -> const char* { o.sponge_one_wave = v != 0; return nullptr; }},
    {"sponge_debug", [](stark_ctx::Options& o, int64_t v) -> const char* { o.sponge_debug = (int)v; return nullptr; }},
    {"merkle_node16_pair", [](stark_ctx::Options& o, int64_t v) -> const char* { o.merkle_node16_pair = v != 0; return nullptr; }},
    {"poseidon_block8", [](stark_ctx::Options& o, int64_t v) -> const char* { o.poseidon_block8 = v != 0; return nullptr; }},
    {"merkle_wave_pair", [](stark_ctx::Options& o, int64_t v) -> const char* { o.merkle_wave_pair = v != 0; return nullptr; }},
    {"fri_side_pair", [](stark_ctx::Options& o, int64_t v) -> const char* { o.fri_side_pair = v != 0; return nullptr; }},
    {"sumcheck_verify_batch_max_slots", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < 1) return "at least 1"; o.sumcheck_verify_batch_max_slots = (size_t)v; return nullptr; }},
    {"ntt_batch_max_elems", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < 1 || v > ((int64_t)1 << 28)) return "1..2^28"; o.ntt_batch_max_elems = (size_t)v; return nullptr; }},
    {"prove_batch_max_rows", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < 1 || v > ((int64_t)1 << 28)) return "1..2^28"; o.prove_batch_max_rows = (size_t)v; return nullptr; }},
    {"mle_log_tile", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v != -1 && (v < 3 || v > 12)) return "3..12, or -1 for the default"; o.mle_log_tile = (int)v; return nullptr; }},
    {"mle_lane_contiguous", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < -1 || v > 1) return "0 or 1, or -1 for the default"; o.mle_lane_contiguous = (int)v; return nullptr; }},
    {"lagrange_max_partials", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v != -1 && (v < 1 || v > ((int64_t)1 << 28))) return "1..2^28, or -1 for the default"; o.lagrange_max_partials = v == -1 ? (size_t)1 << 21 : (size_t)v; return nullptr; }},
    {"lagrange_wide_acc", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < -1 || v > 1) return "0 or 1, or -1 for the default"; o.lagrange_wide_acc = (int)v; return nullptr; }},
    {"lagrange_col_groups", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v != -1 && (v < 1 || v > 65535)) return "1..65535, or -1 for automatic"; o.lagrange_col_groups = (int)v; return nullptr; }},
    {"lagrange_shared_inverse", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < -1 || v > 1) return "0 or 1, or -1 for the default"; o.lagrange_shared_inverse = v == 1; return nullptr; }},
    {"lagrange_share_cosets", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < -1 || v > 1) return "0 or 1, or -1 for the default"; o.lagrange_share_cosets = v == 1; return nullptr; }},
    {"mixed_prove_tail", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < -1 || v > 1) return "0 or 1, or -1 for the default"; o.mixed_prove_tail = v == 1; return nullptr; }},
    {"pool_poison", [](stark_ctx::Options& o, int64_t v) -> const char* { if (v < -1 || v > 255) return "0..255, or -1 for off"; o.pool_poison = (int)v; return nullptr; }},
};
extern "C" {
int32_t stark_ctx_set_option(stark_ctx_t* ctx, const char* key, int64_t value) {
    if (!ctx || !key) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const std::string k(key);
    const OptionDef* def = nullptr; std::string known;
    for (const OptionDef& d : kOptions) { if (k == d.key) def = &d; known += (known.empty() ? "" : ", ") + std::string(d.key); }
    if (!def) return ctx->fail(STARK_ERR_INVALID_ARG, "unknown option '" + k + "' (" + known + ")");
    if (const char* range = def->set(ctx->opt, value)) return ctx->fail(STARK_ERR_INVALID_ARG, k + ": " + range);
    STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    stark::ntt_plans_free(ctx);                  // plans (and their direct tables) are rebuilt lazily under the new options
    return STARK_OK;
}
const char* stark_last_error(stark_ctx_t* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
int32_t stark_malloc(stark_ctx_t* ctx, size_t bytes, void** dptr) { if (!ctx || !dptr) return STARK_ERR_INVALID_ARG; STARK_TRY(ctx_enter(ctx)); STARK_HIP(ctx, hipMalloc(dptr, bytes ? bytes : 32)); return STARK_OK; }
int32_t stark_free(stark_ctx_t* ctx, void* dptr) { if (!ctx) return STARK_ERR_INVALID_ARG; STARK_TRY(ctx_enter(ctx)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream)); STARK_HIP(ctx, hipFree(dptr)); return STARK_OK; }
int32_t stark_memcpy_h2d(stark_ctx_t* ctx, void* d, const void* s, size_t bytes) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return DevMem::fill_sync(ctx, d, s, bytes); }
int32_t stark_memcpy_d2h(stark_ctx_t* ctx, void* d, const void* s, size_t bytes) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    STARK_HIP(ctx, hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream)); return STARK_OK; }
int32_t stark_timer_start(stark_ctx_t* ctx) { if (!ctx) return STARK_ERR_INVALID_ARG; STARK_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream)); return STARK_OK; }
int32_t stark_timer_stop_ms(stark_ctx_t* ctx, float* ms) {
    if (!ctx || !ms) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    STARK_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream)); STARK_HIP(ctx, hipEventSynchronize(ctx->ev1)); STARK_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1)); return STARK_OK; }

// ---- diagnostics: the integer-VALU "speed of light" of this device, measured live -----------------------
}  // extern "C"
// 8 independent v_mad_u64_u32 chains per lane (the primitive of every field product here); 4 waves per SIMD.
#define STARK_DIAG_ITERS 2048
static __global__ void __launch_bounds__(1024) k_diag_mac_rate(uint32_t* out, uint32_t seed) {
    uint32_t a0 = seed + threadIdx.x, a1 = a0 * 3 + 1, a2 = a0 * 5 + 2, a3 = a0 * 7 + 3, a4 = a0 * 9 + 4, a5 = a0 * 11 + 5, a6 = a0 * 13 + 6, a7 = a0 * 15 + 7;
    uint64_t d0 = a0, d1 = a1, d2 = a2, d3 = a3, d4 = a4, d5 = a5, d6 = a6, d7 = a7; const uint32_t b = seed | 1;
#define STARK_DIAG_MAD(i) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(d##i) : "v"(a##i), "v"(b) : "vcc");
    for (int i = 0; i < STARK_DIAG_ITERS; ++i) { STARK_DIAG_MAD(0) STARK_DIAG_MAD(1) STARK_DIAG_MAD(2) STARK_DIAG_MAD(3) STARK_DIAG_MAD(4) STARK_DIAG_MAD(5) STARK_DIAG_MAD(6) STARK_DIAG_MAD(7) }
#undef STARK_DIAG_MAD
    out[blockIdx.x * blockDim.x + threadIdx.x] = (uint32_t)(d0 ^ d1 ^ d2 ^ d3 ^ d4 ^ d5 ^ d6 ^ d7);
}
extern "C" {
int32_t stark_diag_mac_rate(stark_ctx_t* ctx, double* lane_macs_per_s) {
    if (!ctx || !lane_macs_per_s) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    hipDeviceProp_t prop; STARK_HIP(ctx, hipGetDeviceProperties(&prop, ctx->device));
    const int blocks = prop.multiProcessorCount * 2, threads = 1024;        // 2 x 16 waves per CU = 8 waves per SIMD resident, issue-bound either way
    DevBuf o; STARK_HIP(ctx, o.alloc(ctx, (size_t)blocks * threads * 4));
    hipLaunchKernelGGL(k_diag_mac_rate, dim3(blocks), dim3(threads), 0, ctx->stream, (uint32_t*)o.p, 12345u);       // warm-up (clocks, code object)
    STARK_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(k_diag_mac_rate, dim3(blocks), dim3(threads), 0, ctx->stream, (uint32_t*)o.p, 12345u);
    STARK_HIP(ctx, hipGetLastError());
    STARK_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream)); STARK_HIP(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0; STARK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *lane_macs_per_s = (double)blocks * threads * 8.0 * STARK_DIAG_ITERS / (ms * 1e-3);
    return STARK_OK;
}

// TESTS ONLY: the allocation-refusal hook (stark_ctx::alloc_hook).  stats (optional) first receives requests counted since the last arming, refusals
// fired since then, live pooled blocks, live pooled bytes, the cached bytes right after the last give-back (~0: none yet); then mode 1 / 2 / 3 arm the hook for event number nth (0: count only), 0 disarms and stops
// counting, -1 leaves the hook as it is (a read).  Touches neither the stream nor the NTT plans.
int32_t stark_diag_alloc_refusal(stark_ctx_t* ctx, int32_t mode, uint64_t nth, uint64_t* stats) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (mode < -1 || mode > 3) return ctx->fail(STARK_ERR_INVALID_ARG, "alloc refusal mode: -1 (read), 0 (off), 1 (refuse request nth), 2 (refuse the first attempt of pool miss nth), 3 (refuse both attempts of pool miss nth)");
    if (stats) {
        stats[0] = ctx->alloc_hook.requests; stats[1] = ctx->alloc_hook.fired; stats[2] = ctx->pool_live.size(); stats[3] = 0;
        for (const auto& kv : ctx->pool_live) stats[3] += kv.second;
        stats[4] = ctx->alloc_hook.cached_after_give_back;
    }
    if (mode >= 0) { ctx->alloc_hook = stark_ctx::AllocHook(); ctx->alloc_hook.mode = mode; ctx->alloc_hook.at = mode ? nth : 0; }
    return STARK_OK;
}

// ---- constants ---------------------------------------------------------------------------------------
int32_t stark_poseidon_params_upload(stark_ctx_t* ctx, int32_t t, int32_t rf, int32_t rp, const uint64_t* mds, const uint64_t* rc_full, const uint64_t* rc_partial, stark_params_t** out) {
    if (!ctx || !mds || !rc_full || !rc_partial || !out || t < 2 || rf <= 0 || (rf & 1) || rp <= 0) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad params") : STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    host::PoseidonConsts c; c.t = t; c.rf = rf; c.rp = rp;
    c.mds.resize((size_t)t * t); c.rc_full.resize((size_t)rf * t); c.rc_partial.resize(rp);
    for (size_t i = 0; i < c.mds.size(); ++i) c.mds[i] = load_fr(mds + 4 * i);
    for (size_t i = 0; i < c.rc_full.size(); ++i) c.rc_full[i] = load_fr(rc_full + 4 * i);
    for (size_t i = 0; i < c.rc_partial.size(); ++i) c.rc_partial[i] = load_fr(rc_partial + 4 * i);
    return params_for_caller(ctx, c, out);
}
int32_t stark_poseidon_params_for_width(stark_ctx_t* ctx, int32_t t, stark_params_t** out) {
    if (!ctx || !out) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (host::rp_for_width(t) < 0) return ctx->fail(STARK_ERR_UNSUPPORTED, "unsupported Poseidon width t; supported t in {9,17,33,65,129}");   // poseidon/src/lib.rs:127
    return params_for_caller(ctx, host::consts_for_width(t), out);
}
int32_t stark_poseidon_params_t17_seed(stark_ctx_t* ctx, const uint8_t* seed, size_t n, stark_params_t** out) {
    if (!ctx || !out || (!seed && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return params_for_caller(ctx, host::derive_consts(std::string((const char*)seed, n), 17, 8, 64), out);
}
int32_t stark_poseidon_params_export(stark_params_t* p, int32_t* t, int32_t* rf, int32_t* rp, uint64_t* mds, uint64_t* rc_full, uint64_t* rc_partial) {
    if (!p) return STARK_ERR_INVALID_ARG;
    if (t) *t = p->ref.t; if (rf) *rf = p->ref.rf; if (rp) *rp = p->ref.rp;
    if (mds) for (size_t i = 0; i < p->ref.mds.size(); ++i) store_fr(mds + 4 * i, p->ref.mds[i]);
    if (rc_full) for (size_t i = 0; i < p->ref.rc_full.size(); ++i) store_fr(rc_full + 4 * i, p->ref.rc_full[i]);
    if (rc_partial) for (size_t i = 0; i < p->ref.rc_partial.size(); ++i) store_fr(rc_partial + 4 * i, p->ref.rc_partial[i]);
    return STARK_OK;
}
int32_t stark_poseidon_params_free(stark_params_t* p) { if (!p) return STARK_ERR_INVALID_ARG; delete p; return STARK_OK; }

}  // extern "C"
