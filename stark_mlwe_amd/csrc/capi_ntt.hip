// stark_mlwe_amd/csrc/capi_ntt.hip — NTT / iNTT / LDE entry points and plans (crates/fft/src/lib.rs:6-32),
// the per-GPU building blocks of the multi-GPU six-step NTT, and the synthetic-input generator.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "pow_table.hpp"
#include "ntt_mixed_plan.hpp"
#include "fri_dev.hpp"
#include "shard_coll.hpp"

using namespace stark;

namespace stark {

// What a plan holds for ONE coset value at a time (build_coset): only `tab` is required, the optional tables save products or table reads.
struct NttCoset {
    bool have = false; fr_t g;
    DevPowTable tab;              // two-level table of the pre-scale g^j (forward plans) or of the post-scale n^-1 g^-k (inverse plans)
    DevMem direct;                // the pre-scale as ONE table (log_n <= 24)
    // merged form for plans with a strided first pass: (g^S)^p by point + the first pass's twiddles times g^rest (one full-length table read less per element)
    DevMem small, tw_direct;
};
struct NttPlan {
    int field = 0, log_n = 0; bool inverse = false;
    int P = 1; int log_b[3] = {0, 0, 0};
    DevMem stage_tw[3];           // w_B^(+-e), e < B/2 per pass
    DevPowTable root;             // powers of w_N^(+-1)
    DevMem scale;                 // n^-1 (inverse plans)
    DevMem tw_direct[2];          // direct tables (log_n <= 24): inter-pass twiddles of the strided passes
    NttCoset coset;
    // power tables of coset shifts used by the multi-GPU column phase (a handful: the 2^log_blowup cosets of an LDE)
    PowCache shift_tabs{32};
    // plain (c0 = 1) power tables for the element-wise kernels of stark_ntt_rows_coset_dev: coset shifts, and w_N itself
    PowCache plain_tabs{40};
};

}  // namespace stark

static const size_t kMaxLds = 160 * 1024;
// direct (one-product) twiddle / coset tables for transforms up to 2^ntt_direct_max_log points (option, default 24; 0 disables): they cost
// n*32 B of HBM per strided pass and plan, which the VALU-bound transform does not notice, and save a product per element and pass
static inline int ntt_direct_max(const stark_ctx* ctx) { return ctx->opt.ntt_direct_max_log; }

// The NTT kernels multiply by table entries with ONE Montgomery step by 2^261 on nine-limb values (ntt_dev.hpp): every table
// of a plan carries the factor 32 that makes that step a product in the 2^256 domain.
template <class F> static inline fr_t x32(const fr_t& v) { return fr_mul<F>(v, fr_from_u64<F>(32)); }
// the two-level split of a table of 2^log_n powers
static inline int tab_lo(int log_n) { return (log_n + 1) / 2; }
static inline int tab_hi(int log_n) { return log_n - tab_lo(log_n); }
// The one dispatch on the C-ABI's field id: fn receives the field as a tag value (`using F = decltype(f)`).
template <class Fn> static int32_t with_field(stark_ctx* ctx, int32_t field_id, Fn fn) {
    if (field_id == STARK_FIELD_PALLAS_FR) return fn(PallasFr{});
    if (field_id == STARK_FIELD_BLS12_381_FR) return fn(Bls12381Fr{});
    return ctx->fail(STARK_ERR_INVALID_ARG, "unknown field id");
}
// One field element as a device constant (a scale word of ntt_run): a staged upload into a pooled word that goes back to the pool, in stream
// order, with this object.
struct DevWord {
    DevBuf dev;
    int32_t set(stark_ctx* ctx, const fr_t& v) { STARK_HIP(ctx, dev.alloc(ctx, sizeof(fr_t))); return ctx_upload_staged(ctx, dev.p, &v, sizeof(fr_t)); }
};

// THE optional allocations of the library: the direct tables of a plan (get_plan: tw_direct[i]) and of its coset (build_coset: small, tw_direct,
// direct).  One that cannot be had does not fail the transform — the pass kernels fall back to the two-level lookup — and leaves this note, not
// an error, where stark_last_error reads: the call still returns STARK_OK.  Every other allocation of the library fails its call.
static void optional_table_note(stark_ctx* ctx, const char* which, int log_n) {
    ctx->err = std::string("optional NTT table ") + which + " of 2^" + std::to_string(log_n) + " points not allocated: the transform uses the two-level lookup";
}
template <class F>
static int32_t get_plan(stark_ctx* ctx, int log_n, bool inverse, NttPlan** out) {
    uint64_t key = ((uint64_t)F::ID << 40) | ((uint64_t)log_n << 8) | (inverse ? 1 : 0);
    auto it = ctx->plans.find(key);
    if (it != ctx->plans.end()) { *out = it->second; return STARK_OK; }
    std::unique_ptr<NttPlan> p(new NttPlan()); p->field = F::ID; p->log_n = log_n; p->inverse = inverse;
    p->P = ntt_split(log_n, p->log_b);
    fr_t w = fr_root_of_unity<F>((unsigned)log_n); if (inverse) w = fr_inv<F>(w);
    STARK_TRY(p->root.fill<F>(ctx, w, x32<F>(fr_one<F>()), tab_lo(log_n), tab_hi(log_n)));
    for (int i = 0; i < p->P; ++i) {
        int lb = p->log_b[i]; fr_t wb = fr_root_of_unity<F>((unsigned)lb); if (inverse) wb = fr_inv<F>(wb);
        DevPowTable T; STARK_TRY(T.fill<F>(ctx, wb, x32<F>(fr_one<F>()), lb > 0 ? lb - 1 : 0, 0));
        p->stage_tw[i] = std::move(T.lo);           // the one-entry high half goes with T
    }
    if (ntt_direct_max(ctx) >= log_n) {       // direct twiddle tables: 2^log_m entries per strided pass
        int rem = log_n;
        for (int i = 0; i + 1 < p->P; ++i) {
            if (p->tw_direct[i].alloc(ctx, ((size_t)1 << rem) * sizeof(fr_t)) != hipSuccess) { optional_table_note(ctx, i ? "plan.tw_direct[1]" : "plan.tw_direct[0]", log_n); break; }   // no memory: keep the two-level lookup
            hipLaunchKernelGGL(k_fill_tw_direct<F>, dim3((unsigned)((((uint64_t)1 << rem) + 255) / 256)), dim3(256), 0, ctx->stream, p->root.view(), log_n, rem, p->log_b[i], p->tw_direct[i].fr());
            rem -= p->log_b[i];
        }
    }
    if (inverse) {
        fr_t ninv = x32<F>(fr_inv<F>(fr_from_u64<F>(1ull << log_n)));
        STARK_TRY(p->scale.fill_sync(ctx, &ninv, sizeof(fr_t)));
    }
    *out = ctx->plans[key] = p.release(); return STARK_OK;
}

// one workgroup per CU (tile > 80 KiB of LDS) => 512 threads so that every SIMD still holds 2 waves
static inline unsigned ntt_threads(size_t lds) { return lds > 80 * 1024 ? 512u : 256u; }
// tile elements E = B*C: 2^11 by default (64 KiB + twiddles => 2 workgroups per CU); option "ntt_log_tile" overrides for tuning
static inline int ntt_minw(const stark_ctx* ctx) { return ctx->opt.ntt_min_waves; }
// total_log: log2 of all elements the launch covers; small launches take smaller tiles so that the grid still fills the chip
static inline NttTileOpts tile_opts(const stark_ctx* ctx) { NttTileOpts o; o.log_tile = ctx->opt.ntt_log_tile; o.forced = ctx->opt.ntt_log_tile_forced; o.max_lds = kMaxLds; return o; }
static inline int pick_log_c(const stark_ctx* ctx, int log_b, int cap, int total_log = 30) { return ntt_pick_log_c(tile_opts(ctx), log_b, cap, total_log); }

// One launch of a pass kernel.  addr: nothing (the plain kernels: contiguous vectors at src / dst), or how a batched launch finds its vectors —
// NttBatchAddr (one shape: A is the pass of every column) or NttRaggedAddr (A, src and dst unused: every argument comes from the shape table).
template <class F, int MINW, bool STRIDED, class... BT>
static void launch_pass(bool pre, unsigned th, size_t lds, hipStream_t st, uint32_t ntiles, const NttPassArgs& A, const fr_t* src, fr_t* dst, const BT&... addr) {
    const dim3 grid(ntiles), block(th);
    if (STRIDED) { if (pre) hipLaunchKernelGGL((k_ntt_strided<F, MINW, true, BT...>), grid, block, lds, st, A, src, dst, addr...); else hipLaunchKernelGGL((k_ntt_strided<F, MINW, false, BT...>), grid, block, lds, st, A, src, dst, addr...); }
    else { if (pre) hipLaunchKernelGGL((k_ntt_last<F, MINW, true, BT...>), grid, block, lds, st, A, src, dst, addr...); else hipLaunchKernelGGL((k_ntt_last<F, MINW, false, BT...>), grid, block, lds, st, A, src, dst, addr...); }
}
// ... with the wave count and the threads that go with a tile of `lds` bytes
template <class F, bool STRIDED, class... BT>
static int32_t launch_sized(stark_ctx* ctx, bool pre, size_t lds, uint32_t ntiles, const NttPassArgs& A, const fr_t* src, fr_t* dst, const BT&... addr) {
    if (lds > kMaxLds) return ctx->fail(STARK_ERR_UNSUPPORTED, "NTT tile exceeds LDS");
    if (ntt_minw(ctx) > 2 && lds <= 40 * 1024) launch_pass<F, 4, STRIDED>(pre, 256u, lds, ctx->stream, ntiles, A, src, dst, addr...);
    else launch_pass<F, 2, STRIDED>(pre, ntt_threads(lds), lds, ctx->stream, ntiles, A, src, dst, addr...);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
// Bt: the vectors' addresses of a same-size batched pass; nullptr: the plain kernels
template <class F, bool STRIDED>
static int32_t launch_any(stark_ctx* ctx, NttPassArgs A, uint64_t total_elems, bool pre, const fr_t* src, fr_t* dst, const NttBatchAddr* Bt) {
    A.ntiles = (uint32_t)(total_elems >> (A.log_b + A.log_c));
    const size_t lds = ntt_lds_bytes(A.log_b, A.log_c);
    return Bt ? launch_sized<F, STRIDED>(ctx, pre, lds, A.ntiles, A, src, dst, *Bt) : launch_sized<F, STRIDED>(ctx, pre, lds, A.ntiles, A, src, dst);
}
template <class F> static int32_t launch_strided(stark_ctx* ctx, const NttPassArgs& A, uint64_t total_elems, const fr_t* src, fr_t* dst, const NttBatchAddr* Bt = nullptr) { return launch_any<F, true>(ctx, A, total_elems, A.pre_direct || A.pre.lo, src, dst, Bt); }
template <class F> static int32_t launch_last(stark_ctx* ctx, const NttPassArgs& A, uint64_t total_elems, const fr_t* src, fr_t* dst, const NttBatchAddr* Bt = nullptr) { return launch_any<F, false>(ctx, A, total_elems, A.pre.lo != nullptr, src, dst, Bt); }

// plain (c0 = 1) power table of `base` over the plan's 2^log_n points, from the plan's cache (`pin`: PowCache::get)
template <class F> static int32_t plain_table(stark_ctx* ctx, NttPlan* big, const fr_t& base, PowTable* out, const PowTable* pin = nullptr) {
    return big->plain_tabs.get<F>(ctx, base, big->log_n, fr_one<F>(), tab_lo(big->log_n), tab_hi(big->log_n), out, pin);
}
// The coset-dependent tables of plan p for the coset g, into a fresh C (the caller move-assigns it on success, so a failure leaves the plan's
// current coset whole; a plain table of g that a failed build already put into plain_tabs stays there, valid under its own key).  The pre-scale
// of a forward plan takes the first form that can be had: merged into the first pass's twiddle table (option ntt_merged_coset, and
// tw_direct[0] exists), else one direct table, else the two-level lookup.  An optional table that cannot be allocated
// degrades (dev_malloc leaves no runtime error behind); it never fails the transform.  The price of building beside the current coset: its tables (up to two of
// 2^log_n entries) are still allocated meanwhile, so close to the device's memory limit an optional table that used to fit may degrade, and
// that form then stays until the coset next changes.
template <class F>
static int32_t build_coset(stark_ctx* ctx, NttPlan* p, const fr_t& g, NttCoset& C) {
    const int log_n = p->log_n; const bool inverse = p->inverse;
    if (!inverse) STARK_TRY(C.tab.fill<F>(ctx, g, x32<F>(fr_one<F>()), tab_lo(log_n), tab_hi(log_n)));              // g^j
    else STARK_TRY(C.tab.fill<F>(ctx, fr_inv<F>(g), x32<F>(fr_inv<F>(fr_from_u64<F>(1ull << log_n))), tab_lo(log_n), tab_hi(log_n)));   // n^-1 g^-k
    C.g = g; C.have = true;
    bool merged = false;
    if (!inverse && p->P >= 2 && p->tw_direct[0] && ctx->opt.ntt_merged_coset && ntt_direct_max(ctx) >= log_n) {
        // merged tables: the pre-scale's g^rest goes into the first pass's twiddle table, what is left is (g^S)^p by point index
        PowTable gplain; STARK_TRY(plain_table<F>(ctx, p, g, &gplain));
        const int lb0 = p->log_b[0], ls = log_n - lb0;
        if (C.small.alloc(ctx, ((size_t)1 << lb0) * sizeof(fr_t)) != hipSuccess) optional_table_note(ctx, "coset.small", log_n);
        else if (C.tw_direct.alloc(ctx, ((size_t)1 << log_n) * sizeof(fr_t)) != hipSuccess) optional_table_note(ctx, "coset.tw_direct", log_n);
        else {
            hipLaunchKernelGGL(k_fill_coset_merged<F>, dim3((unsigned)((((uint64_t)1 << log_n) + 255) / 256)), dim3(256), 0, ctx->stream, C.tab.view(), gplain, (const fr_t*)p->tw_direct[0].fr(), ls, lb0, C.small.fr(), C.tw_direct.fr());
            merged = hipGetLastError() == hipSuccess;
        }
        if (!merged) { C.small.reset(); C.tw_direct.reset(); }
    }
    if (!merged) {
        if (!inverse && ntt_direct_max(ctx) >= log_n) {
            if (C.direct.alloc(ctx, ((size_t)1 << log_n) * sizeof(fr_t)) == hipSuccess)
                hipLaunchKernelGGL(k_fill_pow_direct<F>, dim3((unsigned)((((uint64_t)1 << log_n) + 255) / 256)), dim3(256), 0, ctx->stream, C.tab.view(), 1ull << log_n, C.direct.fr());
            else optional_table_note(ctx, "coset.direct", log_n);
        }
    }
    return STARK_OK;
}
// the plan's tables for the coset g: a plan holds ONE coset and rebuilds its tables when another one is asked for
template <class F> static int32_t use_coset(stark_ctx* ctx, NttPlan* p, const fr_t& g) {
    if (!p->coset.have || !fr_eq(p->coset.g, g)) { NttCoset C; STARK_TRY(build_coset<F>(ctx, p, g, C)); p->coset = std::move(C); }
    return STARK_OK;
}
// Pass i of plan p at tile width 2^log_c as kernel arguments (all but ntiles, which the launch sets).  coset: the transform runs on the plan's current
// coset (use_coset) — the pre-scale on load in the first pass of a forward plan, the post-scale in the last pass of an inverse one.
template <class F>
static NttPassArgs pass_args(const NttPlan* p, int i, int log_c, bool coset, const fr_t* scale_override_dev, int log_nonzero) {
    const int log_n = p->log_n; const bool inverse = p->inverse; const NttCoset& C = p->coset;
    NttPassArgs A; memset(&A, 0, sizeof(A)); ntt29_offset<F>(A.dlimb);
    A.log_n = log_n; A.root = p->root.view(); A.log_vec = log_n;
    A.log_b = p->log_b[i]; A.log_c = log_c; A.stage_tw = p->stage_tw[i].fr();
    const bool pre = coset && !inverse && i == 0;
    if (pre) A.pre = C.tab.view();
    if (i + 1 < p->P) {                    // strided pass
        int rem = log_n; for (int q = 0; q < i; ++q) rem -= p->log_b[q];       // log2 of the sub-problem this pass splits
        A.log_m = rem; A.stride = 1ull << (rem - A.log_b); A.tw_direct = p->tw_direct[i].fr();
        if (pre) {
            A.pre_direct = C.direct.fr();
            if (C.small && C.tw_direct) { A.pre_small = C.small.fr(); A.tw_direct = C.tw_direct.fr(); }       // merged form
        }
        // zero-padded input (LDE): element j is non-zero only for j < 2^log_nonzero; in the first strided pass that is the points p < 2^log_nonzero / stride
        A.nz_points = (i == 0 && log_nonzero >= 0 && log_nonzero < log_n && (1ull << log_nonzero) >= A.stride) ? (uint32_t)((1ull << log_nonzero) / A.stride) : 0u;
    } else {
        A.log_b1 = p->P >= 2 ? p->log_b[0] : 0; A.log_b2 = p->P == 3 ? p->log_b[1] : 0;
        if (coset && inverse) A.post = C.tab.view();
        A.scale = A.post.lo ? nullptr : (scale_override_dev ? scale_override_dev : (inverse ? p->scale.fr() : nullptr));
    }
    return A;
}
// Where the vectors of a transform start and end.  Plain (ntt_run): contiguous at `src` == `dst`, 2^log_n apart, transformed in place through the
// context's scratch by the plain kernels.  Batched (`batch` set; the NttBatchAddr instantiations): vector v is read at src_tab[v] or src + v * src_pitch
// and leaves at dst_tab[v] or dst + v * dst_pitch (tables of DEVICE pointers in device memory, pitches in elements); `work` holds the [B][2^log_n]
// intermediate of a transform of more than one pass and may be the source (a strided pass works in place), never the destination.
struct NttEnds {
    bool batch = false;
    const fr_t* const* src_tab = nullptr; const fr_t* src = nullptr; uint64_t src_pitch = 0;
    fr_t* const* dst_tab = nullptr; fr_t* dst = nullptr; uint64_t dst_pitch = 0;
    fr_t* work = nullptr;
};
// The passes of `batch` transforms of 2^log_n points (1 <= log_n <= 30, batch >= 1) between the ends E.
template <class F>
static int32_t ntt_passes(stark_ctx* ctx, const NttEnds& E, int log_n, uint64_t batch, bool inverse, const fr_t* coset, const fr_t* scale_override_dev, int log_nonzero) {
    NttPlan* p = nullptr; STARK_TRY(get_plan<F>(ctx, log_n, inverse, &p));
    if (coset) STARK_TRY(use_coset<F>(ctx, p, *coset));
    const uint64_t total = batch << log_n, n = 1ull << log_n;
    // tile width: a plain call sizes its tiles by one vector (what it has always done), a batched pass by all the elements its launches cover
    const int total_log = E.batch ? ntt_floor_log2(total) : log_n;
    fr_t* scratch = E.work;
    if (p->P > 1 && !E.batch) { void* s = nullptr; STARK_TRY(ctx_scratch(ctx, total * sizeof(fr_t), &s)); scratch = (fr_t*)s; }
    const NttBatchAddr first{E.src_tab, nullptr, E.src_pitch, n}, middle{nullptr, nullptr, n, n}, last{p->P == 1 ? E.src_tab : nullptr, E.dst_tab, p->P == 1 ? E.src_pitch : n, E.dst_pitch};
    const fr_t* src = E.src;
    int rem = log_n;                       // log2 of the current sub-problem size
    for (int i = 0; i + 1 < p->P; ++i) {   // strided passes
        const NttPassArgs A = pass_args<F>(p, i, pick_log_c(ctx, p->log_b[i], rem - p->log_b[i], total_log), coset != nullptr, nullptr, log_nonzero);
        STARK_TRY(launch_strided<F>(ctx, A, total, src, scratch, E.batch ? (i == 0 ? &first : &middle) : nullptr));
        src = scratch; rem -= A.log_b;
    }
    const NttPassArgs A = pass_args<F>(p, p->P - 1, p->P == 1 ? 0 : pick_log_c(ctx, p->log_b[p->P - 1], p->log_b[0], total_log), coset != nullptr, scale_override_dev, -1);
    STARK_TRY(launch_last<F>(ctx, A, total, src, E.dst, E.batch ? &last : nullptr));
    return STARK_OK;
}
// `batch` vectors of 2^log_n elements each, contiguous.  data is transformed in place (scratch from the context).
template <class F>
static int32_t ntt_run(stark_ctx* ctx, fr_t* data, int log_n, uint64_t batch, bool inverse, const fr_t* coset, const fr_t* scale_override_dev, int log_nonzero = -1) {
    if (log_n < 0 || log_n > 30) return ctx->fail(STARK_ERR_INVALID_ARG, "log_n out of range");
    if (batch == 0) return STARK_OK;
    if (log_n == 0) {   // size-1 transform: identity (n^-1 = 1, g^0 = 1)
        return STARK_OK;
    }
    NttEnds E; E.src = data; E.dst = data;
    return ntt_passes<F>(ctx, E, log_n, batch, inverse, coset, scale_override_dev, log_nonzero);
}

template <class F>
static int32_t lde_run(stark_ctx* ctx, const fr_t* evals, int log_n, int log_blowup, const fr_t* coset, fr_t* out) {
    const uint64_t n = 1ull << log_n, N = n << log_blowup;
    STARK_HIP(ctx, hipMemcpyAsync(out, evals, n * sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
    STARK_TRY(ntt_run<F>(ctx, out, log_n, 1, true, nullptr, nullptr));                       // evaluations on H -> coefficients
    fr_t one = fr_one<F>(); bool unit = !coset || fr_eq(*coset, one);
    const bool skip = ntt_lde_skips_padding(log_n, log_blowup);                              // the padding is taken as zero, never written
    if (N > n && !skip) { hipLaunchKernelGGL(k_zero_fill<F>, dim3((unsigned)((N - n + 255) / 256)), dim3(256), 0, ctx->stream, out + n, N - n); STARK_HIP(ctx, hipGetLastError()); }
    return ntt_run<F>(ctx, out, log_n + log_blowup, 1, false, unit ? nullptr : coset, nullptr, skip ? log_n : -1);   // coefficients -> coset evaluations on the larger domain
}

// ---- stark_ntt_batch_dev / stark_lde_batch_dev: many columns of one shape and one coset per device pass ---------------------------------------
// A pass's pointer tables ([sources | destinations], one upload) in pooled device memory; the host copy of the upload belongs to the context.
static int32_t upload_tables(stark_ctx* ctx, DevBuf& d, const std::vector<const void*>& tab) {
    STARK_HIP(ctx, d.alloc(ctx, tab.size() * sizeof(void*)));
    return ctx_upload_staged(ctx, d.p, tab.data(), tab.size() * sizeof(void*));
}
template <class F>
static int32_t pad_fill(stark_ctx* ctx, const fr_t* const* src_tab, const fr_t* src, uint64_t src_pitch, fr_t* const* dst_tab, fr_t* dst, uint64_t dst_pitch, uint64_t first, uint64_t head, uint64_t len, uint64_t B) {
    const uint64_t tot = (len - first) * B; if (!tot) return STARK_OK;
    hipLaunchKernelGGL(k_pad_fill_batch<F>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, src_tab, src, src_pitch, dst_tab, dst, dst_pitch, first, head, len, B);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
// One pass of B >= 2 in-place transforms: the first launch reads the caller's vectors through the table, the last one writes them through it.
template <class F>
static int32_t ntt_batch_pass(stark_ctx* ctx, uint64_t* const* data, size_t B, int log_n, bool inverse, const fr_t* coset) {
    if (log_n == 0) return STARK_OK;                                         // size-1 transforms: identity
    NttPlan* p = nullptr; STARK_TRY(get_plan<F>(ctx, log_n, inverse, &p));
    NttEnds E; E.batch = true;
    if (p->P > 1) { void* w = nullptr; STARK_TRY(ctx_scratch(ctx, (B << log_n) * sizeof(fr_t), &w)); E.work = (fr_t*)w; }
    DevBuf dtab; STARK_TRY(upload_tables(ctx, dtab, std::vector<const void*>(data, data + B)));
    E.src_tab = (const fr_t* const*)dtab.p; E.dst_tab = (fr_t* const*)dtab.p;
    return ntt_passes<F>(ctx, E, log_n, B, inverse, coset, nullptr, -1);
}
template <class F>
static int32_t ntt_batch_run(stark_ctx* ctx, size_t batch, uint64_t* const* data, int log_n, bool inverse, const fr_t* coset) {
    size_t b0 = 0;
    for (size_t Bp : ntt_mixed_passes(batch, std::vector<size_t>(batch, (size_t)log_n).data(), ctx->opt.ntt_batch_max_elems)) {
        if (Bp == 1) STARK_TRY(ntt_run<F>(ctx, as_fr(data[b0]), log_n, 1, inverse, coset, nullptr));
        else STARK_TRY(ntt_batch_pass<F>(ctx, data + b0, Bp, log_n, inverse, coset));
        b0 += Bp;
    }
    return STARK_OK;
}
// One pass of B >= 2 extensions, lde_run's steps once each for all columns.  Scratch: X = [B][N] and Cs = [B][n].  The inverse transform reads
// the caller's columns through the table (no copy) and leaves the coefficients where the forward transform's first pass wants them: in Cs at
// pitch n when that pass takes the padding as zero without reading it (lde_run's `skip`), else in X at pitch N with the tails zeroed by one
// launch.  Its own intermediate is the other region.  The forward transform works in X and its last pass stores into the caller's outputs.
// Every input is read by the first launch and every output written by the last, so inside a pass an input may alias any output.
template <class F>
static int32_t lde_batch_pass(stark_ctx* ctx, const uint64_t* const* evals, uint64_t* const* out, size_t B, int log_n, int log_blowup, const fr_t* coset) {
    const int big = log_n + log_blowup;
    const uint64_t n = 1ull << log_n, N = 1ull << big;
    const fr_t one = fr_one<F>(); const bool unit = !coset || fr_eq(*coset, one);
    const bool skip = ntt_lde_skips_padding(log_n, log_blowup);
    void* w = nullptr; STARK_TRY(ctx_scratch(ctx, B * (N + n) * sizeof(fr_t), &w));
    fr_t* const X = (fr_t*)w; fr_t* const Cs = X + B * N;
    std::vector<const void*> tab(2 * B);
    for (size_t b = 0; b < B; ++b) { tab[b] = evals[b]; tab[B + b] = out[b]; }
    DevBuf dtab; STARK_TRY(upload_tables(ctx, dtab, tab));
    const fr_t* const* src_tab = (const fr_t* const*)dtab.p; fr_t* const* dst_tab = (fr_t* const*)dtab.p + B;
    fr_t* const coef = skip ? Cs : X; const uint64_t pitch = skip ? n : N;
    if (log_n == 0) {          // one point: the interpolation is the point itself, written with its padding in one launch
        STARK_TRY(pad_fill<F>(ctx, src_tab, nullptr, 0, nullptr, X, N, 0, 1, N, B));
        if (big == 0) return pad_fill<F>(ctx, nullptr, X, 1, dst_tab, nullptr, 0, 0, 1, 1, B);
    } else {
        NttEnds I; I.batch = true; I.src_tab = src_tab; I.dst = coef; I.dst_pitch = pitch; I.work = skip ? X : Cs;
        STARK_TRY(ntt_passes<F>(ctx, I, log_n, B, true, nullptr, nullptr, -1));                // evaluations on H -> coefficients
        if (N > n && !skip) STARK_TRY(pad_fill<F>(ctx, nullptr, nullptr, 0, nullptr, X, N, n, 0, N, B));
    }
    NttEnds O; O.batch = true; O.src = coef; O.src_pitch = pitch; O.dst_tab = dst_tab; O.work = X;
    return ntt_passes<F>(ctx, O, big, B, false, unit ? nullptr : coset, nullptr, skip ? log_n : -1);   // coefficients -> coset evaluations on the larger domain
}
template <class F>
static int32_t lde_batch_run(stark_ctx* ctx, size_t batch, const uint64_t* const* evals, uint64_t* const* out, int log_n, int log_blowup, const fr_t* coset) {
    size_t b0 = 0;
    for (size_t Bp : ntt_mixed_passes(batch, std::vector<size_t>(batch, (size_t)(log_n + log_blowup)).data(), ctx->opt.ntt_batch_max_elems)) {
        if (Bp == 1) STARK_TRY(lde_run<F>(ctx, as_fr(evals[b0]), log_n, log_blowup, coset, as_fr(out[b0])));
        else STARK_TRY(lde_batch_pass<F>(ctx, evals + b0, out + b0, Bp, log_n, log_blowup, coset));
        b0 += Bp;
    }
    return STARK_OK;
}

// ---- stark_ntt_mixed_batch_dev / stark_lde_mixed_batch_dev: columns of any lengths in one device pass (the plan: ntt_mixed_plan.hpp) -------------------
// The launches of one pass.  in / out: the caller's tables for the columns of this pass (the same table for in-place transforms); g_inv / g_fwd: the
// coset of the inverse / forward transforms (nullptr: none).  A launch of one shape (ntt_mixed_one_shape: the 2^12 columns' strided pass beside 2^5 ones)
// takes its pass as the kernel argument and finds its vectors through NttBatchAddr: a table of the caller's pointers in launch order, or base + pitch
// in the scratch.  Any other launch is ragged: shape records, column records and the first-tile list.  All device tables of the pass go up as ONE
// staged upload into one pooled block.
template <class F>
static int32_t mixed_pass_run(stark_ctx* ctx, const NttMixedPlan& plan, const uint64_t* const* in, uint64_t* const* out, const fr_t* g_inv, const fr_t* g_fwd) {
    void* w = nullptr; if (plan.scratch_elems) STARK_TRY(ctx_scratch(ctx, plan.scratch_elems * sizeof(fr_t), &w));
    fr_t* const scratch = (fr_t*)w;
    auto at = [&](const NttMixedRef& r, uint32_t col) -> fr_t* { return r.mem == NTT_MEM_IN ? const_cast<fr_t*>(as_fr(in[col])) : r.mem == NTT_MEM_OUT ? as_fr(out[col]) : scratch + r.off; };
    struct Staged { bool one = false; NttOneShape ends; NttPassArgs A; size_t shapes = 0, cols = 0, first = 0, src_tab = 0, dst_tab = 0; };   // offsets in 8-byte words
    std::vector<uint64_t> blob; std::vector<Staged> staged;
    auto put = [&](const void* src, size_t bytes) { const size_t o = blob.size(); blob.resize(o + (bytes + 7) / 8); memcpy(blob.data() + o, src, bytes); return o; };
    std::vector<const void*> tab, last_tab; size_t last_off = 0;
    auto table = [&](const NttMixedLaunch& L, int mem) {                         // an in-place transform reads and writes through one table
        tab.clear(); for (const NttMixedCol& c : L.cols) tab.push_back(mem == NTT_MEM_IN ? (const void*)in[c.col] : (const void*)out[c.col]);
        if (tab != last_tab) { last_off = put(tab.data(), tab.size() * sizeof(void*)); last_tab = tab; }
        return last_off;
    };
    for (const NttMixedLaunch& L : plan.launches) {
        Staged S;
        if (L.kind == NTT_MIXED_PAD) {
            std::vector<NttPadCol> cols; for (const NttMixedCol& c : L.cols) cols.push_back(NttPadCol{at(c.src, c.col), at(c.dst, c.col), c.first, c.head, c.len});
            S.cols = put(cols.data(), cols.size() * sizeof(NttPadCol));
        } else {
            const bool inverse = L.kind == NTT_MIXED_INVERSE; const fr_t* g = inverse ? g_inv : g_fwd;
            std::vector<NttPassArgs> shapes;
            for (const NttMixedShape& s : L.shapes) {
                NttPlan* p = nullptr; STARK_TRY(get_plan<F>(ctx, s.log_n, inverse, &p));
                if (g) STARK_TRY(use_coset<F>(ctx, p, *g));
                NttPassArgs A = pass_args<F>(p, s.pass, s.log_c, g != nullptr, nullptr, s.log_nonzero); A.ntiles = s.tiles;
                shapes.push_back(A);
            }
            S.one = ntt_mixed_one_shape(L, &S.ends);
            if (S.one) {
                S.A = shapes[0]; S.A.ntiles = L.ntiles;
                if (S.ends.src.mem != NTT_MEM_SCRATCH) S.src_tab = table(L, S.ends.src.mem);
                if (S.ends.dst.mem != NTT_MEM_SCRATCH) S.dst_tab = table(L, S.ends.dst.mem);
                staged.push_back(S); continue;
            }
            std::vector<NttRaggedCol> cols; for (const NttMixedCol& c : L.cols) cols.push_back(NttRaggedCol{at(c.src, c.col), at(c.dst, c.col), c.shape, c.first_tile});
            S.shapes = put(shapes.data(), shapes.size() * sizeof(NttPassArgs)); S.cols = put(cols.data(), cols.size() * sizeof(NttRaggedCol));
        }
        std::vector<uint32_t> first; for (const NttMixedCol& c : L.cols) first.push_back(c.first_tile);
        S.first = put(first.data(), first.size() * sizeof(uint32_t));
        staged.push_back(S);
    }
    if (blob.empty()) return STARK_OK;                                           // no launch (the first launch of a plan reads the caller's columns through a table)
    DevBuf dtab; STARK_HIP(ctx, dtab.alloc(ctx, blob.size() * 8)); STARK_TRY(ctx_upload_staged(ctx, dtab.p, blob.data(), blob.size() * 8));
    const uint64_t* const base = (const uint64_t*)dtab.p;
    for (size_t l = 0; l < plan.launches.size(); ++l) {
        const NttMixedLaunch& L = plan.launches[l]; const Staged& S = staged[l]; const uint32_t ncols = (uint32_t)L.cols.size();
        const uint32_t* const first = (const uint32_t*)(base + S.first);
        if (L.kind == NTT_MIXED_PAD) {
            hipLaunchKernelGGL(k_pad_fill_ragged<F>, dim3(L.ntiles), dim3(NTT_PAD_BLOCK), 0, ctx->stream, (const NttPadCol*)(base + S.cols), first, ncols);
            STARK_HIP(ctx, hipGetLastError());
        } else if (S.one) {
            const bool stab = S.ends.src.mem != NTT_MEM_SCRATCH, dtb = S.ends.dst.mem != NTT_MEM_SCRATCH;
            const NttBatchAddr Bt{stab ? (const fr_t* const*)(base + S.src_tab) : nullptr, dtb ? (fr_t* const*)(base + S.dst_tab) : nullptr, S.ends.src.pitch, S.ends.dst.pitch};
            const fr_t* const src = stab ? nullptr : scratch + S.ends.src.off; fr_t* const dst = dtb ? nullptr : scratch + S.ends.dst.off;
            if (L.strided) STARK_TRY((launch_sized<F, true>(ctx, L.pre, L.lds, L.ntiles, S.A, src, dst, Bt)));
            else STARK_TRY((launch_sized<F, false>(ctx, L.pre, L.lds, L.ntiles, S.A, src, dst, Bt)));
        } else {
            const NttRaggedAddr R{(const NttPassArgs*)(base + S.shapes), (const NttRaggedCol*)(base + S.cols), first, ncols};
            NttPassArgs none; memset(&none, 0, sizeof(none));                    // the ragged kernels take every argument from R.shapes
            if (L.strided) STARK_TRY((launch_sized<F, true>(ctx, L.pre, L.lds, L.ntiles, none, nullptr, nullptr, R)));
            else STARK_TRY((launch_sized<F, false>(ctx, L.pre, L.lds, L.ntiles, none, nullptr, nullptr, R)));
        }
    }
    return STARK_OK;
}
template <class F>
static int32_t ntt_mixed_run(stark_ctx* ctx, size_t batch, uint64_t* const* data, const size_t* log_n, bool inverse, const fr_t* coset) {
    size_t b0 = 0;
    for (size_t Bp : ntt_mixed_passes(batch, log_n, ctx->opt.ntt_batch_max_elems)) {
        if (Bp == 1) STARK_TRY(ntt_run<F>(ctx, as_fr(data[b0]), (int)log_n[b0], 1, inverse, coset, nullptr));
        else STARK_TRY(mixed_pass_run<F>(ctx, ntt_mixed_ntt_plan(log_n + b0, Bp, inverse, coset != nullptr, tile_opts(ctx)), data + b0, data + b0, inverse ? coset : nullptr, inverse ? nullptr : coset));
        b0 += Bp;
    }
    return STARK_OK;
}
template <class F>
static int32_t lde_mixed_run(stark_ctx* ctx, size_t batch, const uint64_t* const* evals, uint64_t* const* out, const size_t* log_n, int log_blowup, const fr_t* coset) {
    const fr_t one = fr_one<F>(); const bool unit = !coset || fr_eq(*coset, one);
    std::vector<size_t> log_out(log_n, log_n + batch); for (size_t& l : log_out) l += (size_t)log_blowup;
    size_t b0 = 0;
    for (size_t Bp : ntt_mixed_passes(batch, log_out.data(), ctx->opt.ntt_batch_max_elems)) {
        if (Bp == 1) STARK_TRY(lde_run<F>(ctx, as_fr(evals[b0]), (int)log_n[b0], log_blowup, coset, as_fr(out[b0])));
        else STARK_TRY(mixed_pass_run<F>(ctx, ntt_mixed_lde_plan(log_n + b0, Bp, log_blowup, !unit, tile_opts(ctx)), evals + b0, out + b0, nullptr, unit ? nullptr : coset));
        b0 += Bp;
    }
    return STARK_OK;
}

void stark::ntt_plans_free(stark_ctx* ctx) { for (auto& kv : ctx->plans) delete kv.second; ctx->plans.clear(); }

// Per-DEVICE kernel attributes (the default tile is 64 KiB + twiddles, above the 64 KiB a kernel may use without opting in):
// called from stark_ctx_create with the context's device current, so a process holding contexts on several GPUs sets them on each.
template <class F> static void set_attrs_for() {
    (void)hipFuncSetAttribute((const void*)k_ntt_strided<F, 2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_strided<F, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_last<F, 2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_last<F, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_strided<F, 2, false, NttBatchAddr>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_strided<F, 2, true, NttBatchAddr>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_last<F, 2, false, NttBatchAddr>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_last<F, 2, true, NttBatchAddr>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_strided<F, 2, false, NttRaggedAddr>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_strided<F, 2, true, NttRaggedAddr>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_last<F, 2, false, NttRaggedAddr>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)k_ntt_last<F, 2, true, NttRaggedAddr>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
}
void stark::ntt_set_attrs() { set_attrs_for<PallasFr>(); set_attrs_for<Bls12381Fr>(); }

// Multi-GPU phase A: column NTTs of size 2^log_rows over a row-major [2^log_rows][ncols] slab whose first
// column has global index col0, followed by the twiddle w_N^(col_global * k), N = 2^log_n.  In place.
template <class F>
static int32_t columns_run(stark_ctx* ctx, fr_t* slab, int log_rows, uint64_t ncols, uint64_t col0, int log_n, bool inverse, const fr_t* shift = nullptr) {
    if (log_rows < 1 || log_rows > 10) return ctx->fail(STARK_ERR_UNSUPPORTED, "column NTT size must be 2..1024");
    if (ncols == 0 || (ncols & (ncols - 1))) return ctx->fail(STARK_ERR_INVALID_ARG, "ncols must be a power of two");
    NttPlan* big = nullptr; STARK_TRY(get_plan<F>(ctx, log_n, inverse, &big));        // root table of w_N
    NttPlan* sm = nullptr; STARK_TRY(get_plan<F>(ctx, log_rows, inverse, &sm));       // stage twiddles of w_R (P == 1 plan)
    NttPassArgs A; memset(&A, 0, sizeof(A)); ntt29_offset<F>(A.dlimb);
    int log_cols = 0; while ((1ull << log_cols) < ncols) ++log_cols;
    A.log_b = log_rows; A.log_c = pick_log_c(ctx, log_rows, log_cols); A.log_n = log_n; A.stride = ncols; A.log_m = log_n;
    A.stage_tw = sm->stage_tw[0].fr(); A.root = big->root.view(); A.rest0 = col0;
    if (shift && !fr_eq(*shift, fr_one<F>())) {
        // coset evaluation: x[j] *= shift^j with j the GLOBAL natural index of the element (row * C + global column)
        if (inverse) return ctx->fail(STARK_ERR_UNSUPPORTED, "column phase: the coset pre-scale belongs to a forward transform");
        STARK_TRY(big->shift_tabs.get<F>(ctx, *shift, log_n, x32<F>(fr_one<F>()), tab_lo(log_n), tab_hi(log_n), &A.pre));
        A.pre_row_stride = 1ull << (log_n - log_rows);
    }
    return launch_strided<F>(ctx, A, (uint64_t)ncols << log_rows, slab, slab);
}
// Multi-GPU forward transform, first local phase, on the layout the inverse transform leaves behind (dist.py ShardedLde): rows k1 = row0 + i of the
// [R][C] view c[k1 + R k'] (R = 2^(log_n - log_cols) rows in the whole vector, this rank holds nrows of them, each contiguous over k').
//   dst[i][m] = w_n^(k1 m) * sum_k' src[i][k'] shift^(k' R + k1) w_C^(k' m)
// i.e. coset pre-scale at the natural index, size-C transforms along the contiguous axis, inter-step twiddle.  The second phase is a plain size-R
// transform over k1 after the exchange.  src is left untouched (the 2^log_blowup cosets of an LDE all start from the same coefficients).
template <class F>
static int32_t rows_coset_run(stark_ctx* ctx, const fr_t* src, fr_t* dst, uint64_t nrows, int log_cols, uint64_t row0, int log_n, const fr_t& shift) {
    if (log_cols < 0 || log_cols > log_n || log_n > 30) return ctx->fail(STARK_ERR_INVALID_ARG, "rows_coset: sizes");
    const int log_rows = log_n - log_cols;
    if (!nrows || row0 + nrows > (1ull << log_rows)) return ctx->fail(STARK_ERR_INVALID_ARG, "rows_coset: row range");
    NttPlan* big = nullptr; STARK_TRY(get_plan<F>(ctx, log_n, false, &big));
    // tsh is pinned while w_N's table is fetched: a miss there may evict, but never the table asked for a line earlier.  The root of unity itself
    // is a legal shift, and then the two are the same table — which is correct
    PowTable tsh, troot;
    STARK_TRY(plain_table<F>(ctx, big, shift, &tsh));
    STARK_TRY(plain_table<F>(ctx, big, fr_root_of_unity<F>((unsigned)log_n), &troot, &tsh));
    const uint64_t tot = nrows << log_cols; const unsigned grid = (unsigned)((tot + 255) / 256);
    hipLaunchKernelGGL(k_rows_coset_pre<F>, dim3(grid), dim3(256), 0, ctx->stream, src, dst, tsh, nrows, log_cols, row0, log_rows);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(ntt_run<F>(ctx, dst, log_cols, nrows, false, nullptr, nullptr));
    hipLaunchKernelGGL(k_rows_twiddle<F>, dim3(grid), dim3(256), 0, ctx->stream, dst, troot, nrows, log_cols, row0, log_n);
    STARK_HIP(ctx, hipGetLastError());
    return STARK_OK;
}

// ---- one column of a trace block-sharded over the ranks of the context's communicator: the LDE as ONE call (dist.py ShardedLde in C++) ----------
// A host without Python composes nothing: rank q passes its natural-order block [q n/W, (q+1) n/W) of the 2^log_n evaluations and receives its block of the
// 2^(log_n + log_blowup) evaluations on shift * <w_N>.  Four all-to-alls (ShardColl, shard_coll.hpp), whatever the blow-up: natural rows -> column
// blocks; the inverse transform's transpose; ONE exchange for the first-phase outputs of all cosets; ONE to natural blocks.  Between them only local
// phases (columns_run, ntt_run rows, rows_coset_run) and the pack kernel.
static int32_t pack3(stark_ctx* ctx, const fr_t* src, fr_t* dst, uint64_t d0, uint64_t d1, uint64_t d2, int p0, int p1, int p2) {
    const uint64_t d[3] = {d0, d1, d2}, st[3] = {d1 * d2, d2, 1}; const int pm[3] = {p0, p1, p2};
    const uint64_t tot = d0 * d1 * d2; if (!tot) return STARK_OK;
    hipLaunchKernelGGL(k_permute3, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, src, dst, d[pm[0]], d[pm[1]], d[pm[2]], st[pm[0]], st[pm[1]], st[pm[2]]);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
// One rank's buffers and the five local phases between the four exchanges.  One driver (lde_sharded) runs them for the local ranks of a ShardColl:
// the communicator's rank (stark_lde_sharded_dev) or W ranks emulated on one GPU (stark_diag_lde_sharded_emulated_dev).
struct ShardPlan { int W, log_n, lb, log_rows, log_cols; uint64_t R, Cc, b, nrl, ncl, nl; };
struct ShardRank { int rank; const fr_t* block; fr_t* out; DevBuf t0, t1, big0, big1; };
static int32_t shard_plan(stark_ctx* ctx, int W, int log_n, int lb, ShardPlan& P) {
    if (log_n < 2 || log_n + lb > 30) return ctx->fail(STARK_ERR_INVALID_ARG, "lde_sharded: sizes");
    P.W = W; P.log_n = log_n; P.lb = lb; P.log_rows = std::min(10, log_n / 2); P.log_cols = log_n - P.log_rows;
    P.R = 1ull << P.log_rows; P.Cc = 1ull << P.log_cols; P.b = 1ull << lb;
    if (W < 1 || (W & (W - 1)) || P.R % W || P.Cc % W) return ctx->fail(STARK_ERR_INVALID_ARG, "lde_sharded: the ranks must divide the 2^log_rows x 2^log_cols view");
    P.nrl = P.R / W; P.ncl = P.Cc / W; P.nl = P.nrl * P.Cc;               // local rows, local columns, local elements of one size-n vector
    return STARK_OK;
}
static int32_t shard_alloc(stark_ctx* ctx, const ShardPlan& P, ShardRank& K) {
    STARK_HIP(ctx, K.t0.alloc(ctx, P.nl * sizeof(fr_t))); STARK_HIP(ctx, K.t1.alloc(ctx, P.nl * sizeof(fr_t)));
    STARK_HIP(ctx, K.big0.alloc(ctx, P.b * P.nl * sizeof(fr_t))); STARK_HIP(ctx, K.big1.alloc(ctx, P.b * P.nl * sizeof(fr_t)));
    return STARK_OK;
}
// phase k runs after exchange k (phase 0: before the first).  Exchange k sends `send_of(k)` and receives into `recv_of(k)`, `per_peer(k)` elements per peer.
static const fr_t* shard_send(const ShardRank& K, int x) { return x == 0 ? K.t0.fr() : x == 1 ? K.t1.fr() : K.big1.fr(); }
static fr_t* shard_recv(const ShardRank& K, int x) { return x == 0 ? K.t1.fr() : x == 1 ? K.t0.fr() : K.big0.fr(); }
static uint64_t shard_per_peer(const ShardPlan& P, int x) { return x < 2 ? P.nrl * P.ncl : P.b * P.nrl * P.ncl; }
template <class F>
static int32_t shard_phase(stark_ctx* ctx, const ShardPlan& P, ShardRank& K, int phase, const fr_t& shift) {
    const uint64_t W = P.W, nrl = P.nrl, ncl = P.ncl, nl = P.nl, b = P.b, R = P.R;
    switch (phase) {
    case 0:   // natural row block [nrl][W][ncl] -> [W][nrl][ncl]; exchange 0 makes it the column block [R][ncl]
        return pack3(ctx, K.block, K.t0.fr(), nrl, W, ncl, 1, 0, 2);
    case 1:   // inverse six-step transform: column phase + twiddle; exchange 1 is its transpose
        return columns_run<F>(ctx, K.t1.fr(), P.log_rows, ncl, (uint64_t)K.rank * ncl, P.log_n, true);
    case 2: { // [W][nrl][ncl] -> [nrl][C] (rows k1 of c[k1 + R k']); row phase with n^-1; first phase of every coset transform on that slab; pack for exchange 2
        STARK_TRY(pack3(ctx, K.t0.fr(), K.t1.fr(), W, nrl, ncl, 1, 0, 2));
        { DevWord sc; STARK_TRY(sc.set(ctx, x32<F>(fr_inv<F>(fr_from_u64<F>(1ull << P.log_n)))));
          STARK_TRY((ntt_run<F>(ctx, K.t1.fr(), P.log_cols, nrl, true, nullptr, sc.dev.fr()))); }
        const fr_t wN = fr_root_of_unity<F>((unsigned)(P.log_n + P.lb)); fr_t sh = shift;
        for (uint64_t s_ = 0; s_ < b; ++s_) { STARK_TRY((rows_coset_run<F>(ctx, K.t1.fr(), K.big0.fr() + s_ * nl, nrl, P.log_cols, (uint64_t)K.rank * nrl, P.log_n, sh))); sh = fr_mul<F>(sh, wN); }
        return pack3(ctx, K.big0.fr(), K.big1.fr(), b * nrl, W, ncl, 1, 0, 2); }                     // [b nrl][W][ncl] -> [W][b nrl][ncl]
    case 3:   // [W][b][nrl ncl] -> [b][R][ncl] -> [b ncl][R]; size-R transforms; [b][ncl][R] -> [R][ncl][b] for exchange 3
        STARK_TRY(pack3(ctx, K.big0.fr(), K.big1.fr(), W, b, nrl * ncl, 1, 0, 2));
        STARK_TRY(pack3(ctx, K.big1.fr(), K.big0.fr(), b, R, ncl, 0, 2, 1));
        STARK_TRY((ntt_run<F>(ctx, K.big0.fr(), P.log_rows, b * ncl, false, nullptr, nullptr)));
        return pack3(ctx, K.big0.fr(), K.big1.fr(), b, ncl, R, 2, 1, 0);
    default:  // [W][nrl][ncl b] -> [nrl][W][ncl b]: natural order of the interleaved result out[(K2 C + K1) b + s]
        return pack3(ctx, K.big0.fr(), K.out, W, nrl, ncl * b, 1, 0, 2);
    }
}
// block / out: this rank's blocks, or the whole arrays when C is emulated
template <class F>
static int32_t lde_sharded(const ShardColl& C, const fr_t* block, int log_n, int lb, const fr_t& shift, fr_t* out) {
    stark_ctx* ctx = C.ctx;
    ShardPlan P; STARK_TRY(shard_plan(ctx, C.W, log_n, lb, P));
    std::vector<ShardRank> K(C.local());
    for (size_t i = 0; i < K.size(); ++i) {
        K[i].rank = C.rank(i); K[i].block = block + C.block(i) * P.nl; K[i].out = out + (C.block(i) * P.nl << lb); STARK_TRY(shard_alloc(ctx, P, K[i]));
    }
    for (int phase = 0; phase < 5; ++phase) {
        for (auto& k : K) STARK_TRY((shard_phase<F>(ctx, P, k, phase, shift)));
        if (phase == 4) break;
        std::vector<const void*> send; std::vector<void*> recv;
        for (auto& k : K) { send.push_back(shard_send(k, phase)); recv.push_back(shard_recv(k, phase)); }
        STARK_TRY(C.all_to_all(send, recv, shard_per_peer(P, phase) * sizeof(fr_t)));
    }
    return STARK_OK;
}

extern "C" {

int32_t stark_lde_sharded_dev(stark_ctx_t* ctx, int32_t field_id, const uint64_t* block, size_t log_n, size_t log_blowup, const uint64_t* shift4, uint64_t* out) {
    if (!ctx || !block || !out || !shift4 || block == out) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const fr_t sh = load_fr(shift4); ShardColl C = ShardColl::real(ctx);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return lde_sharded<F>(C, as_fr(block), (int)log_n, (int)log_blowup, sh, as_fr(out)); });
}
int32_t stark_diag_lde_sharded_emulated_dev(stark_ctx_t* ctx, int32_t field_id, int32_t nranks, const uint64_t* evals, size_t log_n, size_t log_blowup, const uint64_t* shift4, uint64_t* out) {
    if (!ctx || !evals || !out || !shift4 || evals == out || nranks < 1) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const fr_t sh = load_fr(shift4); ShardColl C = ShardColl::emulate(ctx, nranks);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return lde_sharded<F>(C, as_fr(evals), (int)log_n, (int)log_blowup, sh, as_fr(out)); });
}
int32_t stark_ntt_rows_coset_dev(stark_ctx_t* ctx, int32_t field_id, const uint64_t* src, uint64_t* dst, size_t nrows, size_t log_cols, size_t row0, size_t log_n, const uint64_t* shift4) {
    if (!ctx || !src || !dst || !shift4 || src == dst) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const fr_t sh = load_fr(shift4);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return rows_coset_run<F>(ctx, as_fr(src), as_fr(dst), nrows, (int)log_cols, row0, (int)log_n, sh); });
}
int32_t stark_ntt_dev(stark_ctx_t* ctx, int32_t field_id, uint64_t* data, size_t log_n, int32_t inverse, const uint64_t* coset4) {
    if (!ctx || !data) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    fr_t cs; if (coset4) cs = load_fr(coset4);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return ntt_run<F>(ctx, as_fr(data), (int)log_n, 1, inverse != 0, coset4 ? &cs : nullptr, nullptr); });
}
int32_t stark_ntt(stark_ctx_t* ctx, int32_t field_id, uint64_t* data, size_t log_n, int32_t inverse, const uint64_t* coset4) {
    if (!ctx || !data || log_n > 30) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    size_t bytes = ((size_t)1 << log_n) * sizeof(fr_t); DevBuf d; CallerUploads up(ctx); STARK_HIP(ctx, up.up(d, data, bytes));
    STARK_TRY(stark_ntt_dev(ctx, field_id, (uint64_t*)d.p, log_n, inverse, coset4));
    STARK_HIP(ctx, up.download_sync(data, d.p, bytes)); return STARK_OK;
}
int32_t stark_lde_dev(stark_ctx_t* ctx, int32_t field_id, const uint64_t* evals, size_t log_n, size_t log_blowup, const uint64_t* coset4, uint64_t* out) {
    if (!ctx || !evals || !out || log_n + log_blowup > 30) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    fr_t cs; if (coset4) cs = load_fr(coset4);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return lde_run<F>(ctx, as_fr(evals), (int)log_n, (int)log_blowup, coset4 ? &cs : nullptr, as_fr(out)); });
}
// What the four batched calls refuse after ctx_enter, under the call's name: a null column, an output longer than 2^30, two outputs that overlap.
// evals: the inputs of an extension (nullptr: a transform in place, whose outputs are its columns); output b has 2^(log_n[b] + log_blowup) elements.
static int32_t batch_check(stark_ctx* ctx, const std::string& call, size_t batch, const uint64_t* const* evals, uint64_t* const* out, const size_t* log_n, size_t log_blowup) {
    std::vector<size_t> bytes(batch);
    for (size_t b = 0; b < batch; ++b) {
        if (!out[b] || (evals && !evals[b])) return ctx->fail(STARK_ERR_INVALID_ARG, call + ": null column");
        if (log_n[b] > 30 || log_n[b] + log_blowup > 30) return ctx->fail(STARK_ERR_INVALID_ARG, call + (evals ? ": log_n + log_blowup out of range" : ": log_n out of range"));
        bytes[b] = sizeof(fr_t) << (log_n[b] + log_blowup);
    }
    if (ntt_batch_ranges_overlap((const void* const*)out, batch, bytes.data())) return ctx->fail(STARK_ERR_INVALID_ARG, call + (evals ? ": outputs overlap" : ": columns overlap"));
    return STARK_OK;
}
int32_t stark_ntt_mixed_batch_dev(stark_ctx_t* ctx, int32_t field_id, size_t batch, uint64_t* const* data, const size_t* log_n, int32_t inverse, const uint64_t* coset4) {
    if (!ctx || (batch && (!data || !log_n))) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    STARK_TRY(batch_check(ctx, "ntt_mixed_batch", batch, nullptr, data, log_n, 0));
    fr_t cs; if (coset4) cs = load_fr(coset4);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return ntt_mixed_run<F>(ctx, batch, data, log_n, inverse != 0, coset4 ? &cs : nullptr); });
}
int32_t stark_lde_mixed_batch_dev(stark_ctx_t* ctx, int32_t field_id, size_t batch, const uint64_t* const* evals, const size_t* log_n, size_t log_blowup, const uint64_t* coset4, uint64_t* const* out) {
    if (!ctx || (batch && (!evals || !out || !log_n)) || log_blowup > 30) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    STARK_TRY(batch_check(ctx, "lde_mixed_batch", batch, evals, out, log_n, log_blowup));
    fr_t cs; if (coset4) cs = load_fr(coset4);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return lde_mixed_run<F>(ctx, batch, evals, out, log_n, (int)log_blowup, coset4 ? &cs : nullptr); });
}
// The same-size calls keep drivers of their own (on the plan they measured slower at some shapes); the checks are the shared ones.
int32_t stark_ntt_batch_dev(stark_ctx_t* ctx, int32_t field_id, size_t batch, uint64_t* const* data, size_t log_n, int32_t inverse, const uint64_t* coset4) {
    if (!ctx || (batch && !data) || log_n > 30) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const std::vector<size_t> lns(batch, log_n);
    STARK_TRY(batch_check(ctx, "ntt_batch", batch, nullptr, data, lns.data(), 0));
    fr_t cs; if (coset4) cs = load_fr(coset4);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return ntt_batch_run<F>(ctx, batch, data, (int)log_n, inverse != 0, coset4 ? &cs : nullptr); });
}
int32_t stark_lde_batch_dev(stark_ctx_t* ctx, int32_t field_id, size_t batch, const uint64_t* const* evals, size_t log_n, size_t log_blowup, const uint64_t* coset4, uint64_t* const* out) {
    if (!ctx || (batch && (!evals || !out)) || log_n > 30 || log_blowup > 30 || log_n + log_blowup > 30) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const std::vector<size_t> lns(batch, log_n);
    STARK_TRY(batch_check(ctx, "lde_batch", batch, evals, out, lns.data(), log_blowup));
    fr_t cs; if (coset4) cs = load_fr(coset4);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return lde_batch_run<F>(ctx, batch, evals, out, (int)log_n, (int)log_blowup, coset4 ? &cs : nullptr); });
}
int32_t stark_lde(stark_ctx_t* ctx, int32_t field_id, const uint64_t* evals, size_t log_n, size_t log_blowup, const uint64_t* coset4, uint64_t* out) {
    if (!ctx || !evals || !out || log_n + log_blowup > 30) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    size_t n = (size_t)1 << log_n, N = n << log_blowup; DevBuf di, dout; CallerUploads up(ctx); STARK_HIP(ctx, up.up(di, evals, n * sizeof(fr_t))); STARK_HIP(ctx, dout.alloc(ctx, N * sizeof(fr_t)));
    STARK_TRY(stark_lde_dev(ctx, field_id, (const uint64_t*)di.p, log_n, log_blowup, coset4, (uint64_t*)dout.p));
    STARK_HIP(ctx, up.download_sync(out, dout.p, N * sizeof(fr_t))); return STARK_OK;
}

int32_t stark_ntt_columns_dev(stark_ctx_t* ctx, int32_t field_id, uint64_t* slab, size_t log_rows, size_t ncols, size_t col0, size_t log_n, int32_t inverse) {
    if (!ctx || !slab) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return columns_run<F>(ctx, as_fr(slab), (int)log_rows, ncols, col0, (int)log_n, inverse != 0); });
}
int32_t stark_ntt_columns_coset_dev(stark_ctx_t* ctx, int32_t field_id, uint64_t* slab, size_t log_rows, size_t ncols, size_t col0, size_t log_n, const uint64_t* shift4) {
    if (!ctx || !slab || !shift4) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const fr_t sh = load_fr(shift4);
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return columns_run<F>(ctx, as_fr(slab), (int)log_rows, ncols, col0, (int)log_n, false, &sh); });
}
int32_t stark_permute3_dev(stark_ctx_t* ctx, const uint64_t* src, uint64_t* dst, size_t d0, size_t d1, size_t d2, int32_t p0, int32_t p1, int32_t p2) {
    if (!ctx || !src || !dst || src == dst) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const int pm[3] = {p0, p1, p2}; int seen = 0; for (int i = 0; i < 3; ++i) { if (pm[i] < 0 || pm[i] > 2) return ctx->fail(STARK_ERR_INVALID_ARG, "permutation"); seen |= 1 << pm[i]; }
    if (seen != 7) return ctx->fail(STARK_ERR_INVALID_ARG, "permutation");
    return pack3(ctx, as_fr(src), as_fr(dst), d0, d1, d2, p0, p1, p2);
}
int32_t stark_interleave_dev(stark_ctx_t* ctx, const uint64_t* src, uint64_t* dst, size_t n, size_t stride, size_t offset) {
    if (!ctx || !src || !dst || !stride || offset >= stride) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (!n) return STARK_OK;
    hipLaunchKernelGGL(k_interleave, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, as_fr(src), as_fr(dst), (uint64_t)n, (uint64_t)stride, (uint64_t)offset);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
// Multi-GPU phase B: `nrows` contiguous NTTs of size 2^log_cols.  scale4 (optional) multiplies every output
// (the caller passes N^-1 of the FULL transform for an inverse; the per-row n^-1 is not applied).
int32_t stark_ntt_rows_dev(stark_ctx_t* ctx, int32_t field_id, uint64_t* slab, size_t nrows, size_t log_cols, int32_t inverse, const uint64_t* scale4) {
    if (!ctx || !slab) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return with_field(ctx, field_id, [&](auto f) -> int32_t {
        using F = decltype(f); DevWord sc;
        // into the kernels' table domain; an inverse without scale4 multiplies by one, which suppresses the plan's per-row n^-1
        if (scale4 || inverse) STARK_TRY(sc.set(ctx, x32<F>(scale4 ? load_fr(scale4) : fr_one<F>())));
        return ntt_run<F>(ctx, as_fr(slab), (int)log_cols, nrows, inverse != 0, nullptr, sc.dev.fr());
    });
}

// ---- crates/field: Domain::new / compute_powers (field/src/lib.rs:43-53, 125-133) ------------------------------------------------
// get_root_of_unity(2^log_n) of the field (host-only: no context, no device)
int32_t stark_root_of_unity(int32_t field_id, size_t log_n, uint64_t* out4) {
    if (!out4 || log_n > 32) return STARK_ERR_INVALID_ARG;                                   // two-adicity 32 in both fields
    if (field_id == STARK_FIELD_PALLAS_FR) store_fr(out4, fr_root_of_unity<PallasFr>((unsigned)log_n));
    else if (field_id == STARK_FIELD_BLS12_381_FR) store_fr(out4, fr_root_of_unity<Bls12381Fr>((unsigned)log_n));
    else return STARK_ERR_INVALID_ARG;
    return STARK_OK;
}
}  // extern "C"
template <class F> static int32_t powers_run(stark_ctx* ctx, const fr_t& base, size_t n, fr_t* out_dev) {
    if (!n) return STARK_OK;
    int bits = 1; while (((size_t)1 << bits) < n) ++bits;
    const int lo_bits = (bits + 1) / 2, hi_bits = bits - lo_bits + 1;
    DevPowTable T; STARK_TRY(T.fill<F>(ctx, base, fr_one<F>(), lo_bits, hi_bits));
    hipLaunchKernelGGL(k_fill_pow_direct<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, T.view(), (uint64_t)n, out_dev);
    hipError_t e = hipGetLastError(); if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // the two-level table is a temporary of this call: synchronised before T frees it
    if (e != hipSuccess) return ctx->fail(STARK_ERR_HIP, "compute_powers");
    return STARK_OK;
}
extern "C" {
// compute_powers(base, n) = [1, base, ..., base^(n-1)] (also Domain::precompute_elements with base = omega); *_dev writes device memory
int32_t stark_compute_powers_dev(stark_ctx_t* ctx, int32_t field_id, const uint64_t* base4, size_t n, uint64_t* out) {
    if (!ctx || !base4 || (!out && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return with_field(ctx, field_id, [&](auto f) { using F = decltype(f); return powers_run<F>(ctx, load_fr(base4), n, as_fr(out)); });
}
int32_t stark_compute_powers(stark_ctx_t* ctx, int32_t field_id, const uint64_t* base4, size_t n, uint64_t* out) {
    if (!ctx || !base4 || (!out && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    DevBuf d; STARK_HIP(ctx, d.alloc(ctx, n * sizeof(fr_t)));
    STARK_TRY(stark_compute_powers_dev(ctx, field_id, base4, n, (uint64_t*)d.p));
    STARK_HIP(ctx, d.download_sync(out, n * sizeof(fr_t))); return STARK_OK;
}

int32_t stark_synth_column_dev(stark_ctx_t* ctx, uint64_t seed, uint64_t col, size_t i0, size_t n, uint64_t* out) {
    if (!ctx || (!out && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (!n) return STARK_OK;
    hipLaunchKernelGGL(k_synth, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, seed, col, (uint64_t)i0, (uint64_t)n, as_fr(out));
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}

}  // extern "C"
