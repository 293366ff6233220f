// stark_mlwe_amd/csrc/capi_fri.hip — FRI folding, fri_build_transcript, DEEP-ALI merge, build_f0 and
// the end-to-end deep_fri_prove orchestration (host logic in C++ above the kernels, mirroring
// crates/deep_ali/src/fri.rs and crates/deep_ali/src/lib.rs).  C-ABI in include/stark_mlwe.h.
//
// One trace is a batch of one.  Every prove — stark_deep_fri_prove_dev from columns or from f0, and the two batch entry points — is
//   challenge_stage (columns only: all column sponges and Fiat-Shamir hashes of the batch, three synchronisations)
//   -> prove_pass per pass of traces: PassCommit::run (layer 0 + commit phase, no synchronisation) -> batch_queries (four synchronisations).
// Each of these is written once.  Only the commit phase has three forms — fri_build_impl for a pass of one trace, FriDevBatch (fri_batch.hpp) side
// by side for traces of one n0, FriDevMixed (fri_mixed.hpp) for traces of one schedule and any n0 (the classes of "mixed_prove_tail") — and
// PassCommit::run is the one place that chooses; what follows reads any of them through a view (StateArrays / BatchArrays / MixedArrays).  The
// sharded prover (fri_shard_impl.hpp) shares the plan, the assembly and the row gather (merkle_batch.hpp: MerkleGatherList; gather_rows).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include "poseidon_launch.hpp"
#include "pow_table.hpp"
#include "fri_dev.hpp"
#include "fri_batch.hpp"
#include "fri_mixed.hpp"
#include "merkle_batch.hpp"
#include "lagrange_dev.hpp"
#include "shard_coll.hpp"

using namespace stark;

struct stark_fri_state {
    CtxRef ref_;
    stark_ctx* ctx = nullptr;
    std::vector<size_t> schedule;
    std::vector<DevBuf> f; std::vector<size_t> n;          // L+1 layers (device, pooled)
    std::vector<fr_t> z;                                    // L fold challenges
    std::vector<std::unique_ptr<stark_tree>> trees; std::vector<size_t> arity;
    std::vector<fr_t> roots;                                // fetched on first use (one download + one sync for all L+1)
};

static inline bool is_pow2(size_t x) { return x && !(x & (x - 1)); }
static inline int ilog2(size_t x) { return ilog2_ceil(x); }
using Clock = std::chrono::steady_clock;
static double ms_between(Clock::time_point x, Clock::time_point y) { return std::chrono::duration<double, std::milli>(y - x).count(); }

// fold on `st` with the z-power table zp (m entries, device)
static int32_t fold_launch(stark_ctx* ctx, hipStream_t st, const fr_t* f, size_t n, const fr_t* zp, size_t m, fr_t* out) {
    if (is_pow2(m)) {
        int log_m = ilog2(m), log_g = std::min(log_m, 4);
        uint64_t lanes = (uint64_t)n >> (log_m - log_g);
        hipLaunchKernelGGL(k_fri_fold_pow2<PallasFr>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, f, (uint64_t)n, zp, log_m, log_g, out);
    } else {
        uint64_t no = n / m;
        hipLaunchKernelGGL(k_fri_fold_any<PallasFr>, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, st, f, no, zp, (uint64_t)m, out);
    }
    STARK_HIP(ctx, hipGetLastError());
    return STARK_OK;
}
// z^0..z^(m-1) (fri.rs:91-93) computed ON the device into a pooled table: no host round trip, nothing to keep alive on the host.
static int32_t zpows_launch(stark_ctx* ctx, hipStream_t st, const fr_t& z, size_t m, fr_t* zp) {
    hipLaunchKernelGGL(k_zpows<PallasFr>, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, z, (uint64_t)m, zp);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
static int32_t fold_dev(stark_ctx* ctx, const fr_t* f, size_t n, const fr_t& z, size_t m, fr_t* out) {
    if (m < 2) return ctx->fail(STARK_ERR_INVALID_ARG, "m >= 2");                                        // fri.rs:86
    if (n % m) return ctx->fail(STARK_ERR_INVALID_ARG, "layer size must be divisible by m");             // fri.rs:87
    if (!n) return STARK_OK;
    DevBuf zp; STARK_HIP(ctx, zp.alloc(ctx, m * sizeof(fr_t)));
    STARK_TRY(zpows_launch(ctx, ctx->stream, z, m, zp.fr()));
    return fold_launch(ctx, ctx->stream, f, n, zp.fr(), m, out);     // zp returns to the pool: its next user is ordered behind this fold on the same stream
}

// fri_sample_z_ell (fri.rs:59-82): transcript hash on the device, ChaCha12 + candidate test on the host.  The value depends
// only on (seed_z, level, domain_size) (fri.rs:250), so it is computed once per context and key.
static int32_t sample_z(stark_ctx* ctx, uint64_t seed_z, size_t level, size_t domain_size, fr_t* z) {
    const stark_ctx::ZKey key{seed_z, level, domain_size};
    auto it = ctx->z_cache.find(key);
    if (it != ctx->z_cache.end()) { *z = it->second; return STARK_OK; }
    fr_t fused; STARK_TRY(tr_hash_host1(ctx, "FRI/z/l", {host::h_u64(seed_z), host::h_u64(level), host::h_u64(domain_size)}, &fused));
    *z = fri_z_from_fused(fused, seed_z, level, domain_size);
    ctx->z_cache[key] = *z; return STARK_OK;
}

// All L+1 roots with one download and one synchronisation (the query phase needs them on the host; a caller that only builds
// the commitments never pays for it).
static int32_t state_roots(stark_fri_state* S) {
    if (!S->roots.empty()) return STARK_OK;
    stark_ctx* ctx = S->ctx; std::vector<fr_t> r(S->trees.size());
    for (size_t l = 0; l < S->trees.size(); ++l) {
        const stark_tree* T = S->trees[l].get();
        if (T->lens.back() != 1) return ctx->fail(STARK_ERR_INVALID_ARG, "partial (sharded) tree has no root");
        STARK_HIP(ctx, hipMemcpyAsync(&r[l], T->levels.back(), sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    S->roots = r; return STARK_OK;
}

// What a refused layer shape (fri_plan.hpp: fri_layers) is to the entry points of this file: INVALID_ARG for an empty layer or a schedule that does not
// divide.  A layer with arity 1 passes here: the single commit leaves it to merkle_build_on (STARK_ERR_UNSUPPORTED), the batched one to FriBatchCommit::shape.
static int32_t layers_or_fail(stark_ctx* ctx, size_t n0, const size_t* schedule, size_t L, std::vector<size_t>& n, std::vector<size_t>& arity) {
    const LayerShape sh = fri_layers(n0, schedule, L, n, arity);
    return sh == LayerShape::empty_layer || sh == LayerShape::not_dividing ? ctx->fail(STARK_ERR_INVALID_ARG, layer_shape_text(sh)) : STARK_OK;
}
// Everything of a commit phase that may upload constants (and synchronise doing so), to run before its first launch: the transcript parameters,
// the Merkle parameters of every layer (MerkleChannelCfg::new(arity), fri.rs:277) and the fold challenges (fri.rs:250).  After the first call
// these are all cached.
static int32_t fri_prelude(stark_ctx* ctx, const std::vector<size_t>& n, const std::vector<size_t>& arity, uint64_t seed_z, std::vector<stark_params*>& mps,
                           std::vector<fr_t>& z) {
    stark_params* tp = nullptr; STARK_TRY(ctx_transcript_params(ctx, &tp));
    mps.assign(arity.size(), nullptr);
    for (size_t l = 0; l < arity.size(); ++l) STARK_TRY(ctx_merkle_params(ctx, host::width_for_arity(arity[l]), &mps[l]));
    z.assign(n.size() - 1, host::h_zero());
    for (size_t l = 0; l + 1 < n.size(); ++l) STARK_TRY(sample_z(ctx, seed_z, l, n[l], &z[l]));
    return STARK_OK;
}
// The commitment of layer l on `st`.  A hashed arity hashes the leaf pairs (f[i], s[i] = f_next[i / m]; zeros on the last layer, fri.rs:266, 283)
// and moves the digests into the tree as level 0; any other arity is commit_pairs(f, s) (fri.rs:289).  The n leaves sit at DS positions pos0 onwards, and the
// tree climbs until a level of `stop` nodes (0: to the root).
static int32_t commit_layer_on(stark_ctx* ctx, hipStream_t st, stark_params* mp, size_t arity, size_t l, const fr_t* f, const fr_t* f_next, size_t n, size_t m,
                               uint64_t pos0, size_t stop, std::unique_ptr<stark_tree>& out) {
    if (!hashed_arity(arity)) return merkle_build_on(ctx, st, mp, arity, (uint64_t)l, f, n, 1, f_next, m, pos0, 0, stop, DevBuf(), out);
    DevBuf h; STARK_TRY(h.take(ctx, n * sizeof(fr_t)));
    STARK_TRY(leaf_pair_hash_on(ctx, st, f, f_next, n, m, h.fr()));
    return merkle_build_on(ctx, st, mp, arity, (uint64_t)l, nullptr, n, 0, nullptr, 1, pos0, 0, stop, std::move(h), out);
}

static int32_t fri_build_impl(stark_ctx* ctx, const fr_t* f0_dev, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, std::unique_ptr<stark_fri_state>& out) {
    std::unique_ptr<stark_fri_state> S(new stark_fri_state()); S->ref_.bind(ctx); S->ctx = ctx; S->schedule.assign(schedule, schedule + L);
    STARK_TRY(layers_or_fail(ctx, n0, schedule, L, S->n, S->arity));
    S->trees.resize(L + 1);
    // The prelude runs BEFORE any stream is forked.
    std::vector<stark_params*> mps;
    STARK_TRY(fri_prelude(ctx, S->n, S->arity, seed_z, mps, S->z));
    size_t zp_total = 0; for (size_t l = 0; l < L; ++l) zp_total += schedule[l];
    hipStream_t main_stream = ctx->stream;
    // layer 0 copy + folds back to back (the challenges do not depend on any commitment: fri.rs:250)
    S->f.resize(L + 1);
    for (size_t l = 0; l <= L; ++l) STARK_TRY(S->f[l].take(ctx, S->n[l] * sizeof(fr_t)));
    if (hipMemcpyAsync(S->f[0].p, f0_dev, n0 * sizeof(fr_t), hipMemcpyDeviceToDevice, main_stream) != hipSuccess) return ctx->fail(STARK_ERR_HIP, "copy f0");
    DevBuf zp; if (L && zp.alloc(ctx, zp_total * sizeof(fr_t)) != hipSuccess) return ctx->fail(STARK_ERR_OOM, "z powers: " + ctx->err);
    { size_t off = 0;
      for (size_t l = 0; l < L; ++l) {
          STARK_TRY(zpows_launch(ctx, main_stream, S->z[l], schedule[l], zp.fr() + off));
          STARK_TRY(fold_launch(ctx, main_stream, S->f[l].fr(), S->n[l], zp.fr() + off, schedule[l], S->f[l + 1].fr()));
          off += schedule[l];
      } }
    // Commitments of all L+1 layers (independent jobs).  Layer 0 is ~94 % of the hashing and fills the GPU; the later layers
    // are small and mostly LATENCY-bound (tree tops: one dependent permutation per level), so they go to a side stream and run
    // underneath layer 0 instead of after it.  The streams are passed explicitly; the side stream is forked from and joined back
    // into the main one with events, so nothing here synchronises the host.  A failure from here on leaves through the guard, which
    // drains both streams before S and zp return their blocks.
    StreamFork fk(ctx); STARK_TRY(fk.fork());
    auto commit_layer = [&](size_t l, hipStream_t st) {
        return commit_layer_on(ctx, st, mps[l], S->arity[l], l, S->f[l].fr(), l < L ? S->f[l + 1].fr() : nullptr, S->n[l], l < L ? schedule[l] : 1, 0, 0, S->trees[l]);
    };
    // Underneath a layer-0 leaf launch of 32 or more chip-fills (k_leaf_pair2: 4 workgroups of 64 leaves per CU) the side stream has time to spare,
    // but every wave slot it holds is one the leaf launch cannot use: its levels and leaf layers then take the wave-pair form at every size (64
    // sponges per two waves) instead of the latency forms (one wave, or five waves, per sponge) — option "fri_side_pair", read by the selector of capi_poseidon.hip.
    ctx->side_commit = ctx->opt.fri_side_pair && S->n[0] >= (size_t)ctx->num_cus * 4 * 64 * 32;
    int32_t crc = STARK_OK;
    for (size_t l = L; l >= 1 && crc == STARK_OK; --l) crc = commit_layer(l, fk.side);
    ctx->side_commit = false;
    if (crc == STARK_OK) crc = commit_layer(0, main_stream);
    STARK_TRY(crc);
    STARK_TRY(fk.join());                                           // the main stream continues only after the side stream's commitments
    out = std::move(S); return STARK_OK;
}

// Two-level power table of a domain generator, cached per (generator, size) — the reference's DomainH (deep_ali/src/lib.rs:109-125).
static int32_t omega_table(stark_ctx* ctx, const fr_t& omega, size_t n_global, PowTable* out) {
    int bits = ilog2(n_global); if (bits < 1) bits = 1;
    const int lo_bits = (bits + 1) / 2, hi_bits = bits - lo_bits + 1;
    if (!ctx->omega_tabs) ctx->omega_tabs.reset(new PowCache(16));
    return ctx->omega_tabs->get<PallasFr>(ctx, omega, bits, host::h_one(), lo_bits, hi_bits, out);
}

// deep_ali_merge_evals_blinded on device pointers (deep_ali/src/lib.rs:60-105).
static int32_t ali_merge_dev_impl(stark_ctx* ctx, const fr_t* a, const fr_t* s, const fr_t* e, const fr_t* t, const fr_t* r_opt, const fr_t& beta,
                                  const fr_t& omega, const fr_t& z, size_t n, fr_t* f0, fr_t* c_star_host,
                                  uint64_t j0 = 0, size_t n_global = 0, bool partial_only = false) {
    // n = number of local elements, holding the global positions j0 .. j0+n-1 of a domain of n_global points (whole vector: j0 = 0, n_global = n)
    if (!n_global) n_global = n;
    if (n_global <= 1 || !n || j0 + n > n_global) return ctx->fail(STARK_ERR_INVALID_ARG, "n > 1");                        // lib.rs:71
    if (fr_eq(fr_pow_u64<PallasFr>(z, n_global), host::h_one())) return ctx->fail(STARK_ERR_INVALID_ARG, "z must be outside H");   // lib.rs:78
    PowTable wp; STARK_TRY(omega_table(ctx, omega, n_global, &wp));
    const unsigned block = 256; uint64_t lanes = (n + ALI_K - 1) / ALI_K; unsigned grid = (unsigned)((lanes + block - 1) / block);
    const uint64_t T = (uint64_t)grid * block;
    fr_t w_step = fr_pow_u64<PallasFr>(omega, T);
    DevBuf sums; if (c_star_host) STARK_HIP(ctx, sums.alloc(ctx, (size_t)grid * sizeof(fr_t)));
    hipLaunchKernelGGL(k_ali_merge<PallasFr>, dim3(grid), dim3(block), 0, ctx->stream, a, s, e, t, r_opt, beta, wp, w_step, fr_inv<PallasFr>(w_step), z, (uint64_t)n, j0, f0, c_star_host ? sums.fr() : (fr_t*)nullptr);
    STARK_HIP(ctx, hipGetLastError());
    if (c_star_host) {
        // c* = phi(z)/Z_H(z) = (1/n) * sum_j phi_j w^j/(z - w^j)   (lib.rs:44 and :94); block partials are reduced on the device
        DevBuf tot; STARK_HIP(ctx, tot.alloc(ctx, sizeof(fr_t)));
        hipLaunchKernelGGL(k_sum_single_block<PallasFr>, dim3(1), dim3(256), 0, ctx->stream, (const fr_t*)sums.fr(), (uint64_t)grid, partial_only ? host::h_one() : fr_inv<PallasFr>(host::h_u64(n_global)), tot.fr());
        STARK_HIP(ctx, hipGetLastError());
        STARK_HIP(ctx, hipMemcpyAsync(c_star_host, tot.p, sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
        STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the caller reads *c_star_host on return
    }
    return STARK_OK;
}

// the RNG part of ali_sample_z_beta_fs (fri.rs:516-532): beta, then the first candidate outside H
static void ali_z_beta_from_fused(const fr_t& fused, size_t n0, const fr_t& roots_seed, fr_t* z, fr_t* beta) {
    uint8_t seed[32]; host::h_to_bytes_le(fused, seed); host::ChaCha12Rng rng(seed);
    *beta = host::h_u64(rng.next_u64());
    const fr_t one = host::h_one();
    for (size_t tries = 0;;) {
        fr_t cand = host::h_u64(rng.next_u64());
        if (!fr_is_zero(cand) && !fr_eq(fr_pow_u64<PallasFr>(cand, n0), one)) { *z = cand; return; }
        if (++tries >= 1000) {
            fr_t fb = host::h_add(roots_seed, host::h_u64(17));
            *z = !fr_eq(fr_pow_u64<PallasFr>(fb, n0), one) ? fb : host::h_u64(19); return;
        }
    }
}
// The challenges of build_f0 from the four column digests (fri.rs:556-560): seed_f = H("ALI/seed", [h_a, h_s, h_e, h_t, n0]), then
// ali_sample_z_beta_fs (fri.rs:511-533) under the tag "ALI/DEEP".
static int32_t ali_challenges(stark_ctx* ctx, const fr_t h[4], size_t n0, fr_t* seed_f, fr_t* z, fr_t* beta) {
    STARK_TRY(tr_hash_host1(ctx, "ALI/seed", {h[0], h[1], h[2], h[3], host::h_u64(n0)}, seed_f));
    fr_t fused; STARK_TRY(tr_hash_host1(ctx, "ALI/DEEP", {*seed_f, host::h_u64(n0)}, &fused));
    ali_z_beta_from_fused(fused, n0, *seed_f, z, beta); return STARK_OK;
}
// The challenge stage of build_f0 (fri.rs:548-560, 511-533) for B traces, trace p of n0[p] rows; cols[4 p + c] = column c of trace p (device).  What bounds one
// prove is the serial column sponge (n0 / 16 dependent permutations per column, one block each), and the chains of different traces are independent
// whatever their lengths: all 4 B of them run in ONE launch — traces of one size through the BatchColumns layout, traces of several sizes through the
// Ragged one (longest chains first, poseidon_streams.hpp), so the stage costs what its longest chain costs — and the two Fiat-Shamir hashes per trace
// ("ALI/seed", "ALI/DEEP", each with its trace's n0) are one launch each for the batch.
// THREE host synchronisations whatever B: the digests, the seeds, the fused hashes.  Per trace p: h[4 p ..], seed_f[p], z[p], beta[p].
struct AliChallenges { std::vector<fr_t> h, seed_f, z, beta; };
static int32_t challenge_stage(stark_ctx* ctx, size_t B, const fr_t* const* cols, const size_t* n0, AliChallenges& out) {
    DevBuf dptr, dig, seeds_in, seeds, deep_in, fused;
    STARK_HIP(ctx, dig.alloc(ctx, 4 * B * sizeof(fr_t)));
    const char* tags[4] = {"ALI/A", "ALI/S", "ALI/E", "ALI/T"};
    if (std::all_of(n0, n0 + B, [&](size_t n) { return n == n0[0]; })) {
        STARK_HIP(ctx, dptr.alloc(ctx, 4 * B * sizeof(void*)));
        STARK_TRY(ctx_upload_staged(ctx, dptr.p, cols, 4 * B * sizeof(void*)));
        STARK_TRY(tr_hash_columns_batch_dev(ctx, tags, (const fr_t* const*)dptr.p, B, n0[0], dig.fr()));
    } else {
        std::vector<const char*> tg(4 * B); std::vector<size_t> kk(4 * B);
        for (size_t p = 0; p < B; ++p) for (int c = 0; c < 4; ++c) { tg[4 * p + c] = tags[c]; kk[4 * p + c] = n0[p]; }
        STARK_TRY(tr_hash_many_dev(ctx, 4 * B, tg.data(), cols, kk.data(), dig.fr(), true));
    }
    out.h.resize(4 * B);
    STARK_HIP(ctx, hipMemcpyAsync(out.h.data(), dig.p, 4 * B * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // seed_f = H("ALI/seed", [h_a, h_s, h_e, h_t, n0]) and the fused hash of ali_sample_z_beta_fs (fri.rs:556-557, 511-515)
    std::vector<fr_t> in5(5 * B); for (size_t p = 0; p < B; ++p) { for (int c = 0; c < 4; ++c) in5[5 * p + c] = out.h[4 * p + c]; in5[5 * p + 4] = host::h_u64(n0[p]); }
    STARK_HIP(ctx, seeds_in.alloc(ctx, in5.size() * sizeof(fr_t))); STARK_HIP(ctx, seeds.alloc(ctx, B * sizeof(fr_t)));
    STARK_TRY(ctx_upload_staged(ctx, seeds_in.p, in5.data(), in5.size() * sizeof(fr_t)));
    STARK_TRY(tr_hash_dev(ctx, "ALI/seed", seeds_in.fr(), 5, B, seeds.fr()));
    out.seed_f.resize(B);
    STARK_HIP(ctx, hipMemcpyAsync(out.seed_f.data(), seeds.p, B * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<fr_t> in2(2 * B), fu(B); for (size_t p = 0; p < B; ++p) { in2[2 * p] = out.seed_f[p]; in2[2 * p + 1] = host::h_u64(n0[p]); }
    STARK_HIP(ctx, deep_in.alloc(ctx, in2.size() * sizeof(fr_t))); STARK_HIP(ctx, fused.alloc(ctx, B * sizeof(fr_t)));
    STARK_TRY(ctx_upload_staged(ctx, deep_in.p, in2.data(), in2.size() * sizeof(fr_t)));
    STARK_TRY(tr_hash_dev(ctx, "ALI/DEEP", deep_in.fr(), 2, B, fused.fr()));
    STARK_HIP(ctx, hipMemcpyAsync(fu.data(), fused.p, B * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out.z.resize(B); out.beta.resize(B);
    for (size_t p = 0; p < B; ++p) ali_z_beta_from_fused(fu[p], n0[p], out.seed_f[p], &out.z[p], &out.beta[p]);
    return STARK_OK;
}
// B traces of one size: the same stage with a constant vector
static int32_t challenge_stage(stark_ctx* ctx, size_t B, const fr_t* const* cols, size_t n0, AliChallenges& out) {
    const std::vector<size_t> n(B, n0); return challenge_stage(ctx, B, cols, n.data(), out);
}
// DeepAliRealBuilder::build_f0 (fri.rs:535-569), default builder: no blinding, ds_tag "ALI/DEEP": the challenge stage of one trace, then the merge.
static int32_t build_f0_dev_impl(stark_ctx* ctx, const fr_t* a, const fr_t* s, const fr_t* e, const fr_t* t, size_t n0, fr_t* f0, fr_t* aux7) {
    if (n0 <= 1) return ctx->fail(STARK_ERR_INVALID_ARG, "n0 > 1");
    const fr_t* cols[4] = {a, s, e, t}; AliChallenges ch; STARK_TRY(challenge_stage(ctx, 1, cols, n0, ch));
    if (aux7) { for (int c = 0; c < 4; ++c) aux7[c] = ch.h[c]; aux7[4] = ch.seed_f[0]; aux7[5] = ch.z[0]; aux7[6] = ch.beta[0]; }
    fr_t omega = fr_root_of_unity<PallasFr>((unsigned)ilog2(n0));         // FriDomain::new_radix2(n0).omega (fri.rs:53-56); Radix2EvaluationDomain::new rounds n0 up to a power of two, as ilog2 does
    return ali_merge_dev_impl(ctx, a, s, e, t, nullptr, host::h_zero(), omega, ch.z[0], n0, f0, nullptr);
}

// The transcript hasher of the query phase (fri_plan.hpp) on the device.
struct DeviceHasher : TrHasher {
    stark_ctx* ctx; explicit DeviceHasher(stark_ctx* c) : ctx(c) {}
    int32_t hash(const char* tag, const fr_t* fields, size_t k, size_t n, fr_t* out) override {
        if (n == 1) return tr_hash_host1(ctx, tag, std::vector<fr_t>(fields, fields + k), out);
        return stark_tr_hash_fields_tagged(ctx, nullptr, tag, (const uint64_t*)fields, k, n, (uint64_t*)out);
    }
};
// Transcript hashes of the query phase are pure functions of their inputs: the plan pass and the assembling pass ask for the same ones.
struct MemoHasher : TrHasher {
    TrHasher& inner; std::map<std::string, std::vector<fr_t>> memo;
    explicit MemoHasher(TrHasher& h) : inner(h) {}
    static std::string key_of(const char* tag, const fr_t* fields, size_t k, size_t n) {
        std::string key(tag); key.push_back('\0'); key.append((const char*)&k, sizeof(k)); key.append((const char*)fields, k * n * sizeof(fr_t)); return key;
    }
    // a result computed elsewhere (the batched query phase hashes the seeds of all its proofs in one launch)
    void preload(const char* tag, const fr_t* fields, size_t k, size_t n, const fr_t* out) { memo[key_of(tag, fields, k, n)] = std::vector<fr_t>(out, out + n); }
    int32_t hash(const char* tag, const fr_t* fields, size_t k, size_t n, fr_t* out) override {
        std::string key = key_of(tag, fields, k, n);
        auto it = memo.find(key);
        if (it == memo.end()) { std::vector<fr_t> v(n); int32_t rc = inner.hash(tag, fields, k, n, v.data()); if (rc) return rc; it = memo.emplace(std::move(key), std::move(v)).first; }
        memcpy((void*)out, it->second.data(), n * sizeof(fr_t)); return 0;
    }
};
// ---- the query phase: plan, ONE gather of the opened values, assembly -----------------------------------------------------------------------
// The query plan of a commit phase with the given roots.  The failures are INVALID_ARG: a refused shape under FriShape::make's message, an index
// outside its layer (fri_plan_make's -1) under the caller's wording.
static int32_t make_query_plan(stark_ctx* ctx, FriPlan& plan, size_t n0, const size_t* schedule, size_t L, const fr_t* roots, size_t r, TrHasher& H,
                               const char* bad_index = "query phase: bad index") {
    plan.r = r;
    { std::string err; if (!plan.shape.make(n0, schedule, L, roots, err)) return ctx->fail(STARK_ERR_INVALID_ARG, err); }
    const int32_t rc = fri_plan_make(plan, H);
    return rc == -1 ? ctx->fail(STARK_ERR_INVALID_ARG, bad_index) : rc;
}
// The proof from the n values of the plan's requests, in request order.  A list that runs short (assemble_proof's -1) or is not used up is
// INVALID_ARG under the caller's wording; any other failure is the hasher's and is returned as it is.
static int32_t assemble_from_values(stark_ctx* ctx, const FriShape& shape, size_t r, TrHasher& H, const fr_t* vals, size_t n, stark_proof* P,
                                    const char* mismatch = "query phase: value list does not match the plan") {
    ReplaySource rep(vals, n);
    const int32_t rc = assemble_proof(shape, r, H, rep, P->bytes, P->size_estimate);
    return rc == -1 || (rc == 0 && rep.pos != n) ? ctx->fail(STARK_ERR_INVALID_ARG, mismatch) : rc;
}
// One opened value of a query phase: row `to_row` of the gathered table is from[index] (the one row gather: MerkleGatherList, gather_rows).
static int32_t add_opening(stark_ctx* ctx, MerkleGatherList& G, const fr_t* from, size_t len, uint64_t index, uint64_t to_row) {
    if (index >= len) return ctx->fail(STARK_ERR_INVALID_ARG, "query phase: opening index out of range");
    G.add(from, index, to_row); return STARK_OK;
}
// Where a request of trace b reads when the whole commit phase of its pass is on this GPU: `c` names the layers and tree levels
// (layers(); layer(b, l, &len); levels(b, l); level(b, l, v, &len)), and the range checks are written here.
template <class Commit> static int32_t resolve_opening(stark_ctx* ctx, const Commit& c, size_t b, const FriRequest& q, const fr_t** from, size_t* len) {
    if (q.kind == 0) {
        if (q.which >= c.layers()) return ctx->fail(STARK_ERR_INVALID_ARG, "layer out of range");
        *from = c.layer(b, q.which, len); return STARK_OK;
    }
    if (q.which >= c.layers() || q.level >= c.levels(b, q.which)) return ctx->fail(STARK_ERR_INVALID_ARG, "tree level out of range");
    *from = c.level(b, q.which, q.level, len); return STARK_OK;
}
// The three views the query phase reads a commit phase through.  Besides the arrays each gives a proof's own shape (n0(b), r(b): constants of the
// pass in the first two) and says how its (L + 1) x traces() roots reach the host (roots_host: rt[b (L + 1) + l], one download and one synchronisation).
struct StateArrays {                                    // a stark_fri_state: one trace
    stark_fri_state* S; size_t r_;
    size_t traces() const { return 1; }
    size_t n0(size_t) const { return S->n[0]; }
    size_t r(size_t) const { return r_; }
    size_t layers() const { return S->f.size(); }
    const fr_t* layer(size_t, size_t l, size_t* len) const { *len = S->n[l]; return S->f[l].fr(); }
    size_t levels(size_t, size_t l) const { return S->trees[l]->levels.size(); }
    const fr_t* level(size_t, size_t l, size_t v, size_t* len) const { *len = S->trees[l]->lens[v]; return S->trees[l]->levels[v]; }
    int32_t roots_host(stark_ctx*, std::vector<fr_t>& rt) const { STARK_TRY(state_roots(S)); rt = S->roots; return STARK_OK; }
};

// Query plan of a commit phase whose layers live elsewhere (sharded over ranks): see fri_plan.hpp.
struct stark_fri_plan { CtxRef ref_; stark_ctx* ctx = nullptr; FriPlan plan; };

// ---- a pass of traces: the side-by-side commit (fri_batch.hpp), the query phase, the pass function and the batch drivers over them ----------
// The executor of FriBatchCommit on the device.  Its memory is the arena's; the folds run on the context's stream, the commitments on the
// current one (the side stream between fork() and side(false)).
struct FriDevExec : DevArena {
    hipStream_t main_st, cur; StreamFork fk;      // fk is destroyed before the arena's blocks: a scope left forked drains before they are released
    explicit FriDevExec(stark_ctx* c) : DevArena(c), main_st(c->stream), cur(c->stream), fk(c) {}
    int32_t zpows(const fr_t& z, size_t m, fr_t* zp) { return zpows_launch(ctx, main_st, z, m, zp); }
    int32_t fold(const fr_t* f, size_t n, const fr_t* zp, size_t m, fr_t* out) { return fold_launch(ctx, main_st, f, n, zp, m, out); }
    int32_t leaf_pairs(const fr_t* f, const fr_t* f_next, size_t n, size_t m, fr_t* h) { return leaf_pair_hash_on(ctx, cur, f, f_next, n, m, h); }
    template <class DS> int32_t hash_level(size_t arity, const DS& D, fr_t* out) { stark_params* mp = nullptr; STARK_TRY(ctx_merkle_params(ctx, host::width_for_arity(arity), &mp)); return hash_ds_on(ctx, cur, mp, D, out); }
    int32_t fork() { return fk.fork(); }
    void side(bool on) { cur = on && fk.side ? fk.side : main_st; }
    int32_t join() { return fk.join(); }
};
typedef FriBatchCommit<FriDevExec> FriDevBatch;
constexpr size_t kMaxPassTraces = 32768;             // blockIdx.y of the merge and copy kernels is the trace
// How many traces of n0 rows go into one pass (option "prove_batch_max_rows").
static size_t pass_traces(const stark_ctx* ctx, size_t n0) { return std::min(std::max<size_t>(ctx->opt.prove_batch_max_rows / std::max<size_t>(n0, 1), 1), kMaxPassTraces); }
// Shapes, challenges and buffers of a pass; everything that may upload constants (and synchronise doing so) runs here, before the first launch.
static int32_t batch_commit_begin(stark_ctx* ctx, FriDevBatch& C, size_t Bp, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z) {
    std::string err; int32_t rc = C.shape(Bp, n0, schedule, L, err);
    if (rc == -1) return ctx->fail(STARK_ERR_INVALID_ARG, err); if (rc == -2) return ctx->fail(STARK_ERR_UNSUPPORTED, err);
    std::vector<stark_params*> mps; std::vector<fr_t> z; STARK_TRY(fri_prelude(ctx, C.n, C.arity, seed_z, mps, z));
    return C.init(z.data());
}
// Layer 0 of a pass from a host table of per-trace device pointers: one copy kernel.
static int32_t batch_fill_layer0(stark_ctx* ctx, DevArena& X, FriDevBatch& C, const uint64_t* const* f0) {
    std::vector<const fr_t*> h(C.Bp); for (size_t b = 0; b < C.Bp; ++b) h[b] = as_fr(f0[b]);
    const fr_t** d = nullptr; STARK_TRY(X.put(h, &d));
    hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)((C.n[0] + 255) / 256), (unsigned)C.Bp), dim3(256), 0, ctx->stream, (const fr_t* const*)d, (uint64_t)C.n[0], C.f[0]);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
// deep_ali_merge_evals_blinded of Bp <= kMaxPassTraces traces over one domain of n points in one launch (k_ali_merge_batch).  Tables, z and beta are
// device arrays; the result goes to out_base + b n or to out_ptrs[b]; c_star_dev (optional) receives c*[b] through one batched reduction.
static int32_t ali_merge_batch_launch(stark_ctx* ctx, DevArena& X, size_t Bp, const fr_t* const* a, const fr_t* const* s, const fr_t* const* e, const fr_t* const* t,
                                      const fr_t* const* r_opt, const fr_t* beta, const fr_t& omega, const fr_t* z, size_t n, fr_t* out_base, fr_t* const* out_ptrs, fr_t* c_star_dev) {
    PowTable wp; STARK_TRY(omega_table(ctx, omega, n, &wp));
    const unsigned block = 256; const uint64_t lanes = (n + ALI_K - 1) / ALI_K; const unsigned grid = (unsigned)((lanes + block - 1) / block);
    const fr_t w_step = fr_pow_u64<PallasFr>(omega, (uint64_t)grid * block);
    fr_t* sums = nullptr; if (c_star_dev) { void* q = nullptr; STARK_TRY(X.alloc(Bp * grid * sizeof(fr_t), &q)); sums = (fr_t*)q; }
    hipLaunchKernelGGL(k_ali_merge_batch<PallasFr>, dim3(grid, (unsigned)Bp), dim3(block), 0, ctx->stream, a, s, e, t, r_opt, beta, wp, w_step, fr_inv<PallasFr>(w_step), z, (uint64_t)n, out_base, out_ptrs, sums);
    STARK_HIP(ctx, hipGetLastError());
    if (c_star_dev) {                                   // c*[b] = (1/n) * sum of trace b's block partials (lib.rs:44, :94)
        hipLaunchKernelGGL(k_sum_single_block<PallasFr>, dim3((unsigned)Bp), dim3(256), 0, ctx->stream, (const fr_t*)sums, (uint64_t)grid, fr_inv<PallasFr>(host::h_u64(n)), c_star_dev);
        STARK_HIP(ctx, hipGetLastError());
    }
    return STARK_OK;
}
// What a proof's MemoHasher of the query phase may still ask the device for: the reseed of fri.rs:379-381 alone (it cannot occur with power-of-two
// layers).  Anything else was to be pre-loaded; a request for it means the pre-loaded keys no longer match what fri_plan.hpp asks for, and is an error
// rather than a silent launch and synchronisation per proof (the constant of four synchronisations per pass rests on this).
struct ReseedOnlyHasher : TrHasher {
    DeviceHasher dev; explicit ReseedOnlyHasher(stark_ctx* c) : dev(c) {}
    int32_t hash(const char* tag, const fr_t* fields, size_t k, size_t n, fr_t* out) override {
        if (strcmp(tag, "FRI/index") || k != 2 || n != 1) return dev.ctx->fail(STARK_ERR_HIP, std::string("batched query phase: hash '") + tag + "' was not pre-loaded");
        return dev.hash(tag, fields, k, n, out);
    }
};
struct BatchArrays {                                    // the traces of a side-by-side pass
    const FriDevBatch& C; size_t r_;
    size_t traces() const { return C.Bp; }
    size_t n0(size_t) const { return C.n[0]; }
    size_t r(size_t) const { return r_; }
    size_t layers() const { return C.L + 1; }
    const fr_t* layer(size_t b, size_t l, size_t* len) const { *len = C.n[l]; return C.layer_at(b, l); }
    size_t levels(size_t, size_t l) const { return C.trees[l].levels.size(); }
    const fr_t* level(size_t b, size_t l, size_t v, size_t* len) const { *len = C.trees[l].lens[v]; return C.level_at(b, l, v); }
    int32_t roots_host(stark_ctx* ctx, std::vector<fr_t>& rt) const {
        const size_t Bp = C.Bp, R = C.L + 1; std::vector<fr_t> rl(R * Bp);                                               // C.roots is layer-major
        STARK_HIP(ctx, hipMemcpyAsync(rl.data(), C.roots, rl.size() * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        rt.resize(R * Bp); for (size_t b = 0; b < Bp; ++b) for (size_t l = 0; l < R; ++l) rt[b * R + l] = rl[l * Bp + b];
        return STARK_OK;
    }
};
// The executor of FriMixedCommit (fri_mixed.hpp) on the device: FriDevExec's arena, streams and launches, plus the ragged fold, the tables of a whole
// pass and the segment tables of the ragged climbs (as MerkleMixedDevExec has them).  Uploads run on the context's stream: one made while the side
// stream is current is followed by a fork of its own, so that the side stream's next launch waits for it.
struct FriMixedDevExec : FriDevExec {
    using FriDevExec::FriDevExec;
    int32_t zpows_many(const ZpowJob* jobs, size_t n_jobs, size_t max_m, fr_t* zp) {
        if (!n_jobs || !max_m) return STARK_OK;
        hipLaunchKernelGGL(k_zpows_many<PallasFr>, dim3((unsigned)((max_m + 63) / 64), (unsigned)n_jobs), dim3(64), 0, main_st, jobs, zp);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    int32_t fold_ragged(const fr_t* f, size_t n, const FoldSeg* segs, size_t n_seg, const fr_t* zp, size_t m, fr_t* out) {
        if (!is_pow2(m)) return ctx->fail(STARK_ERR_UNSUPPORTED, "ragged fold: m must be a power of two");     // every m divides a power-of-two n0
        const int log_m = ilog2(m), log_g = std::min(log_m, 4);
        const uint64_t lanes = (uint64_t)n >> (log_m - log_g);
        hipLaunchKernelGGL(k_fri_fold_ragged<PallasFr>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, main_st, f, (uint64_t)n, segs, (uint32_t)n_seg, zp, log_m, log_g, out);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** x) {
        DsRaggedStream::Seg* d = nullptr; STARK_TRY(put(h, &d)); *x = d;
        return cur != main_st ? fk.fork() : STARK_OK;
    }
    int32_t gather(const MerkleGatherList& G, fr_t* out) { return gather_rows(ctx, G, out, nullptr); }
};
typedef FriMixedCommit<FriMixedDevExec> FriDevMixed;
struct MixedArrays {                                    // the traces of a ragged pass: every proof has its own shape
    const FriDevMixed& C; const size_t* r_;
    size_t traces() const { return C.Bp; }
    size_t n0(size_t b) const { return C.n[b][0]; }
    size_t r(size_t b) const { return r_[b]; }
    size_t layers() const { return C.L + 1; }
    const fr_t* layer(size_t b, size_t l, size_t* len) const { *len = C.n[b][l]; return C.layer_at(b, l); }
    size_t levels(size_t b, size_t l) const { return C.levels(b, l); }
    const fr_t* level(size_t b, size_t l, size_t v, size_t* len) const { return C.level_at(b, l, v, len); }
    int32_t roots_host(stark_ctx* ctx, std::vector<fr_t>& rt) const {                                                    // C.roots is trace-major already
        rt.resize((C.L + 1) * C.Bp);
        STARK_HIP(ctx, hipMemcpyAsync(rt.data(), C.roots, rt.size() * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return STARK_OK;
    }
};
// THE query phase: fri_prove_queries + payload assembly + canonical encoding (fri.rs:355-466, 613-640) of every proof of a pass, read through the
// view V of its commit phase (one trace: StateArrays; side by side: BatchArrays; ragged: MixedArrays), which also gives every proof's own n0 and r
// (the seed and index arrays are sized by the sum of r_b * L, proof b's at its own offset; with equal shapes that is B r L as before).  The indices of every opened value depend only on the roots, so
// the phase first RECORDS what it will read (fri_plan.hpp: the same code against a recording source), fetches all of it — layer elements and tree
// nodes spread over every layer and level of every proof — with ONE gather, and then assembles the proofs from that list.  FOUR host
// synchronisations, whatever the number of traces: the roots; the "FRI/seed" hashes (one launch); the r * L "FRI/index" hashes per proof (one
// launch; none when r * L = 0); the opened values (one gather launch; none when nothing is opened).  Seeds and index seeds are pre-loaded into each
// proof's MemoHasher, so fri_plan_make and assemble_proof run per proof without touching the device (ReseedOnlyHasher).
template <class View> static int32_t batch_queries(stark_ctx* ctx, const View& V, const size_t* schedule, size_t L, std::unique_ptr<stark_proof>* out) {
    const size_t Bp = V.traces(), R = L + 1;
    std::vector<size_t> q0(Bp + 1, 0); for (size_t b = 0; b < Bp; ++b) q0[b + 1] = q0[b] + V.r(b) * L;                   // proof b's index seeds: [q0[b], q0[b + 1])
    const size_t q = q0[Bp];
    std::vector<fr_t> rt, seed(Bp), in(3 * q), idx(q);
    STARK_TRY(V.roots_host(ctx, rt));
    DevBuf d_rt, d_seed, d_in, d_idx;
    STARK_HIP(ctx, d_rt.alloc(ctx, rt.size() * sizeof(fr_t))); STARK_HIP(ctx, d_seed.alloc(ctx, Bp * sizeof(fr_t)));
    STARK_TRY(ctx_upload_staged(ctx, d_rt.p, rt.data(), rt.size() * sizeof(fr_t)));
    STARK_TRY(tr_hash_dev(ctx, "FRI/seed", d_rt.fr(), R, Bp, d_seed.fr()));                                               // fs_seed_from_roots, fri.rs:178
    STARK_HIP(ctx, d_seed.download_sync(seed.data(), Bp * sizeof(fr_t)));
    if (q) {                                                                                                             // the index seeds of all (proof, query, layer): fri.rs:374, :189-191
        for (size_t b = 0; b < Bp; ++b) for (size_t j = 0; j < V.r(b); ++j) for (size_t l = 0; l < L; ++l) { fr_t* p = &in[3 * (q0[b] + j * L + l)]; p[0] = seed[b]; p[1] = host::h_u64(l); p[2] = host::h_u64(j); }
        STARK_HIP(ctx, d_in.alloc(ctx, in.size() * sizeof(fr_t))); STARK_HIP(ctx, d_idx.alloc(ctx, q * sizeof(fr_t)));
        STARK_TRY(ctx_upload_staged(ctx, d_in.p, in.data(), in.size() * sizeof(fr_t)));
        STARK_TRY(tr_hash_dev(ctx, "FRI/index", d_in.fr(), 3, q, d_idx.fr()));
        STARK_HIP(ctx, d_idx.download_sync(idx.data(), q * sizeof(fr_t)));
    }
    ReseedOnlyHasher H0(ctx); std::vector<std::unique_ptr<MemoHasher>> H(Bp); std::vector<FriPlan> plan(Bp);
    std::vector<size_t> row0(Bp + 1, 0);
    MerkleGatherList G;                                                                                                  // row: the running count over all proofs
    for (size_t b = 0; b < Bp; ++b) {
        H[b].reset(new MemoHasher(H0));
        H[b]->preload("FRI/seed", &rt[b * R], R, 1, &seed[b]);
        if (q0[b + 1] > q0[b]) H[b]->preload("FRI/index", &in[3 * q0[b]], 3, q0[b + 1] - q0[b], &idx[q0[b]]);
        STARK_TRY(make_query_plan(ctx, plan[b], V.n0(b), schedule, L, &rt[b * R], V.r(b), *H[b]));
        for (const FriRequest& rq : plan[b].req) { const fr_t* from; size_t len; STARK_TRY(resolve_opening(ctx, V, b, rq, &from, &len)); STARK_TRY(add_opening(ctx, G, from, len, rq.index, G.size())); }
        row0[b + 1] = G.size();
    }
    std::vector<fr_t> vals(G.size());
    STARK_TRY(gather_rows(ctx, G, nullptr, vals.data()));                                                                // ONE gather over all proofs' requests, one download
    for (size_t b = 0; b < Bp; ++b) {
        out[b].reset(new stark_proof());
        STARK_TRY(assemble_from_values(ctx, plan[b].shape, V.r(b), *H[b], vals.data() + row0[b], row0[b + 1] - row0[b], out[b].get()));
    }
    return STARK_OK;
}
// All fold challenges of a ragged pass (fri.rs:250; FriMixedCommit::zkeys) before its first kernel: the "FRI/z/l" hashes of the keys the context has not seen
// yet are ONE tr_hash launch and one download; with every key cached nothing is launched.
static int32_t sample_z_many(stark_ctx* ctx, uint64_t seed_z, const std::vector<FriDevMixed::ZKey>& keys, std::vector<fr_t>& z) {
    std::vector<size_t> miss; std::vector<fr_t> in;
    z.assign(keys.size(), host::h_zero());
    for (size_t k = 0; k < keys.size(); ++k) {
        auto it = ctx->z_cache.find(stark_ctx::ZKey{seed_z, keys[k].l, keys[k].n});
        if (it != ctx->z_cache.end()) { z[k] = it->second; continue; }
        miss.push_back(k); in.push_back(host::h_u64(seed_z)); in.push_back(host::h_u64(keys[k].l)); in.push_back(host::h_u64(keys[k].n));
    }
    if (miss.empty()) return STARK_OK;
    DevBuf d_in, d_out; std::vector<fr_t> fused(miss.size());
    STARK_HIP(ctx, d_in.alloc(ctx, in.size() * sizeof(fr_t))); STARK_HIP(ctx, d_out.alloc(ctx, miss.size() * sizeof(fr_t)));
    STARK_TRY(ctx_upload_staged(ctx, d_in.p, in.data(), in.size() * sizeof(fr_t)));
    STARK_TRY(tr_hash_dev(ctx, "FRI/z/l", d_in.fr(), 3, miss.size(), d_out.fr()));
    STARK_HIP(ctx, d_out.download_sync(fused.data(), miss.size() * sizeof(fr_t)));
    for (size_t i = 0; i < miss.size(); ++i) {
        const FriDevMixed::ZKey& K = keys[miss[i]];
        z[miss[i]] = fri_z_from_fused(fused[i], seed_z, K.l, K.n); ctx->z_cache[stark_ctx::ZKey{seed_z, K.l, K.n}] = z[miss[i]];
    }
    return STARK_OK;
}
// Shapes, constants, challenges and buffers of a ragged pass: everything that may upload constants or synchronise, before the first launch.
static int32_t mixed_commit_begin(stark_ctx* ctx, FriDevMixed& M, size_t Bp, const size_t* n0, const size_t* schedule, size_t L, uint64_t seed_z) {
    std::string err; const int32_t rc = M.shape(Bp, n0, schedule, L, err);
    if (rc == -2) return ctx->fail(STARK_ERR_UNSUPPORTED, err); if (rc) return ctx->fail(STARK_ERR_INVALID_ARG, err);
    stark_params* p = nullptr; STARK_TRY(ctx_transcript_params(ctx, &p));
    for (const auto& layer : M.parts) for (const auto& part : layer) STARK_TRY(ctx_merkle_params(ctx, host::width_for_arity(part.arity), &p));
    std::vector<fr_t> z; STARK_TRY(sample_z_many(ctx, seed_z, M.zkeys, z));
    return M.init(z.data());
}
// deep_ali_merge_evals_blinded (no blinding) of Bp traces of DIFFERENT lengths in one launch (k_ali_merge_ragged): trace b of n0[b] rows with its own z and
// generator goes to f0 + at0[b].  One power table, the largest domain's.  The check of every z against its own H (lib.rs:78) is the caller's.
static int32_t ali_merge_ragged_launch(stark_ctx* ctx, DevArena& X, size_t Bp, const uint64_t* const* const cols[4], const fr_t* zs, const size_t* n0, const size_t* at0, fr_t* f0) {
    const size_t n_max = *std::max_element(n0, n0 + Bp);
    PowTable wp; STARK_TRY(omega_table(ctx, fr_root_of_unity<PallasFr>((unsigned)ilog2(n_max)), n_max, &wp));
    const unsigned block = 256; unsigned grid = 1;
    std::vector<AliRaggedJob> jobs(Bp);
    for (size_t b = 0; b < Bp; ++b) {
        const uint64_t lanes = (n0[b] + ALI_K - 1) / ALI_K, blocks = (lanes + block - 1) / block;
        const fr_t w_step = fr_pow_u64<PallasFr>(fr_root_of_unity<PallasFr>((unsigned)ilog2(n0[b])), blocks * block);
        jobs[b] = AliRaggedJob{as_fr(cols[0][b]), as_fr(cols[1][b]), as_fr(cols[2][b]), as_fr(cols[3][b]), zs[b], w_step, fr_inv<PallasFr>(w_step), (uint64_t)n0[b], (uint64_t)at0[b], (uint64_t)(n_max / n0[b])};
        grid = std::max(grid, (unsigned)blocks);
    }
    AliRaggedJob* d = nullptr; STARK_TRY(X.put(jobs, &d));
    hipLaunchKernelGGL(k_ali_merge_ragged<PallasFr>, dim3(grid, (unsigned)Bp), dim3(block), 0, ctx->stream, (const AliRaggedJob*)d, wp, f0);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
// Layer 0 and the commit phase of one pass of Bp >= 1 traces, in the three forms of the commit, chosen HERE and nowhere else:
//   one trace      fri_build_impl — the stark_fri_state that stark_fri_build_dev hands out and the benchmark step runs through, and the only
//                  commit whose levels are DsStreams (k_node16_pair, the "fri_side_pair" form); layer 0 is the caller's f0 or ali_merge_dev_impl's;
//   side by side   FriDevBatch (fri_batch.hpp) — traces of one n0; layer 0 of every trace from one copy kernel or the batched merge;
//   ragged         FriDevMixed (fri_mixed.hpp) — traces of one schedule and any n0 (`ragged`: the classes of "mixed_prove_tail"); layer 0 from the ragged merge.
// No form synchronises the host after its prelude.  Whatever reads the result goes through with_view and does not know which form ran.
struct PassCommit {
    stark_ctx* ctx; FriDevExec X; FriDevBatch C; std::unique_ptr<stark_fri_state> S; FriMixedDevExec XM; FriDevMixed M; bool ragged_ran = false;
    explicit PassCommit(stark_ctx* c) : ctx(c), X(c), C(X), XM(c), M(XM) {}
    // cols: host tables of device pointers a, s, e, t with the traces' z on the host (zs), or f0: a host table of device pointers.  n0s: the traces' rows, all
    // equal unless `ragged` (which needs cols).  *t_layer0 (optional): when layer 0 was enqueued.
    int32_t run(size_t Bp, const uint64_t* const* const cols[4], const fr_t* zs, const uint64_t* const* f0, const size_t* n0s, bool ragged, const size_t* schedule, size_t L, uint64_t seed_z,
                Clock::time_point* t_layer0) {
        const size_t n0 = n0s[0];
        const fr_t omega = fr_root_of_unity<PallasFr>((unsigned)ilog2(n0));
        if (Bp == 1) {
            DevBuf merged; const fr_t* f = f0 ? as_fr(f0[0]) : nullptr;
            if (!f) {
                if (merged.alloc(ctx, n0 * sizeof(fr_t)) != hipSuccess) return ctx->fail(STARK_ERR_OOM, "f0: " + ctx->err);
                STARK_TRY(ali_merge_dev_impl(ctx, as_fr(cols[0][0]), as_fr(cols[1][0]), as_fr(cols[2][0]), as_fr(cols[3][0]), nullptr, host::h_zero(), omega, zs[0], n0, merged.fr(), nullptr));
                f = merged.fr();
            }
            if (t_layer0) *t_layer0 = Clock::now();
            return fri_build_impl(ctx, f, n0, schedule, L, seed_z, S);       // copies f: `merged` returns to the pool behind that copy
        }
        if (ragged) {
            if (!cols) return ctx->fail(STARK_ERR_INVALID_ARG, "ragged pass: columns needed");
            for (size_t b = 0; b < Bp; ++b) if (fr_eq(fr_pow_u64<PallasFr>(zs[b], n0s[b]), host::h_one())) return ctx->fail(STARK_ERR_INVALID_ARG, "z must be outside H");   // lib.rs:78, before any launch
            STARK_TRY(mixed_commit_begin(ctx, M, Bp, n0s, schedule, L, seed_z));
            ragged_ran = true;
            STARK_TRY(ali_merge_ragged_launch(ctx, XM, Bp, cols, zs, n0s, M.at[0].data(), M.f[0]));
            if (t_layer0) *t_layer0 = Clock::now();
            return M.run();
        }
        STARK_TRY(batch_commit_begin(ctx, C, Bp, n0, schedule, L, seed_z));
        if (f0) STARK_TRY(batch_fill_layer0(ctx, X, C, f0));
        else {
            for (size_t b = 0; b < Bp; ++b) if (fr_eq(fr_pow_u64<PallasFr>(zs[b], n0), host::h_one())) return ctx->fail(STARK_ERR_INVALID_ARG, "z must be outside H");   // lib.rs:78
            std::vector<const fr_t*> tab(4 * Bp); for (int c = 0; c < 4; ++c) for (size_t b = 0; b < Bp; ++b) tab[c * Bp + b] = as_fr(cols[c][b]);
            const fr_t** d_tab = nullptr; fr_t* d_z = nullptr; STARK_TRY(X.put(tab, &d_tab)); STARK_TRY(X.put(std::vector<fr_t>(zs, zs + Bp), &d_z));
            STARK_TRY(ali_merge_batch_launch(ctx, X, Bp, d_tab, d_tab + Bp, d_tab + 2 * Bp, d_tab + 3 * Bp, nullptr, nullptr, omega, d_z, n0, C.f[0], nullptr, nullptr));
        }
        if (t_layer0) *t_layer0 = Clock::now();
        return C.run();
    }
    // rs: the traces' query counts (all equal unless the ragged form ran)
    template <class F> int32_t with_view(const size_t* rs, F f) const { return S ? f(StateArrays{S.get(), rs[0]}) : ragged_ran ? f(MixedArrays{M, rs}) : f(BatchArrays{C, rs[0]}); }
};
// One pass of a batch prove: layer 0 -> commit phase -> query phase -> stage times.  Host synchronisations per pass: the FOUR of batch_queries, whatever
// Bp (layer 0 and the commit phase only enqueue).  stage_ms of every proof of the pass: shared_ms + the pass's layer 0, its commit, its queries.
// n0s / rs: the traces' rows and query counts, all equal unless `ragged`.
static int32_t prove_pass(stark_ctx* ctx, size_t Bp, const uint64_t* const* const cols[4], const fr_t* zs, const uint64_t* const* f0, const size_t* n0s, bool ragged,
                          const size_t* schedule, size_t L, const size_t* rs, uint64_t seed_z, double shared_ms, std::unique_ptr<stark_proof>* out) {
    const auto u0 = Clock::now(); auto u1 = u0;
    PassCommit P(ctx);
    STARK_TRY(P.run(Bp, cols, zs, f0, n0s, ragged, schedule, L, seed_z, &u1));
    const auto u2 = Clock::now();
    const int32_t rc = P.with_view(rs, [&](const auto& V) { return batch_queries(ctx, V, schedule, L, out); });
    P.S.reset();                                                                            // a single state's layers and trees go back to the pool here, before the proofs are handed out
    if (rc) return rc;
    const auto u3 = Clock::now();
    for (size_t b = 0; b < Bp; ++b) { out[b]->ms[0] = shared_ms + ms_between(u0, u1); out[b]->ms[1] = ms_between(u1, u2); out[b]->ms[2] = ms_between(u2, u3); }
    return STARK_OK;
}
// stark_deep_fri_prove_f0_batch_dev, and stark_deep_fri_prove_dev given f0 with B = 1: the batch cut into passes of at most "prove_batch_max_rows" rows.
static int32_t prove_f0_batch_impl(stark_ctx* ctx, size_t B, const uint64_t* const* f0, size_t n0, const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof** out) {
    const size_t per = pass_traces(ctx, n0); const std::vector<size_t> nn(std::min(per, B), n0), rr(std::min(per, B), r);
    std::vector<std::unique_ptr<stark_proof>> pf(B);
    for (size_t p0 = 0; p0 < B; p0 += per) STARK_TRY(prove_pass(ctx, std::min(per, B - p0), nullptr, nullptr, f0 + p0, nn.data(), false, schedule, L, rr.data(), seed_z, 0.0, pf.data() + p0));
    hand_out(pf, out); return STARK_OK;
}
// stark_fri_commit_batch_dev: the roots of fri_build of every trace, roots[(b (L + 1) + l) * 4 ..]; one synchronisation per pass.
static int32_t commit_batch_impl(stark_ctx* ctx, size_t B, const uint64_t* const* f0, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, uint64_t* roots) {
    const size_t per = pass_traces(ctx, n0), R = L + 1;
    for (size_t p0 = 0; p0 < B; p0 += per) {
        const size_t Bp = std::min(per, B - p0);
        PassCommit P(ctx); std::vector<fr_t> rt; const std::vector<size_t> nn(Bp, n0); const size_t no_queries = 0;
        STARK_TRY(P.run(Bp, nullptr, nullptr, f0 + p0, nn.data(), false, schedule, L, seed_z, nullptr));
        STARK_TRY(P.with_view(&no_queries, [&](const auto& V) { return V.roots_host(ctx, rt); }));
        for (size_t i = 0; i < Bp * R; ++i) store_fr(roots + 4 * (p0 * R + i), rt[i]);
    }
    return STARK_OK;
}
// stark_ali_merge_batch_dev: tables of `batch` device pointers (host), z / beta on the host; kMaxPassTraces traces per launch.
static int32_t ali_merge_batch_impl(stark_ctx* ctx, size_t B, const uint64_t* const* a, const uint64_t* const* s, const uint64_t* const* e, const uint64_t* const* t, const uint64_t* const* r_opt,
                                    const uint64_t* beta, const fr_t& omega, const uint64_t* z, size_t n, uint64_t* const* f0, uint64_t* c_star) {
    DevArena X(ctx);
    std::vector<const fr_t*> tab(5 * B, nullptr); std::vector<fr_t*> outp(B); std::vector<fr_t> zb(2 * B, host::h_zero()), cs(B);
    bool blinded = false;
    for (size_t b = 0; b < B; ++b) {
        tab[b] = as_fr(a[b]); tab[B + b] = as_fr(s[b]); tab[2 * B + b] = as_fr(e[b]); tab[3 * B + b] = as_fr(t[b]);
        if (r_opt && r_opt[b]) { tab[4 * B + b] = as_fr(r_opt[b]); zb[B + b] = load_fr(beta + 4 * b); blinded = true; }
        outp[b] = as_fr(f0[b]); zb[b] = load_fr(z + 4 * b);
    }
    const fr_t** d_tab = nullptr; fr_t** d_out = nullptr; fr_t *d_zb = nullptr, *d_cs = nullptr;
    STARK_TRY(X.put(tab, &d_tab)); STARK_TRY(X.put(outp, &d_out)); STARK_TRY(X.put(zb, &d_zb));
    if (c_star) { void* q = nullptr; STARK_TRY(X.alloc(B * sizeof(fr_t), &q)); d_cs = (fr_t*)q; }
    for (size_t b0 = 0; b0 < B; b0 += kMaxPassTraces) {
        const size_t Bp = std::min(kMaxPassTraces, B - b0);
        STARK_TRY(ali_merge_batch_launch(ctx, X, Bp, d_tab + b0, d_tab + B + b0, d_tab + 2 * B + b0, d_tab + 3 * B + b0, blinded ? d_tab + 4 * B + b0 : nullptr, d_zb + B + b0, omega, d_zb + b0, n,
                                         nullptr, d_out + b0, d_cs ? d_cs + b0 : nullptr));
    }
    STARK_TRY(X.download(cs.data(), d_cs, c_star ? B * sizeof(fr_t) : 0));       // the caller reads f0 and c_star on return
    if (c_star) for (size_t b = 0; b < B; ++b) store_fr(c_star + 4 * b, cs[b]);
    return STARK_OK;
}

// ---- lagrange_eval_on_h of device-resident columns (deep_ali/src/lib.rs:17-45; lagrange_dev.hpp) -----------------------------------------------
// (n, omega4) of a lagrange_eval entry point: *omega = the caller's generator or the radix-2 one of size n
static int32_t lagrange_check_domain(stark_ctx* ctx, size_t n, const uint64_t* omega4, fr_t* omega) {
    if (!is_pow2(n) || n > ((size_t)1 << kLagMaxLogN)) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: n must be a power of two, 1 <= n <= 2^30");
    *omega = omega4 ? load_fr(omega4) : fr_root_of_unity<PallasFr>((unsigned)ilog2(n));       // FriDomain::new_radix2(n).omega, fri.rs:53-56
    if (const char* why = lag_check_domain(n, *omega)) return ctx->fail(STARK_ERR_INVALID_ARG, std::string("lagrange_eval: ") + why);
    return STARK_OK;
}
// The executor of lagrange_eval_batch on the device: the arena's memory, every launch on the context's stream.
struct LagDevExec : DevArena {
    explicit LagDevExec(stark_ctx* c) : DevArena(c) {}
    int32_t pow_table(const fr_t& omega, size_t n, LagPow* out) {                        // the merge's table of this domain (PowCache): a prove that merged over it has filled it
        PowTable t; STARK_TRY(omega_table(ctx, omega, n, &t)); *out = LagPow{t.lo, t.hi, t.lo_bits}; return STARK_OK;
    }
    int32_t gather(const fr_t* const* cols, size_t ncols, const uint64_t* j, const uint64_t* slot, size_t cnt, fr_t* out) {
        hipLaunchKernelGGL(k_lagrange_gather, dim3((unsigned)((cnt * ncols + 255) / 256)), dim3(256), 0, ctx->stream, cols, (uint64_t)ncols, j, slot, (uint64_t)cnt, out);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    int32_t totals(size_t n_local, uint64_t j0, const LagPow& wp, const fr_t& w_step, const fr_t* zs, size_t npts, unsigned grid, fr_t* tot) {
        hipLaunchKernelGGL(k_lagrange_totals, dim3(grid, (unsigned)std::min<size_t>(npts, 65535)), dim3(256), 0, ctx->stream, (uint64_t)n_local, j0, wp, w_step, zs, (uint64_t)npts, tot);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    int32_t invert(const fr_t* tot, size_t npts, unsigned grid, fr_t* inv) {
        hipLaunchKernelGGL(k_lagrange_invert, dim3((unsigned)npts), dim3(256), 0, ctx->stream, tot, (uint64_t)grid, inv);       // one workgroup per point; a pass has at most 2^28 ("lagrange_max_partials")
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    template <bool WIDE, bool SHARED, bool COSETS>
    void launch_partials(const dim3& g, const fr_t* const* cols, size_t ncols, size_t n_local, uint64_t j0, const LagPow& wp, const fr_t& w_step, const fr_t& w_step_inv, const fr_t* zs, size_t npts,
                         const LagEntries& E, const fr_t* inv, size_t group_cols, fr_t* part) {
        hipLaunchKernelGGL((k_lagrange_partials<WIDE, SHARED, COSETS>), g, dim3(256), 0, ctx->stream, cols, (uint64_t)ncols, (uint64_t)n_local, j0, wp, w_step, w_step_inv, zs, (uint64_t)npts, E, inv,
                           (uint64_t)group_cols, part);
    }
    // zs: the npts classes of the launch (E.off null: every class one point); inv null: every workgroup inverts its own product, else the table of `invert`
    int32_t partials(const fr_t* const* cols, size_t ncols, size_t n_local, uint64_t j0, const LagPow& wp, const fr_t& w_step, const fr_t& w_step_inv, const fr_t* zs, size_t npts, const LagEntries& E,
                     const fr_t* inv, unsigned groups, unsigned col_groups, size_t group_cols, unsigned grid, fr_t* part) {
        const bool wide = ctx->opt.lagrange_wide_acc < 0 ? kLagWideAcc : ctx->opt.lagrange_wide_acc != 0;
        const dim3 g(grid, groups, col_groups);
#define STARK_LAG_PARTIALS(W, S, C) launch_partials<W, S, C>(g, cols, ncols, n_local, j0, wp, w_step, w_step_inv, zs, npts, E, inv, group_cols, part)
        switch ((wide ? 4 : 0) | (inv ? 2 : 0) | (E.off ? 1 : 0)) {
            case 0: STARK_LAG_PARTIALS(false, false, false); break;
            case 1: STARK_LAG_PARTIALS(false, false, true); break;
            case 2: STARK_LAG_PARTIALS(false, true, false); break;
            case 3: STARK_LAG_PARTIALS(false, true, true); break;
            case 4: STARK_LAG_PARTIALS(true, false, false); break;
            case 5: STARK_LAG_PARTIALS(true, false, true); break;
            case 6: STARK_LAG_PARTIALS(true, true, false); break;
            default: STARK_LAG_PARTIALS(true, true, true); break;
        }
#undef STARK_LAG_PARTIALS
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    int32_t finish(const fr_t* part, unsigned grid, const fr_t* scale, const uint64_t* slot, size_t npts, size_t ncols, fr_t* out) {
        hipLaunchKernelGGL(k_lagrange_finish, dim3((unsigned)(npts * ncols)), dim3(256), 0, ctx->stream, part, (uint64_t)grid, scale, slot, (uint64_t)ncols, out);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    int32_t combine(const fr_t* partials, size_t nparts, const fr_t* scale, size_t npoints, size_t ncols, fr_t* out) {
        const uint64_t total = (uint64_t)npoints * ncols;
        hipLaunchKernelGGL(k_lagrange_combine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, partials, (uint64_t)nparts, scale, total, (uint64_t)ncols, out);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
};
// The argument checks of the lagrange_eval entry points, all before anything is enqueued: ncols columns of col_len rows each (the whole column, or a
// block of it) over a domain of n points, results into `out_elems` elements at out.  *omega = the caller's generator or the radix-2 one of size n.
static int32_t lagrange_check_args(stark_ctx* ctx, size_t ncols, const uint64_t* const* cols, size_t col_len, size_t n, const uint64_t* omega4, size_t npoints, const uint64_t* z, const uint64_t* out,
                                   size_t out_elems, fr_t* omega) {
    if (!cols) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: null column table");
    if (!out) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: null out");
    if (!z) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: null z with npoints > 0");
    STARK_TRY(lagrange_check_domain(ctx, n, omega4, omega));
    if (ncols > kLagMaxCols) return ctx->fail(STARK_ERR_UNSUPPORTED, "lagrange_eval: more than 2^24 columns in one call");
    if (npoints > ((size_t)1 << 36) / ncols) return ctx->fail(STARK_ERR_UNSUPPORTED, "lagrange_eval: more than 2^36 results in one call");
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + out_elems * sizeof(fr_t), cbytes = col_len * sizeof(fr_t);
    for (size_t c = 0; c < ncols; ++c) {
        if (!cols[c]) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: null column entry " + std::to_string(c));
        const uintptr_t c0 = (uintptr_t)cols[c];
        if (c0 < o1 && o0 < c0 + cbytes) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: out overlaps column " + std::to_string(c));
    }
    return STARK_OK;
}
static std::vector<fr_t> lagrange_points(size_t npoints, const uint64_t* z) { std::vector<fr_t> zs(npoints); for (size_t p = 0; p < npoints; ++p) zs[p] = load_fr(z + 4 * p); return zs; }
// the block B of the columns `cols` (a host table of device pointers to the block's rows) through THE driver; B = lag_whole(n): the batch call
static int32_t lagrange_eval_block_impl(stark_ctx* ctx, size_t ncols, const uint64_t* const* cols, const LagBlock& B, const fr_t& omega, const std::vector<fr_t>& zs, fr_t* out) {
    std::vector<const fr_t*> cp(ncols); for (size_t c = 0; c < ncols; ++c) cp[c] = as_fr(cols[c]);
    LagDevExec X(ctx);
    return lagrange_eval_batch(X, ncols, cp.data(), B, omega, zs.size(), zs.data(), ctx->opt.lagrange_max_partials, ctx->opt.lagrange_col_groups, ctx->opt.lagrange_shared_inverse, ctx->opt.lagrange_share_cosets, out, nullptr);
}

// ---- lagrange_eval_on_h of columns block-sharded over the ranks of a ShardColl: block partials, ONE all-gather of the W tables, the combine --------
// One driver for the communicator's rank (stark_lagrange_eval_on_h_sharded_dev) and for W ranks emulated on one GPU
// (stark_diag_lagrange_eval_sharded_emulated_dev).  cols[c]: this rank's rows [q n/W, (q+1) n/W) of column c, or the whole column when C is emulated;
// out: npoints x ncols per local rank.  The arguments have passed lagrange_check_args.  Collective 0 is the header: ranks that were given a different
// (n, ncols, npoints, omega, z) all return STARK_ERR_INVALID_ARG (the rule of shard_header_agree, fri_shard_impl.hpp).
static int32_t lagrange_sharded(const ShardColl& C, size_t ncols, const uint64_t* const* cols, size_t n, const fr_t& omega, const std::vector<fr_t>& zs, fr_t* out) {
    stark_ctx* ctx = C.ctx; const size_t W = (size_t)C.W, nl = n / W, total = zs.size() * ncols, chunk = total * sizeof(fr_t), hbytes = kLagHdrWords * 8;
    uint64_t h[kLagHdrWords]; lag_shard_header(n, ncols, zs.size(), omega, zs.data(), h);
    {
        std::vector<DevBuf> hb(C.local()); std::vector<void*> buf;
        for (size_t i = 0; i < hb.size(); ++i) {
            STARK_TRY(hb[i].take(ctx, W * hbytes));
            STARK_TRY(ctx_upload_staged(ctx, (char*)hb[i].p + (size_t)C.rank(i) * hbytes, h, hbytes));
            buf.push_back(hb[i].p);
        }
        STARK_TRY(C.all_gather(buf, hbytes));
        std::vector<uint64_t> all(W * kLagHdrWords); bool same = true;
        for (auto& b : hb) { STARK_HIP(ctx, b.download_sync(all.data(), W * hbytes)); same = same && lag_headers_agree(all.data(), W, h); }
        if (!same) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval sharded: the ranks disagree on (n_global, ncols, npoints, omega, z)");
    }
    std::vector<DevBuf> tab(C.local()); std::vector<void*> buf; std::vector<const uint64_t*> blk(ncols);
    for (size_t i = 0; i < tab.size(); ++i) {                  // in place: this rank's table sits at rank * chunk of its W tables
        STARK_TRY(tab[i].take(ctx, W * chunk)); buf.push_back(tab[i].p);
        for (size_t c = 0; c < ncols; ++c) blk[c] = cols[c] + 4 * C.block(i) * nl;
        STARK_TRY(lagrange_eval_block_impl(ctx, ncols, blk.data(), LagBlock{nl, (uint64_t)C.rank(i) * nl, n, false}, omega, zs, tab[i].fr() + (size_t)C.rank(i) * total));
    }
    STARK_TRY(C.all_gather(buf, chunk));
    for (size_t i = 0; i < tab.size(); ++i) { LagDevExec X(ctx); STARK_TRY(lagrange_combine(X, W, (const fr_t*)tab[i].fr(), ncols, n, zs.size(), zs.data(), out + C.block(i) * total)); }
    return STARK_OK;
}

// B independent proofs of equal shape (stark_deep_fri_prove_batch_dev; stark_deep_fri_prove_dev from columns is B = 1): the challenge stage of all
// traces at once, then merge, commit phase and query phase pass by pass (prove_pass).
// Every proof is byte-for-byte what stark_deep_fri_prove_dev returns for that trace alone.
static int32_t prove_batch_impl(stark_ctx* ctx, size_t B, const uint64_t* const* a, const uint64_t* const* s, const uint64_t* const* e, const uint64_t* const* t, size_t n0,
                                const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof** out) {
    if (!is_pow2(n0)) return ctx->fail(STARK_ERR_INVALID_ARG, "n0 must be a power of two (radix-2 domain)");
    if (n0 <= 1) return ctx->fail(STARK_ERR_INVALID_ARG, "n0 > 1");
    for (size_t p = 0; p < B; ++p) out[p] = nullptr;
    const auto t0 = Clock::now();
    std::vector<const fr_t*> ptrs(4 * B);
    for (size_t p = 0; p < B; ++p) { ptrs[4 * p] = as_fr(a[p]); ptrs[4 * p + 1] = as_fr(s[p]); ptrs[4 * p + 2] = as_fr(e[p]); ptrs[4 * p + 3] = as_fr(t[p]); }
    AliChallenges ch; STARK_TRY(challenge_stage(ctx, B, ptrs.data(), n0, ch));
    const double shared_ms = ms_between(t0, Clock::now());
    const size_t per = pass_traces(ctx, n0); const std::vector<size_t> nn(std::min(per, B), n0), rr(std::min(per, B), r);
    std::vector<std::unique_ptr<stark_proof>> pf(B);
    for (size_t p0 = 0; p0 < B; p0 += per) {
        const uint64_t* const* const cols[4] = {a + p0, s + p0, e + p0, t + p0};
        STARK_TRY(prove_pass(ctx, std::min(per, B - p0), cols, ch.z.data() + p0, nullptr, nn.data(), false, schedule, L, rr.data(), seed_z, shared_ms, pf.data() + p0));
    }
    hand_out(pf, out); return STARK_OK;
}

// B independent proofs of ANY shapes (stark_deep_fri_prove_mixed_batch_dev): trace i has n0[i] rows, folds by schedule[sched_off[i] .. sched_off[i + 1])
// and answers r[i] queries.  The challenge stage of all traces at once — the 4 B column sponges side by side in one Ragged launch, which is where
// the time of a prove is — then, chosen HERE by the option "mixed_prove_tail":
//   0 (default)  the traces of equal (n0, schedule, r) together (mixed_prove_groups, fri_plan.hpp), each group through the passes of the equal-shape batch;
//   1            the traces of equal SCHEDULE together (mixed_prove_classes), each class through ragged passes (fri_mixed.hpp): one merge, one commit
//                phase and one query phase per pass whatever the sizes and query counts in it.
// Either way a group or class is cut into passes of consecutive traces of at most "prove_batch_max_rows" rows (mixed_prove_passes) that go through
// prove_pass, and a pass of one trace takes the single commit.  No merge, commit or query code of its own.
// stage_ms[0] of a proof: the challenge stage of the whole batch + its pass's layer 0; [1], [2]: its pass's commit and queries.
// The arguments were checked by the entry point.  Every proof is byte-for-byte what stark_deep_fri_prove_dev returns for that trace alone.
static int32_t prove_mixed_batch_impl(stark_ctx* ctx, size_t B, const uint64_t* const* a, const uint64_t* const* s, const uint64_t* const* e, const uint64_t* const* t, const size_t* n0,
                                      const size_t* schedule, const size_t* sched_off, const size_t* r, uint64_t seed_z, stark_proof** out) {
    const auto t0 = Clock::now();
    std::vector<const fr_t*> ptrs(4 * B);
    for (size_t p = 0; p < B; ++p) { ptrs[4 * p] = as_fr(a[p]); ptrs[4 * p + 1] = as_fr(s[p]); ptrs[4 * p + 2] = as_fr(e[p]); ptrs[4 * p + 3] = as_fr(t[p]); }
    AliChallenges ch; STARK_TRY(challenge_stage(ctx, B, ptrs.data(), n0, ch));
    const double shared_ms = ms_between(t0, Clock::now());
    std::vector<std::unique_ptr<stark_proof>> pf(B);
    const bool ragged = ctx->opt.mixed_prove_tail;
    for (const std::vector<size_t>& G : ragged ? mixed_prove_classes(B, schedule, sched_off) : mixed_prove_groups(B, n0, schedule, sched_off, r)) {
        const size_t g0 = G[0], Bg = G.size(), L = sched_off[g0 + 1] - sched_off[g0];
        const size_t* sched = L ? schedule + sched_off[g0] : nullptr;
        std::vector<const uint64_t*> tab[4]; std::vector<fr_t> zs(Bg); std::vector<size_t> nn(Bg), rr(Bg); std::vector<std::unique_ptr<stark_proof>> gp(Bg);
        for (size_t j = 0; j < Bg; ++j) { tab[0].push_back(a[G[j]]); tab[1].push_back(s[G[j]]); tab[2].push_back(e[G[j]]); tab[3].push_back(t[G[j]]); zs[j] = ch.z[G[j]]; nn[j] = n0[G[j]]; rr[j] = r[G[j]]; }
        size_t p0 = 0;
        for (const size_t Bp : mixed_prove_passes(Bg, nn.data(), ctx->opt.prove_batch_max_rows, kMaxPassTraces)) {
            const uint64_t* const* const cols[4] = {tab[0].data() + p0, tab[1].data() + p0, tab[2].data() + p0, tab[3].data() + p0};
            STARK_TRY(prove_pass(ctx, Bp, cols, zs.data() + p0, nullptr, nn.data() + p0, ragged, sched, L, rr.data() + p0, seed_z, shared_ms, gp.data() + p0));
            p0 += Bp;
        }
        for (size_t j = 0; j < Bg; ++j) pf[G[j]] = std::move(gp[j]);
    }
    hand_out(pf, out); return STARK_OK;
}

extern "C" {

int32_t stark_fri_sample_z(stark_ctx_t* ctx, stark_params_t* tp, uint64_t seed_z, size_t level, size_t domain_size, uint64_t* z4) {
    if (!ctx || !z4) return STARK_ERR_INVALID_ARG; (void)tp;
    fr_t z; STARK_TRY(sample_z(ctx, seed_z, level, domain_size, &z)); store_fr(z4, z); return STARK_OK;
}
int32_t stark_fri_fold_dev(stark_ctx_t* ctx, const uint64_t* f, size_t n, const uint64_t* z4, size_t m, uint64_t* out) {
    if (!ctx || !z4 || (!f && n) || (!out && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return fold_dev(ctx, as_fr(f), n, load_fr(z4), m, as_fr(out));
}
int32_t stark_fri_fold(stark_ctx_t* ctx, const uint64_t* f, size_t n, const uint64_t* z4, size_t m, uint64_t* out) {
    if (!ctx || !z4 || (!f && n) || (!out && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (m < 2) return ctx->fail(STARK_ERR_INVALID_ARG, "m >= 2"); if (n % m) return ctx->fail(STARK_ERR_INVALID_ARG, "layer size must be divisible by m");
    DevBuf df, dout; CallerUploads up(ctx); STARK_HIP(ctx, up.up(df, f, n * sizeof(fr_t))); STARK_HIP(ctx, dout.alloc(ctx, n / m * sizeof(fr_t)));
    STARK_TRY(fold_dev(ctx, df.fr(), n, load_fr(z4), m, dout.fr()));
    STARK_HIP(ctx, up.download_sync(out, dout.p, n / m * sizeof(fr_t))); return STARK_OK;
}
int32_t stark_fri_build_dev(stark_ctx_t* ctx, const uint64_t* f0, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, stark_fri_state_t** out) {
    if (!ctx || !f0 || !out || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    std::unique_ptr<stark_fri_state> S; STARK_TRY(fri_build_impl(ctx, as_fr(f0), n0, schedule, L, seed_z, S));
    *out = S.release(); return STARK_OK;
}
int32_t stark_fri_build(stark_ctx_t* ctx, const uint64_t* f0, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, stark_fri_state_t** out) {
    if (!ctx || !f0 || !out || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    DevBuf d; CallerUploads up(ctx); STARK_HIP(ctx, up.up(d, f0, n0 * sizeof(fr_t)));
    std::unique_ptr<stark_fri_state> S; STARK_TRY(fri_build_impl(ctx, d.fr(), n0, schedule, L, seed_z, S));
    STARK_HIP(ctx, up.sync());                                      // fri_build_impl only enqueues: the device has read f0 from here on
    *out = S.release(); return STARK_OK;
}
int32_t stark_fri_num_layers(stark_fri_state_t* s) { return s ? (int32_t)s->f.size() : STARK_ERR_INVALID_ARG; }
size_t stark_fri_layer_len(stark_fri_state_t* s, int32_t l) { return (s && l >= 0 && (size_t)l < s->n.size()) ? s->n[l] : 0; }
int32_t stark_fri_layer_f(stark_fri_state_t* s, int32_t l, uint64_t* out) {
    if (!s || !out || l < 0 || (size_t)l >= s->f.size()) return STARK_ERR_INVALID_ARG; stark_ctx* ctx = s->ctx;
    STARK_HIP(ctx, hipMemcpyAsync(out, s->f[l].p, s->n[l] * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream)); return STARK_OK;
}
int32_t stark_fri_layer_root(stark_fri_state_t* s, int32_t l, uint64_t* out4) {
    if (!s || !out4 || l < 0 || (size_t)l >= s->trees.size()) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(s->ctx)); STARK_TRY(state_roots(s)); store_fr(out4, s->roots[l]); return STARK_OK;
}
int32_t stark_fri_layer_z(stark_fri_state_t* s, int32_t l, uint64_t* out4) { if (!s || !out4 || l < 0 || (size_t)l >= s->z.size()) return STARK_ERR_INVALID_ARG; store_fr(out4, s->z[l]); return STARK_OK; }
stark_tree_t* stark_fri_layer_tree(stark_fri_state_t* s, int32_t l) { return (s && l >= 0 && (size_t)l < s->trees.size()) ? s->trees[l].get() : nullptr; }
int32_t stark_fri_state_free(stark_fri_state_t* s) { if (!s) return STARK_ERR_INVALID_ARG; delete s; return STARK_OK; }   // layers and levels return to the pool (stream-ordered reuse)

int32_t stark_ali_merge_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* r_opt, const uint64_t* beta4,
                            const uint64_t* omega4, const uint64_t* z4, size_t n, uint64_t* f0, uint64_t* c_star4) {
    if (!ctx || !a || !s || !e || !t || !omega4 || !z4 || !f0 || (r_opt && !beta4)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    fr_t cs; STARK_TRY(ali_merge_dev_impl(ctx, as_fr(a), as_fr(s), as_fr(e), as_fr(t), as_fr(r_opt), beta4 ? load_fr(beta4) : host::h_zero(), load_fr(omega4), load_fr(z4), n, as_fr(f0), c_star4 ? &cs : nullptr));
    if (c_star4) store_fr(c_star4, cs); return STARK_OK;
}
int32_t stark_ali_merge(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* r_opt, const uint64_t* beta4,
                        const uint64_t* omega4, const uint64_t* z4, size_t n, uint64_t* f0, uint64_t* c_star4) {
    if (!ctx || !a || !s || !e || !t || !omega4 || !z4 || !f0 || (r_opt && !beta4)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    DevBuf d[6]; CallerUploads up(ctx); const uint64_t* src[5] = {a, s, e, t, r_opt};
    for (int i = 0; i < 5; ++i) if (src[i]) STARK_HIP(ctx, up.up(d[i], src[i], n * sizeof(fr_t)));
    STARK_HIP(ctx, d[5].alloc(ctx, n * sizeof(fr_t)));
    STARK_TRY(stark_ali_merge_dev(ctx, (const uint64_t*)d[0].p, (const uint64_t*)d[1].p, (const uint64_t*)d[2].p, (const uint64_t*)d[3].p, r_opt ? (const uint64_t*)d[4].p : nullptr, beta4, omega4, z4, n, (uint64_t*)d[5].p, c_star4));
    STARK_HIP(ctx, up.download_sync(f0, d[5].p, n * sizeof(fr_t))); return STARK_OK;
}
int32_t stark_build_f0_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, size_t n0, uint64_t* f0, uint64_t* aux7) {
    if (!ctx || !a || !s || !e || !t || !f0) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    fr_t aux[7]; STARK_TRY(build_f0_dev_impl(ctx, as_fr(a), as_fr(s), as_fr(e), as_fr(t), n0, as_fr(f0), aux7 ? aux : nullptr));
    if (aux7) for (int i = 0; i < 7; ++i) store_fr(aux7 + 4 * i, aux[i]); return STARK_OK;
}
int32_t stark_build_f0(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, size_t n0, uint64_t* f0, uint64_t* aux7) {
    if (!ctx || !a || !s || !e || !t || !f0) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    DevBuf d[5]; CallerUploads up(ctx); const uint64_t* src[4] = {a, s, e, t};
    for (int i = 0; i < 4; ++i) STARK_HIP(ctx, up.up(d[i], src[i], n0 * sizeof(fr_t)));
    STARK_HIP(ctx, d[4].alloc(ctx, n0 * sizeof(fr_t)));
    STARK_TRY(stark_build_f0_dev(ctx, (const uint64_t*)d[0].p, (const uint64_t*)d[1].p, (const uint64_t*)d[2].p, (const uint64_t*)d[3].p, n0, (uint64_t*)d[4].p, aux7));
    STARK_HIP(ctx, up.download_sync(f0, d[4].p, n0 * sizeof(fr_t))); return STARK_OK;
}

int32_t stark_deep_fri_prove_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* f0, size_t n0,
                                 const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out) {
    if (!ctx || !out || (!schedule && L) || (!f0 && (!a || !s || !e || !t))) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    stark_proof* P = nullptr; int32_t rc;                                     // a batch of one; *out is written on success only
    if (f0) {
        if (!is_pow2(n0)) return ctx->fail(STARK_ERR_INVALID_ARG, "n0 must be a power of two (radix-2 domain)");
        rc = prove_f0_batch_impl(ctx, 1, &f0, n0, schedule, L, r, seed_z, &P);
    } else rc = prove_batch_impl(ctx, 1, &a, &s, &e, &t, n0, schedule, L, r, seed_z, &P);
    if (rc == STARK_OK) *out = P;
    return rc;
}
int32_t stark_deep_fri_prove(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* f0, size_t n0,
                             const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out) {
    if (!ctx || !out || (!schedule && L) || (!f0 && (!a || !s || !e || !t))) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    DevBuf d[5]; CallerUploads up(ctx); const uint64_t* src[5] = {a, s, e, t, f0};
    for (int i = 0; i < 5; ++i) if ((i < 4 && !f0) || (i == 4 && f0)) STARK_HIP(ctx, up.up(d[i], src[i], n0 * sizeof(fr_t)));
    return stark_deep_fri_prove_dev(ctx, (const uint64_t*)d[0].p, (const uint64_t*)d[1].p, (const uint64_t*)d[2].p, (const uint64_t*)d[3].p, f0 ? (const uint64_t*)d[4].p : nullptr, n0, schedule, L, r, seed_z, out);
}
int32_t stark_deep_fri_prove_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* a, const uint64_t* const* s, const uint64_t* const* e, const uint64_t* const* t, size_t n0,
                                       const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out) {
    if (!ctx || !out || !batch || !a || !s || !e || !t || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    for (size_t p = 0; p < batch; ++p) if (!a[p] || !s[p] || !e[p] || !t[p]) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return prove_batch_impl(ctx, batch, a, s, e, t, n0, schedule, L, r, seed_z, out);
}
int32_t stark_deep_fri_prove_mixed_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* a, const uint64_t* const* s, const uint64_t* const* e, const uint64_t* const* t, const size_t* n0,
                                             const size_t* schedule, const size_t* sched_off, const size_t* r, uint64_t seed_z, stark_proof_t** out) {
    if (out) for (size_t p = 0; p < batch; ++p) out[p] = nullptr;
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!batch) return STARK_OK;
    if (!out || !a || !s || !e || !t || !n0 || !r || !sched_off) return STARK_ERR_INVALID_ARG;
    for (size_t p = 0; p < batch; ++p) if (!a[p] || !s[p] || !e[p] || !t[p]) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    for (size_t p = 0; p < batch; ++p) if (sched_off[p + 1] < sched_off[p]) return ctx->fail(STARK_ERR_INVALID_ARG, "sched_off must not decrease");
    if (!schedule && sched_off[batch] != sched_off[0]) return ctx->fail(STARK_ERR_INVALID_ARG, "null schedule with a fold");
    for (size_t p = 0; p < batch; ++p) {
        if (!is_pow2(n0[p]) || n0[p] <= 1) return ctx->fail(STARK_ERR_INVALID_ARG, "n0 must be a power of two above 1 (radix-2 domain), trace " + std::to_string(p));
        const size_t L = sched_off[p + 1] - sched_off[p]; std::vector<size_t> n, arity;
        STARK_TRY(layers_or_fail(ctx, n0[p], L ? schedule + sched_off[p] : nullptr, L, n, arity));
    }
    return prove_mixed_batch_impl(ctx, batch, a, s, e, t, n0, schedule, sched_off, r, seed_z, out);
}
int32_t stark_deep_fri_prove_f0_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* f0, size_t n0, const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out) {
    if (out) for (size_t p = 0; p < batch; ++p) out[p] = nullptr;
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!batch) return STARK_OK;
    if (!out || !f0 || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    for (size_t p = 0; p < batch; ++p) if (!f0[p]) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (!is_pow2(n0) || n0 <= 1) return ctx->fail(STARK_ERR_INVALID_ARG, "n0 must be a power of two above 1 (radix-2 domain)");
    { std::vector<size_t> n, arity; STARK_TRY(layers_or_fail(ctx, n0, schedule, L, n, arity)); }
    return prove_f0_batch_impl(ctx, batch, f0, n0, schedule, L, r, seed_z, out);
}
int32_t stark_fri_commit_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* f0, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, uint64_t* roots) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!batch) return STARK_OK;
    if (!roots || !f0 || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    for (size_t p = 0; p < batch; ++p) if (!f0[p]) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    { std::vector<size_t> n, arity; STARK_TRY(layers_or_fail(ctx, n0, schedule, L, n, arity)); }
    return commit_batch_impl(ctx, batch, f0, n0, schedule, L, seed_z, roots);
}
int32_t stark_ali_merge_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* a, const uint64_t* const* s, const uint64_t* const* e, const uint64_t* const* t,
                                  const uint64_t* const* r_opt, const uint64_t* beta, const uint64_t* omega4, const uint64_t* z, size_t n, uint64_t* const* f0, uint64_t* c_star) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!batch) return STARK_OK;
    if (!a || !s || !e || !t || !omega4 || !z || !f0 || (r_opt && !beta)) return STARK_ERR_INVALID_ARG;
    for (size_t p = 0; p < batch; ++p) if (!a[p] || !s[p] || !e[p] || !t[p] || !f0[p]) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (n <= 1) return ctx->fail(STARK_ERR_INVALID_ARG, "n > 1");                                                                                       // lib.rs:71
    for (size_t p = 0; p < batch; ++p) if (fr_eq(fr_pow_u64<PallasFr>(load_fr(z + 4 * p), n), host::h_one())) return ctx->fail(STARK_ERR_INVALID_ARG, "z must be outside H");   // lib.rs:78
    return ali_merge_batch_impl(ctx, batch, a, s, e, t, r_opt, beta, load_fr(omega4), z, n, f0, c_star);
}
// lagrange_eval_on_h (deep_ali/src/lib.rs:17-45) of ncols DEVICE columns at npoints HOST points: ONE driver (lagrange_dev.hpp) for the batch, the
// single device form (1 x 1) and the host-pointer form (upload, 1 x 1, download); stream-ordered, z and the pointer table are copied before return.
int32_t stark_lagrange_eval_on_h_batch_dev(stark_ctx_t* ctx, size_t ncols, const uint64_t* const* cols, size_t n, const uint64_t* omega4, size_t npoints, const uint64_t* z, uint64_t* out) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!ncols || !npoints) return STARK_OK;
    fr_t omega; STARK_TRY(lagrange_check_args(ctx, ncols, cols, n, n, omega4, npoints, z, out, npoints * ncols, &omega));
    STARK_TRY(ctx_enter(ctx));
    return lagrange_eval_block_impl(ctx, ncols, cols, lag_whole(n), omega, lagrange_points(npoints, z), as_fr(out));
}
int32_t stark_lagrange_eval_on_h_dev(stark_ctx_t* ctx, const uint64_t* values, size_t n, const uint64_t* z4, const uint64_t* omega4, uint64_t* out4) {
    return stark_lagrange_eval_on_h_batch_dev(ctx, 1, &values, n, omega4, 1, z4, out4);
}
int32_t stark_lagrange_eval_on_h(stark_ctx_t* ctx, const uint64_t* values, size_t n, const uint64_t* z4, const uint64_t* omega4, uint64_t* out4) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!values || !z4 || !out4) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: null values, z or out");
    if (!is_pow2(n) || n > ((size_t)1 << kLagMaxLogN)) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: n must be a power of two, 1 <= n <= 2^30");
    STARK_TRY(ctx_enter(ctx));
    DevBuf d, o; CallerUploads up(ctx); STARK_HIP(ctx, up.up(d, values, n * sizeof(fr_t))); STARK_HIP(ctx, o.alloc(ctx, sizeof(fr_t)));
    STARK_TRY(stark_lagrange_eval_on_h_dev(ctx, (const uint64_t*)d.p, n, z4, omega4, (uint64_t*)o.p));
    STARK_HIP(ctx, up.download_sync(out4, o.p, sizeof(fr_t))); return STARK_OK;
}
// The block form (lagrange_dev.hpp): the unscaled share of the rows [j0, j0 + n_local) of an n_global-point domain, and the combine of such shares.
int32_t stark_lagrange_eval_shard_dev(stark_ctx_t* ctx, size_t ncols, const uint64_t* const* cols, size_t n_local, uint64_t j0, size_t n_global, const uint64_t* omega4, size_t npoints,
                                      const uint64_t* z, uint64_t* partials_out) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!ncols || !npoints) return STARK_OK;
    if (!n_local) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: n_local must be at least 1");
    if (j0 > n_global || n_local > n_global - j0) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: j0 + n_local exceeds n_global");
    fr_t omega; STARK_TRY(lagrange_check_args(ctx, ncols, cols, n_local, n_global, omega4, npoints, z, partials_out, npoints * ncols, &omega));
    STARK_TRY(ctx_enter(ctx));
    return lagrange_eval_block_impl(ctx, ncols, cols, LagBlock{n_local, j0, n_global, false}, omega, lagrange_points(npoints, z), as_fr(partials_out));
}
int32_t stark_lagrange_eval_from_partials_dev(stark_ctx_t* ctx, size_t nparts, const uint64_t* partials, size_t ncols, size_t n_global, const uint64_t* omega4, size_t npoints, const uint64_t* z,
                                              uint64_t* out) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!ncols || !npoints) return STARK_OK;
    if (!nparts) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: nparts must be at least 1");
    if (!partials) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: null partials");
    if (!out) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: null out");
    if (!z) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: null z with npoints > 0");
    fr_t omega; STARK_TRY(lagrange_check_domain(ctx, n_global, omega4, &omega));
    if (ncols > kLagMaxCols || npoints > ((size_t)1 << 36) / ncols || nparts > ((size_t)1 << 20)) return ctx->fail(STARK_ERR_UNSUPPORTED, "lagrange_eval: more than 2^24 columns, 2^36 results or 2^20 parts in one call");
    const uintptr_t o0 = (uintptr_t)out, obytes = npoints * ncols * sizeof(fr_t), p0 = (uintptr_t)partials;
    if (p0 < o0 + obytes && o0 < p0 + nparts * obytes) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval: out overlaps partials");
    STARK_TRY(ctx_enter(ctx));
    const std::vector<fr_t> zs = lagrange_points(npoints, z);
    LagDevExec X(ctx);
    return lagrange_combine(X, nparts, as_fr(partials), ncols, n_global, npoints, zs.data(), as_fr(out));
}
// Collective: the sharded call.  Every check of this rank's arguments comes before the first collective (lagrange_sharded).
int32_t stark_lagrange_eval_on_h_sharded_dev(stark_ctx_t* ctx, size_t ncols, const uint64_t* const* cols_block, size_t n_global, const uint64_t* omega4, size_t npoints, const uint64_t* z,
                                             uint64_t* out) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!ncols || !npoints) return STARK_OK;
    const ShardColl C = ShardColl::real(ctx); const size_t W = (size_t)std::max(C.W, 1);
    if (C.W < 1 || (W & (W - 1)) || !n_global || n_global % W) return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval sharded: the communicator's size must be a power of two that divides n_global");
    fr_t omega; STARK_TRY(lagrange_check_args(ctx, ncols, cols_block, n_global / W, n_global, omega4, npoints, z, out, npoints * ncols, &omega));
    STARK_TRY(ctx_enter(ctx));
    return lagrange_sharded(C, ncols, cols_block, n_global, omega, lagrange_points(npoints, z), as_fr(out));
}
int32_t stark_diag_lagrange_eval_sharded_emulated_dev(stark_ctx_t* ctx, int32_t nranks, size_t ncols, const uint64_t* const* cols_whole, size_t n_global, const uint64_t* omega4, size_t npoints,
                                                      const uint64_t* z, uint64_t* out) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!ncols || !npoints) return STARK_OK;
    if (nranks < 1 || (nranks & (nranks - 1)) || !n_global || (size_t)nranks > n_global || n_global % (size_t)nranks)
        return ctx->fail(STARK_ERR_INVALID_ARG, "lagrange_eval sharded: nranks must be a power of two that divides n_global");
    if (npoints > ((size_t)1 << 36) / ncols / (size_t)nranks) return ctx->fail(STARK_ERR_UNSUPPORTED, "lagrange_eval: more than 2^36 results in one call");
    fr_t omega; STARK_TRY(lagrange_check_args(ctx, ncols, cols_whole, n_global, n_global, omega4, npoints, z, out, (size_t)nranks * npoints * ncols, &omega));
    STARK_TRY(ctx_enter(ctx));
    return lagrange_sharded(ShardColl::emulate(ctx, nranks), ncols, cols_whole, n_global, omega, lagrange_points(npoints, z), as_fr(out));
}
size_t stark_proof_len(stark_proof_t* p) { return p ? p->bytes.size() : 0; }
int32_t stark_proof_bytes(stark_proof_t* p, uint8_t* out) { if (!p || !out) return STARK_ERR_INVALID_ARG; memcpy(out, p->bytes.data(), p->bytes.size()); return STARK_OK; }
size_t stark_proof_size_estimate(stark_proof_t* p) { return p ? p->size_estimate : 0; }
double stark_proof_stage_ms(stark_proof_t* p, int32_t stage) { return (p && stage >= 0 && stage < 3) ? p->ms[stage] : -1.0; }
int32_t stark_proof_free(stark_proof_t* p) { if (!p) return STARK_ERR_INVALID_ARG; delete p; return STARK_OK; }

// ---- one trace sharded over several GPUs: the pieces the orchestrator (stark_mlwe_amd/dist.py) composes --------
int32_t stark_ali_merge_shard_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* r_opt, const uint64_t* beta4,
                                  const uint64_t* omega4, const uint64_t* z4, size_t n_local, uint64_t j0, size_t n_global, uint64_t* f0, uint64_t* partial4) {
    if (!ctx || !a || !s || !e || !t || !z4 || !f0 || (r_opt && !beta4) || !n_global) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const fr_t omega = omega4 ? load_fr(omega4) : fr_root_of_unity<PallasFr>((unsigned)ilog2(n_global));               // FriDomain::new_radix2(n).omega, fri.rs:53-56
    fr_t ps; STARK_TRY(ali_merge_dev_impl(ctx, as_fr(a), as_fr(s), as_fr(e), as_fr(t), as_fr(r_opt), beta4 ? load_fr(beta4) : host::h_zero(), omega, load_fr(z4), n_local, as_fr(f0),
                                          partial4 ? &ps : nullptr, j0, n_global, true));
    if (partial4) store_fr(partial4, ps); return STARK_OK;
}
int32_t stark_ali_cstar_from_partials(stark_ctx_t* ctx, const uint64_t* partials, size_t k, size_t n_global, uint64_t* c_star4) {
    if (!ctx || (!partials && k) || !c_star4 || !n_global) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    fr_t acc = host::h_zero(); for (size_t i = 0; i < k; ++i) acc = host::h_add(acc, load_fr(partials + 4 * i));
    store_fr(c_star4, fr_mul<PallasFr>(acc, fr_inv<PallasFr>(host::h_u64(n_global)))); return STARK_OK;                  // c* = (1/n) * sum (lib.rs:44, :94)
}
int32_t stark_ali_challenges(stark_ctx_t* ctx, const uint64_t* digests16, size_t n0, uint64_t* aux12) {
    if (!ctx || !digests16 || !aux12 || n0 <= 1) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    fr_t h[4]; for (int c = 0; c < 4; ++c) h[c] = load_fr(digests16 + 4 * c);
    fr_t seed_f, z, beta; STARK_TRY(ali_challenges(ctx, h, n0, &seed_f, &z, &beta));
    store_fr(aux12, seed_f); store_fr(aux12 + 4, z); store_fr(aux12 + 8, beta); return STARK_OK;
}
int32_t stark_fri_plan_create(stark_ctx_t* ctx, const uint64_t* roots, size_t n0, const size_t* schedule, size_t L, size_t r, stark_fri_plan_t** out) {
    if (!ctx || !roots || !out || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    std::vector<fr_t> rt(L + 1); for (size_t l = 0; l <= L; ++l) rt[l] = load_fr(roots + 4 * l);
    std::unique_ptr<stark_fri_plan> P(new stark_fri_plan()); P->ref_.bind(ctx); P->ctx = ctx;
    DeviceHasher H(ctx); STARK_TRY(make_query_plan(ctx, P->plan, n0, schedule, L, rt.data(), r, H, "query plan"));
    *out = P.release(); return STARK_OK;
}
size_t stark_fri_plan_num_requests(stark_fri_plan_t* p) { return p ? p->plan.req.size() : 0; }
int32_t stark_fri_plan_requests(stark_fri_plan_t* p, uint32_t* kind, uint32_t* which, uint32_t* level, uint64_t* index) {
    if (!p || !kind || !which || !level || !index) return STARK_ERR_INVALID_ARG;
    for (size_t i = 0; i < p->plan.req.size(); ++i) { kind[i] = p->plan.req[i].kind; which[i] = p->plan.req[i].which; level[i] = p->plan.req[i].level; index[i] = p->plan.req[i].index; }
    return STARK_OK;
}
int32_t stark_fri_plan_assemble(stark_fri_plan_t* p, const uint64_t* values, size_t n_values, stark_proof_t** out) {
    if (!p || (!values && n_values) || !out) return STARK_ERR_INVALID_ARG;
    stark_ctx* ctx = p->ctx;
    if (n_values != p->plan.req.size()) return ctx->fail(STARK_ERR_INVALID_ARG, "value count differs from the plan's request count");
    std::vector<fr_t> v(n_values); for (size_t i = 0; i < n_values; ++i) v[i] = load_fr(values + 4 * i);
    DeviceHasher H(ctx); std::unique_ptr<stark_proof> P(new stark_proof());
    STARK_TRY(assemble_from_values(ctx, p->plan.shape, p->plan.r, H, v.data(), v.size(), P.get(), "assemble: values do not match the plan"));
    *out = P.release(); return STARK_OK;
}
int32_t stark_fri_plan_free(stark_fri_plan_t* p) { if (!p) return STARK_ERR_INVALID_ARG; delete p; return STARK_OK; }

}  // extern "C"

#include "fri_shard_impl.hpp"
