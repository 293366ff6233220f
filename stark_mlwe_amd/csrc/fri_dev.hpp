// stark_mlwe_amd/csrc/fri_dev.hpp — streaming kernels of the FRI path on CDNA4 (gfx950).
//
//   k_fri_fold   fri_fold_layer            crates/deep_ali/src/fri.rs:85-102   out[b] = sum_t f[b*m+t] z^t
//                (compute_s_layer, fri.rs:123-143, is the view s[i] = out[i/m]; never materialised)
//   k_ali_*      deep_ali_merge_evals(_blinded)   crates/deep_ali/src/lib.rs:60-105
//   k_gather_rows  every read of a Merkle opening or a query phase (merkle/src/lib.rs:261-291; fri.rs:355-466) in one launch
//   k_synth      synthetic trace columns for benchmarks (definition in DESIGN.md "Synthetic inputs")
// All HBM-streaming: every lane moves whole 32-byte elements as 2 x dwordx4, consecutive lanes touch
// consecutive elements.
#pragma once
#include <hip/hip_runtime.h>
#include "fr.hpp"
#include "dev_common.hpp"
#include "ntt_dev.hpp"   // PowTable / pow_lookup
#include "poseidon_streams.hpp"   // DsRaggedStream: the segment table of k_copy_ragged
#include "fri_mixed.hpp"          // FoldSeg, ZpowJob: the tables of k_fri_fold_ragged and k_zpows_many

namespace stark {

// Fold with m a power of two.  G = min(m,16) adjacent lanes cooperate on one output: each lane owns
// m/G consecutive inputs (Horner over its run, scaled by z^(lane_run_start)), then a butterfly sum.
// zp[t] = z^t for t < m (uniform table in global memory).
template <class F>
__global__ void __launch_bounds__(256) k_fri_fold_pow2(const fr_t* __restrict__ f, uint64_t n, const fr_t* __restrict__ zp, int log_m, int log_g, fr_t* __restrict__ out) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int per = 1 << (log_m - log_g);                 // inputs per lane
    const uint64_t first = tid << (log_m - log_g);        // index of this lane's first input
    const bool live = first < n;
    fr_t acc = fr_zero<F>();
    if (live) {
        const uint32_t t0 = (uint32_t)(first & ((1ull << log_m) - 1));
        // sum_{u<per} f[first+u] * z^(t0+u)
        for (int u = 0; u < per; ++u) acc = fr_add<F>(acc, fr_mul<F>(ldg(f + first + u), zp[t0 + u]));
    }
    for (int s = 0; s < log_g; ++s) acc = fr_add<F>(acc, shfl_xor_fr(acc, 1 << s));
    if (live && (tid & ((1u << log_g) - 1)) == 0) stg(out + (first >> log_m), acc);
}
// The fold of layers of DIFFERENT lengths that share m, back to back (the ragged commit phase, fri_mixed.hpp): k_fri_fold_pow2 with the power table
// looked up per output.  segs: runs of outputs under one challenge, (first_out, zp_off), first_out ascending from 0; output j folds under
// zp[zp_off_s ..] for the last run s with first_out_s <= j.  A run holds whole outputs, so the G lanes of an output share the run; the lanes of a
// wave need not.  Lanes past n take part in the butterfly with zero and store nothing.  (FoldSeg, fold_seg_of: fri_mixed.hpp.)
template <class F>
__global__ void __launch_bounds__(256) k_fri_fold_ragged(const fr_t* __restrict__ f, uint64_t n, const FoldSeg* __restrict__ segs, uint32_t n_seg, const fr_t* __restrict__ zp_all, int log_m, int log_g,
                                                         fr_t* __restrict__ out) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int per = 1 << (log_m - log_g);
    const uint64_t first = tid << (log_m - log_g);
    const bool live = first < n;
    fr_t acc = fr_zero<F>();
    if (live) {
        const fr_t* zp = zp_all + segs[fold_seg_of(segs, n_seg, first >> log_m)].zp_off;
        const uint32_t t0 = (uint32_t)(first & ((1ull << log_m) - 1));
        for (int u = 0; u < per; ++u) acc = fr_add<F>(acc, fr_mul<F>(ldg(f + first + u), ldg(zp + t0 + u)));
    }
    for (int s = 0; s < log_g; ++s) acc = fr_add<F>(acc, shfl_xor_fr(acc, 1 << s));
    if (live && (tid & ((1u << log_g) - 1)) == 0) stg(out + (first >> log_m), acc);
}
// The z^t tables of a whole pass in one launch: job s = blockIdx.y (ZpowJob, fri_mixed.hpp) fills zp[off_s + t] = z_s^t, t < m_s (gridDim.x covers the largest m).
template <class F>
__global__ void __launch_bounds__(64) k_zpows_many(const ZpowJob* __restrict__ job, fr_t* __restrict__ zp) {
    const ZpowJob* J = job + blockIdx.y;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= J->m) return;
    fr_t acc = fr_one<F>(), b = ldg(&J->z);
    for (uint64_t e = t; e; e >>= 1) { if (e & 1) acc = fr_mul<F>(acc, b); b = fr_sqr<F>(b); }
    stg(zp + J->off + t, acc);
}
// zp[t] = z^t, t < m (square-and-multiply per lane; m is a fold arity, at most a few hundred).
template <class F>
__global__ void __launch_bounds__(64) k_zpows(fr_t z, uint64_t m, fr_t* __restrict__ zp) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    fr_t acc = fr_one<F>(), b = z;
    for (uint64_t e = t; e; e >>= 1) { if (e & 1) acc = fr_mul<F>(acc, b); b = fr_sqr<F>(b); }
    stg(zp + t, acc);
}
// General m (>= 2, any): one lane per output.
template <class F>
__global__ void __launch_bounds__(256) k_fri_fold_any(const fr_t* __restrict__ f, uint64_t n_out, const fr_t* __restrict__ zp, uint64_t m, fr_t* __restrict__ out) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_out) return;
    fr_t acc = fr_zero<F>();
    for (uint64_t t = 0; t < m; ++t) acc = fr_add<F>(acc, fr_mul<F>(ldg(f + b * m + t), zp[t]));
    stg(out + b, acc);
}

// DEEP-ALI merge.  phi_j = a_j s_j + e_j - t_j (+ beta r_j);  f0_j = phi_j / (w^j - z).
// Each lane owns K elements j = tid + u*T (T = total lanes) so loads stay coalesced; ALL 256*K denominators of a
// workgroup are inverted with ONE Fermat inversion (Montgomery's trick, two levels: prefix products per lane, product
// scans across the lanes), as lib.rs's 2n inversions are n independent field inverses whose values do not depend
// on how they are obtained.
// Also accumulates the barycentric partial sum  sum_j phi_j w^j / (z - w^j)  per block (for c*).
#define ALI_K 8
// The work of one workgroup (blockIdx.x) on one trace: k_ali_merge runs it for its only trace, k_ali_merge_batch and k_ali_merge_ragged for trace blockIdx.y.
// block_sum: where this workgroup's barycentric partial goes (nullptr: c* is not asked for).  T: the lanes that work on this trace (its workgroups x
// blockDim.x; the grid's own where every trace has the grid's length).  stride: the power table is that of a generator g with w = g^stride (1: the
// table is w's own).
template <class F>
__device__ __forceinline__ void ali_merge_block(const fr_t* __restrict__ a, const fr_t* __restrict__ s, const fr_t* __restrict__ e, const fr_t* __restrict__ t,
                                                const fr_t* __restrict__ r_opt, const fr_t& beta, const PowTable& wpow, const fr_t& w_step /* w^T */, const fr_t& w_step_inv, const fr_t& z, uint64_t n,
                                                uint64_t j0 /* global position of element 0 */, fr_t* __restrict__ f0, fr_t* __restrict__ block_sum,
                                                uint64_t T /* the lanes of THIS trace's merge */, uint64_t stride /* w = wpow's generator ^ stride */) {
    __shared__ uint4 red[2 * 4];
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    fr_t phi[ALI_K], pre[ALI_K];
    fr_t w = tid < n ? pow_lookup<F>(wpow, (j0 + tid) * stride) : fr_one<F>();     // w^(j0 + tid)
    fr_t run = fr_one<F>();
#pragma unroll
    for (int u = 0; u < ALI_K; ++u) {                              // forward: phi_j and prefix products of (w^j - z)
        const uint64_t j = tid + (uint64_t)u * T;
        fr_t d = fr_one<F>(); phi[u] = fr_zero<F>();
        if (j < n) {
            fr_t p = fr_sub<F>(fr_add<F>(fr_mul<F>(ldg(a + j), ldg(s + j)), ldg(e + j)), ldg(t + j));
            if (r_opt) p = fr_add<F>(p, fr_mul<F>(beta, ldg(r_opt + j)));
            phi[u] = p; d = fr_sub<F>(w, z);
        }
        pre[u] = run; run = fr_mul<F>(run, d);
        w = fr_mul<F>(w, w_step);
    }
    // ONE Fermat inversion per WORKGROUP (it is ~380 products; per lane it would dwarf the ~9 products an element needs):
    // wave-level inclusive prefix / suffix products of the lanes' `run` (shuffles), the four wave totals through LDS, wave 0 inverts
    // their product, and every lane recovers  1/run = (1/P) * (other waves' totals) * (lanes before) * (lanes after).
    __shared__ uint4 tot[2 * 4], pinv[2];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, nwv = (int)(blockDim.x >> 6);
    fr_t pre_i = run, suf_i = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const fr_t a = shfl_up_fr(pre_i, d), b = shfl_dn_fr(suf_i, d);
        if (ln >= d) pre_i = fr_mul<F>(pre_i, a);
        if (ln + d < 64) suf_i = fr_mul<F>(suf_i, b);
    }
    fr_t before = shfl_up_fr(pre_i, 1), after = shfl_dn_fr(suf_i, 1);
    if (ln == 0) before = fr_one<F>();
    if (ln == 63) after = fr_one<F>();
    if (ln == 63) { tot[2 * wv] = make_uint4(pre_i.v[0], pre_i.v[1], pre_i.v[2], pre_i.v[3]); tot[2 * wv + 1] = make_uint4(pre_i.v[4], pre_i.v[5], pre_i.v[6], pre_i.v[7]); }
    __syncthreads();
    auto ld_tot = [&](const uint4* p, int i) { const uint4 lo = p[2 * i], hi = p[2 * i + 1]; fr_t x; x.v[0] = lo.x; x.v[1] = lo.y; x.v[2] = lo.z; x.v[3] = lo.w; x.v[4] = hi.x; x.v[5] = hi.y; x.v[6] = hi.z; x.v[7] = hi.w; return x; };
    if (wv == 0) {
        fr_t P = ld_tot(tot, 0); for (int i = 1; i < nwv; ++i) P = fr_mul<F>(P, ld_tot(tot, i));
        const fr_t Pi = fr_inv<F>(P);
        if (ln == 0) { pinv[0] = make_uint4(Pi.v[0], Pi.v[1], Pi.v[2], Pi.v[3]); pinv[1] = make_uint4(Pi.v[4], Pi.v[5], Pi.v[6], Pi.v[7]); }
    }
    __syncthreads();
    fr_t inv = ld_tot(pinv, 0);
    for (int i = 0; i < nwv; ++i) if (i != wv) inv = fr_mul<F>(inv, ld_tot(tot, i));                       // 1 / (this wave's total)
    inv = fr_mul<F>(fr_mul<F>(inv, before), after);                                                       // 1 / run of this lane
    fr_t bary = fr_zero<F>();
#pragma unroll
    for (int u = ALI_K - 1; u >= 0; --u) {                         // backward: peel the inverses off
        const uint64_t j = tid + (uint64_t)u * T;
        w = fr_mul<F>(w, w_step_inv);                              // back to w^j
        if (j < n) {
            fr_t dinv = fr_mul<F>(inv, pre[u]);                    // 1 / (w^j - z)
            inv = fr_mul<F>(inv, fr_sub<F>(w, z));
            fr_t q = fr_mul<F>(phi[u], dinv);
            stg(f0 + j, q);
            if (block_sum) bary = fr_sub<F>(bary, fr_mul<F>(q, w));   // phi w^j / (z - w^j) = -(phi / (w^j - z)) w^j  (only when c* is asked for)
        }
    }
    if (block_sum) {
        for (int sft = 1; sft < 64; sft <<= 1) bary = fr_add<F>(bary, shfl_xor_fr(bary, sft));
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0) { red[2 * wave] = make_uint4(bary.v[0], bary.v[1], bary.v[2], bary.v[3]); red[2 * wave + 1] = make_uint4(bary.v[4], bary.v[5], bary.v[6], bary.v[7]); }
        __syncthreads();
        if (threadIdx.x == 0) {
            fr_t acc = fr_zero<F>();
            for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) {
                uint4 lo = red[2 * wv], hi = red[2 * wv + 1]; fr_t x;
                x.v[0] = lo.x; x.v[1] = lo.y; x.v[2] = lo.z; x.v[3] = lo.w; x.v[4] = hi.x; x.v[5] = hi.y; x.v[6] = hi.z; x.v[7] = hi.w;
                acc = fr_add<F>(acc, x);
            }
            stg(block_sum, acc);
        }
    }
}
template <class F>
__global__ void __launch_bounds__(256) k_ali_merge(const fr_t* __restrict__ a, const fr_t* __restrict__ s, const fr_t* __restrict__ e, const fr_t* __restrict__ t,
                                                   const fr_t* __restrict__ r_opt, fr_t beta, PowTable wpow, fr_t w_step /* w^T */, fr_t w_step_inv, fr_t z, uint64_t n, uint64_t j0 /* global position of element 0 */,
                                                   fr_t* __restrict__ f0, fr_t* __restrict__ block_sums) {
    ali_merge_block<F>(a, s, e, t, r_opt, beta, wpow, w_step, w_step_inv, z, n, j0, f0, block_sums ? block_sums + blockIdx.x : (fr_t*)nullptr, (uint64_t)gridDim.x * blockDim.x, 1);
}
// The merges of gridDim.y traces of n elements over one domain in ONE launch: trace b = blockIdx.y reads its columns through the pointer tables
// (r_opt == nullptr, or r_opt[b] == nullptr: no blinding term for that trace), its own z[b] and beta[b] from device arrays, and writes
// out_base + b * n (a trace-major layer-0 buffer) or, with out_base == nullptr, out_ptrs[b].  block_sums: gridDim.x partials per trace.
template <class F>
__global__ void __launch_bounds__(256) k_ali_merge_batch(const fr_t* const* __restrict__ a, const fr_t* const* __restrict__ s, const fr_t* const* __restrict__ e, const fr_t* const* __restrict__ t,
                                                         const fr_t* const* __restrict__ r_opt, const fr_t* __restrict__ beta, PowTable wpow, fr_t w_step, fr_t w_step_inv, const fr_t* __restrict__ z,
                                                         uint64_t n, fr_t* __restrict__ out_base, fr_t* const* __restrict__ out_ptrs, fr_t* __restrict__ block_sums) {
    const uint64_t b = blockIdx.y;
    const fr_t* r = r_opt ? r_opt[b] : (const fr_t*)nullptr;
    const fr_t bt = r ? ldg(beta + b) : fr_zero<F>();
    ali_merge_block<F>(a[b], s[b], e[b], t[b], r, bt, wpow, w_step, w_step_inv, ldg(z + b), n, 0, out_base ? out_base + b * n : out_ptrs[b],
                       block_sums ? block_sums + b * gridDim.x + blockIdx.x : (fr_t*)nullptr, (uint64_t)gridDim.x * blockDim.x, 1);
}
// The merges of gridDim.y traces of DIFFERENT lengths in ONE launch (the ragged prove tail, fri_mixed.hpp): trace b = blockIdx.y is job[b] — its
// columns, its own n, z, w_step = w_b^T_b and inverse (T_b = its own workgroups x blockDim.x) — and writes f0 + out_off (layer 0 of the pass, the
// traces back to back).  wpow is the table of the LARGEST domain's generator g; trace b's generator is g^stride, stride = n_max / n_b.  gridDim.x is
// sized for the largest trace: a workgroup beyond trace b's own count leaves before any barrier.  No c*.
struct AliRaggedJob { const fr_t *a, *s, *e, *t; fr_t z, w_step, w_step_inv; uint64_t n, out_off, stride; };
template <class F>
__global__ void __launch_bounds__(256) k_ali_merge_ragged(const AliRaggedJob* __restrict__ job, PowTable wpow, fr_t* __restrict__ f0) {
    const AliRaggedJob* J = job + blockIdx.y;
    const uint64_t n = J->n, lanes = (n + ALI_K - 1) / ALI_K, blocks = (lanes + blockDim.x - 1) / blockDim.x;
    if (blockIdx.x >= blocks) return;                              // the whole workgroup: nothing of it reaches a barrier
    ali_merge_block<F>(J->a, J->s, J->e, J->t, nullptr, fr_zero<F>(), wpow, ldg(&J->w_step), ldg(&J->w_step_inv), ldg(&J->z), n, 0, f0 + J->out_off, nullptr, blocks * blockDim.x, J->stride);
}
// dst[b * n + i] = src[b][i] for b = blockIdx.y: layer 0 of a batch from a table of per-trace pointers (one launch instead of one copy per trace).
static __global__ void __launch_bounds__(256) k_copy_rows(const fr_t* const* __restrict__ src, uint64_t n, fr_t* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i < n) stg(dst + b * n + i, ldg(src[b] + i));
}
// dst[first_s + j] = in0_s[j], j < n_in_s, for every segment s of a pair-leaf table (DsRaggedStream mode 1: `first` counts elements): level 0 of a
// batch of plain trees of different lengths, back to back, in one launch.
static __global__ void __launch_bounds__(256) k_copy_ragged(DsRaggedStream D, fr_t* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D.n_out) return;
    const DsRaggedStream::Seg& S = D.segs[D.seg(i)];
    stg(dst + i, ldg(S.in0 + (i - S.first)));
}
// out[b] = scale * sum_{i<n} v[b * n + i] for b = blockIdx.x   (one 256-thread block per sum; n is a few thousand block partials; a grid of one
// block is the single sum).
template <class F>
__global__ void __launch_bounds__(256) k_sum_single_block(const fr_t* __restrict__ v, uint64_t n, fr_t scale, fr_t* __restrict__ out) {
    __shared__ uint4 red[2 * 4];
    v += (uint64_t)blockIdx.x * n; out += blockIdx.x;
    fr_t acc = fr_zero<F>();
    for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) acc = fr_add<F>(acc, ldg(v + i));
    for (int sft = 1; sft < 64; sft <<= 1) acc = fr_add<F>(acc, shfl_xor_fr(acc, sft));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { red[2 * wave] = make_uint4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]); red[2 * wave + 1] = make_uint4(acc.v[4], acc.v[5], acc.v[6], acc.v[7]); }
    __syncthreads();
    if (threadIdx.x == 0) {
        fr_t tot = fr_zero<F>();
        for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) {
            uint4 lo = red[2 * wv], hi = red[2 * wv + 1]; fr_t x;
            x.v[0] = lo.x; x.v[1] = lo.y; x.v[2] = lo.z; x.v[3] = lo.w; x.v[4] = hi.x; x.v[5] = hi.y; x.v[6] = hi.z; x.v[7] = hi.w;
            tot = fr_add<F>(tot, x);
        }
        stg(out, fr_mul<F>(tot, scale));
    }
}

// THE gather of the library (host side: MerkleGatherList, gather_rows): request i reads element index[i] of the array base[src[i]] (a layer or a
// tree level) into row[i] of the table (layers and tree levels of whole proofs and openings in ONE launch instead of one synchronised gather per level).  A sharded
// prove writes only the rows its rank owns into a zeroed table, so that one all-reduce SUM completes it.  Bounds are checked on the host.
static __global__ void k_gather_rows(const fr_t* const* __restrict__ base, const uint32_t* __restrict__ src, const uint64_t* __restrict__ index,
                                     const uint64_t* __restrict__ row, uint64_t k, fr_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) stg(out + row[i], ldg(base[src[i]] + index[i]));
}
// dst[i] += src[i] on uint64 words (wrapping): the SUM of an all-reduce when several ranks are emulated on one GPU.
static __global__ void k_add_u64(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}
// dst[a][b][c] (contiguous, dims Da x Db x Dc) = src[a*sa + b*sb + c*sc]: the layout changes around the all-to-all exchanges
// of the six-step NTT (32-byte elements, so even the transposing cases move whole 32-B units).
static __global__ void k_permute3(const fr_t* __restrict__ src, fr_t* __restrict__ dst, uint64_t Da, uint64_t Db, uint64_t Dc, uint64_t sa, uint64_t sb, uint64_t sc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Da * Db * Dc) return;
    const uint64_t c = i % Dc, b = (i / Dc) % Db, a = i / (Dc * Db);
    stg(dst + i, ldg(src + a * sa + b * sb + c * sc));
}
// dst[k * stride + offset] = src[k]: interleaves the `stride` coset transforms of an LDE into natural order.
static __global__ void k_interleave(const fr_t* __restrict__ src, fr_t* __restrict__ dst, uint64_t n, uint64_t stride, uint64_t offset) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) stg(dst + k * stride + offset, ldg(src + k));
}

// Synthetic column: limb j of element i = mix64(seed + (col << 56) + 4*i + j), top limb masked to 62
// bits; the limbs are the stored (Montgomery) representation.  (DESIGN.md "Synthetic inputs".)
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull; return x ^ (x >> 31);
}
static __global__ void k_synth(uint64_t seed, uint64_t col, uint64_t i0, uint64_t n, fr_t* __restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fr_t x;
#pragma unroll
    for (int j = 0; j < 4; ++j) { uint64_t v = mix64(seed + (col << 56) + 4 * (i0 + i) + j); if (j == 3) v &= 0x3FFFFFFFFFFFFFFFull; x.v[2 * j] = (uint32_t)v; x.v[2 * j + 1] = (uint32_t)(v >> 32); }
    stg(out + i, x);
}

}  // namespace stark
