// stark_mlwe_amd/csrc/lagrange_dev.hpp — lagrange_eval_on_h (deep_ali/src/lib.rs:17-45) of many columns at many points on CDNA4 (gfx950).
//
//   outside H (z^n != 1):  f(z) = (z^n - 1)/n * sum_j v[j] w^j / (z - w^j)          inside H (z = w^j):  f(z) = v[j], copied
//
// The weights W_j(z) = w^j / (z - w^j) depend on the point only, so C columns at one point cost one batch inversion and C dot products.
// The host classifies the points (z is a host array): z^n, the scale (z^n - 1)/n, and for a point inside H its index by the 2-adic discrete
// logarithm (one bit of j per step, no device search).  Points inside H are one k_lagrange_gather launch; the others go, as a compacted list
// cut into passes that bound the scratch, through
//   k_lagrange_partials   grid (tiles of the domain, point groups): a 256-thread workgroup owns the 256 K positions j = tid + u T (tid counted
//                         over the grid's x dimension, T its lanes: every column load of a wave is 64 consecutive elements) and walks the
//                         points of its group: the K weights of a lane from ONE Fermat inversion per
//                         workgroup (the two-level scheme of ali_merge_block, fri_dev.hpp), then per column K products, a wave reduction by
//                         shuffles and the four waves through LDS: one partial per (point, column, workgroup);
//   k_lagrange_finish     one block per (point, column): the sum of its partials times the point's scale -> out[p * ncols + c].
// The driver (lagrange_eval_batch) and the per-lane pieces are host code / FR_HD: hostcheck.cpp runs the same driver with every workgroup in
// lockstep on the CPU (hc_lagrange_eval_batch).  Every stored value is fully reduced, so neither the order of a sum nor how an inverse is
// obtained changes a bit.
//
// BLOCK FORM (LagBlock): the driver works on the rows [j0, j0 + n_local) of a domain of n_global points.  The workgroup geometry, the liveness of a
// position and the column loads are LOCAL (tid + u T < n_local); the weight is GLOBAL, W = w^(j0 + j) / (z - w^(j0 + j)) with w the generator of
// the global domain, so a lane starts from lag_pow(j0 + tid) of the global table.  The sum over j splits over blocks and every stored value is
// fully reduced: the unscaled shares of any partition of [0, n_global), added and scaled by k_lagrange_combine (lagrange_combine), are the bytes of
// the single call.  A point inside H is the row v[j* - j0] on the block that holds j* and zero elsewhere, and its scale in the combine is one, so
// one combine rule serves both kinds of point.  The batch call is the block form with j0 = 0, n_local = n_global and the scaled finish.
//
// COLUMN GROUPS: blockIdx.z of k_lagrange_partials splits the columns of a launch into contiguous groups (the last may be short); a workgroup
// recomputes the weights of its points and walks only its group's columns.  The layout of the partials does not depend on it, hence neither do
// the scratch, the passes or one byte of the result (lag_col_groups: the rule).
//
// SHARED INVERSE (context option "lagrange_shared_inverse" = 1): Montgomery's trick does not stop at a workgroup.  A pass then runs
//   k_lagrange_totals     grid (tiles, points): the product of a workgroup's differences, no inversion -> totals[p * grid + tile];
//   k_lagrange_invert     one workgroup per point: the `grid` totals of its point inverted with ONE Fermat inversion -> inv[p * grid + tile];
//   k_lagrange_partials   in its shared form: Pinv is read from inv, the inverting wave and its barrier are gone; every column group reads the
//                         same table.
// The two tables are arena blocks of pass_points * grid elements, sized once per call; all three launches are ordered on the context's stream.
// A total is never zero: a point outside H differs from every w^j.
//
// SHARED COSETS (context option "lagrange_share_cosets" = 1, the whole-domain form only): for z' = z w^s, W_j(z') = W_(j-s)(z) and z'^n = z^n, so
// f(z') = scale(z) * sum_i v[(i + s) mod n] W_i(z).  The driver sorts the points outside H into classes (lag_classes: a point joins the first earlier
// point of its coset, the class's representative; its shift is the 2-adic logarithm of their quotient) and a workgroup computes the weights of a
// representative once and walks the class's members, reading the columns at the member's shift (LagEntries).  The partials stay indexed by the
// member's own point, so the finish, the scales, the passes and the scratch do not change.  A pass boundary inside a class recomputes the
// representative's weights in the second part.  The block form ignores the option: a rotation leaves the block.  A call in which no two points
// share a coset takes the plain form.
// With both options the totals and the inverses exist per representative only.  Every stored value is fully reduced, so each combination gives the
// bytes of option 0.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <map>
#include <vector>
#include "fr.hpp"
#include "dev_common.hpp"

namespace stark {

constexpr int kLagK = 8;                                        // positions per lane (the merge's ALI_K)
constexpr int kLagMaxLogN = 30;
constexpr size_t kLagDefaultMaxPartials = (size_t)1 << 21;      // context option "lagrange_max_partials": 64 MiB of block partials per pass
constexpr size_t kLagMaxCols = (size_t)1 << 24;                 // blockIdx.x of k_lagrange_finish is the (point, column) pair
constexpr size_t kLagTargetWorkgroups = 1024;                   // point groups are added until a launch has about this many workgroups
constexpr size_t kLagGroupTargetWorkgroups = 512;               // column groups are added while a launch is below this, two workgroups per CU.  Measured at n = 2^17, 64 columns,
                                                                // 2 points (128 workgroups in one group; profiles/lagrange_shard_timing.jsonl): 2 / 4 / 8 groups run 0.73 / 0.71 / 1.07 x
                                                                // the time of one.  Three workgroups fit a CU, so 1024 leave a second round of a third while every group pays its weights
constexpr size_t kLagMinGroupCols = 8;                          // automatic column groups keep at least this many columns: a weight costs 7.75 products, a column term 1
constexpr size_t kLagMaxWorkgroups = (size_t)1 << 22;           // a launch stays below 2^30 lanes whatever "lagrange_col_groups" asks for
constexpr uint64_t kLagNoRow = ~0ull;                           // k_lagrange_gather: a point inside H whose row another block holds -> zero
constexpr bool kLagWideAcc = true;                              // a lane's K products of a column in the lazy accumulator (fr_wide): K multiplications, one reduction

// c0 = 1 view of a two-level power table (PowTable of ntt_dev.hpp, which is device-only): g^e = lo[e mod 2^lo_bits] * hi[e >> lo_bits]
struct LagPow { const fr_t* lo; const fr_t* hi; int lo_bits; };
FR_HD fr_t lag_pow(const LagPow& t, uint64_t e) {
    const fr_t a = ldg(t.lo + (e & ((1ull << t.lo_bits) - 1)));
    const uint64_t h = e >> t.lo_bits;
    return h ? fr_mul<PallasFr>(a, ldg(t.hi + h)) : a;
}
inline void lag_pow_split(size_t n, int* bits, int* lo_bits, int* hi_bits) {     // the split of the merge's omega_table (capi_fri.hip)
    int b = 0; while (((size_t)1 << b) < n) ++b;
    if (b < 1) b = 1;
    *bits = b; *lo_bits = (b + 1) / 2; *hi_bits = b - *lo_bits + 1;
}

// A launch over n positions: `grid` workgroups of 256 lanes, T = 256 grid lanes, lane tid owns j = tid + u T, u < K, where j < n.
struct LagGeom { unsigned grid; uint64_t T; };
inline LagGeom lag_geom(size_t n) {
    const uint64_t lanes = ((uint64_t)n + kLagK - 1) / kLagK; LagGeom g;
    g.grid = (unsigned)((lanes + 255) / 256); g.T = (uint64_t)g.grid * 256; return g;
}
// the points of one pass (a pass of one point is always allowed) and the point groups of its launch (group g walks the points g, g + groups, ...)
inline size_t lag_pass_points(size_t max_partials, size_t ncols, unsigned grid) { return std::max<size_t>(max_partials / (ncols * (size_t)grid), 1); }
inline unsigned lag_point_groups(size_t pass_points, unsigned grid) {
    return (unsigned)std::min<size_t>(std::min<size_t>(pass_points, 65535), std::max<size_t>((kLagTargetWorkgroups + grid - 1) / grid, 1));
}

// The column groups of a launch of `grid` tiles and `point_groups` point groups over ncols columns -> the columns per group; *groups = how many.
// opt = the context option "lagrange_col_groups": 1 = one group; g > 1 = min(g, ncols) groups; -1 = automatic: a group is added while every
// group keeps kLagMinGroupCols columns (a group pays the 7.75 products of a weight again for each of its points and positions, a column term is
// 1 product: at 8 columns the repeated work is below half) and the launch is below kLagGroupTargetWorkgroups.  No group is empty.
inline size_t lag_col_groups(int opt, size_t ncols, unsigned grid, unsigned point_groups, unsigned* groups) {
    const size_t wg = (size_t)grid * point_groups; size_t G = 1;
    if (opt < 0) while (ncols / (G + 1) >= kLagMinGroupCols && wg * G < kLagGroupTargetWorkgroups) ++G;
    else G = std::min<size_t>(std::min<size_t>(std::max(opt, 1), ncols), std::min<size_t>(std::max<size_t>(kLagMaxWorkgroups / wg, 1), 65535));
    const size_t per = (ncols + G - 1) / G;
    *groups = (unsigned)((ncols + per - 1) / per); return per;
}

// The rows [j0, j0 + n_local) of a domain of n_global points; scaled: the finish multiplies by (z^n - 1)/n (the batch call: the whole domain)
struct LagBlock { size_t n_local; uint64_t j0; size_t n_global; bool scaled; };
inline LagBlock lag_whole(size_t n) { return LagBlock{n, 0, n, true}; }

// The first collective of the sharded call all-gathers this header; ranks whose headers differ were given different arguments.
constexpr size_t kLagHdrWords = 8;                              // magic, n_global, ncols, npoints, digest of the omega and z bytes, pad
inline uint64_t lag_digest(uint64_t h, const void* bytes, size_t len) {     // FNV-1a, 64 bit
    const unsigned char* b = (const unsigned char*)bytes;
    for (size_t i = 0; i < len; ++i) { h ^= b[i]; h *= 0x100000001B3ull; }
    return h;
}
inline void lag_shard_header(size_t n_global, size_t ncols, size_t npoints, const fr_t& omega, const fr_t* z, uint64_t* h) {
    for (size_t i = 0; i < kLagHdrWords; ++i) h[i] = 0;
    h[0] = 0x4C41475348415244ull; h[1] = n_global; h[2] = ncols; h[3] = npoints;
    h[4] = lag_digest(lag_digest(0xCBF29CE484222325ull, &omega, sizeof(fr_t)), z, npoints * sizeof(fr_t));
}
inline bool lag_headers_agree(const uint64_t* all, size_t W, const uint64_t* mine) {
    for (size_t q = 0; q < W; ++q) for (size_t i = 0; i < kLagHdrWords; ++i) if (all[q * kLagHdrWords + i] != mine[i]) return false;
    return true;
}

// nullptr, or why (n, omega) is refused: n a power of two in 1 .. 2^30; omega a primitive n-th root of unity (omega^n = 1 and, for n >= 2,
// omega^(n/2) = -1), which is what makes every z with z^n = 1 a power of omega.
inline const char* lag_check_domain(size_t n, const fr_t& omega) {
    if (!n || (n & (n - 1))) return "n must be a power of two";
    if (n > ((size_t)1 << kLagMaxLogN)) return "n too large (at most 2^30)";
    if (!fr_eq(fr_pow_u64<PallasFr>(omega, n), fr_one<PallasFr>())) return "omega^n != 1";
    if (n >= 2 && !fr_eq(fr_pow_u64<PallasFr>(omega, n / 2), fr_neg<PallasFr>(fr_one<PallasFr>()))) return "omega is not a primitive n-th root of unity";
    return nullptr;
}
// j < 2^k with w^j = z, for z^(2^k) = 1 and w of order 2^k; winv2[i] = w^-(2^i).  Bit i of j is set iff (z w^-(j mod 2^i))^(2^(k-1-i)) = -1:
// one power compared against 1 per bit, about k^2 / 2 squarings in all.
inline uint64_t lag_dlog(const fr_t& z, const std::vector<fr_t>& winv2, int k) {
    const fr_t one = fr_one<PallasFr>(); fr_t cur = z; uint64_t j = 0;
    for (int i = 0; i < k; ++i) {
        fr_t t = cur; for (int s = 0; s < k - 1 - i; ++s) t = fr_sqr<PallasFr>(t);
        if (!fr_eq(t, one)) { j |= 1ull << i; cur = fr_mul<PallasFr>(cur, winv2[i]); }
    }
    return j;
}

// ---- the work of one lane (tid counted over the whole launch; tid + (K - 1) T < max(n, 2048) <= 2^30, so positions are 32-bit) ------------------
// tid, T and n are LOCAL to the block (n = n_local); w carries the global power w^(j0 + tid), so nothing below knows j0.
// The lane walks w^j over its K positions with w_step = w^T and back with its inverse, as ali_merge_block does, instead of holding K powers: the 64
// registers they would take are what lets three workgroups share a CU, and several resident workgroups are what covers a wave that inverts.
// forward: pre[u] = product of d_v = z - w^(j_v) over v < u (d = 1 past n); w: w^tid in, w^(tid + K T) out; returns the product over all K
FR_HD fr_t lag_prefix(const fr_t& z, fr_t& w, const fr_t& w_step, uint32_t tid, uint32_t T, uint32_t n, fr_t (&pre)[kLagK]) {
    fr_t run = fr_one<PallasFr>();
#pragma unroll
    for (int u = 0; u < kLagK; ++u) {
        const fr_t d = tid + (uint32_t)u * T < n ? fr_sub<PallasFr>(z, w) : fr_one<PallasFr>();
        pre[u] = run; run = u ? fr_mul<PallasFr>(run, d) : d;
        w = fr_mul<PallasFr>(w, w_step);
    }
    return run;
}
// 1 / (this lane's product) from Pinv = 1 / (the product over the workgroup), the four wave totals, and `others` = the product of the other lanes
// of its wave (formed before the inversion, so that one value and not two stays live across it)
FR_HD fr_t lag_lane_inverse(const fr_t& Pinv, const fr_t (&tot)[4], int wave, const fr_t& others) {
    fr_t inv = Pinv;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (i != wave) inv = fr_mul<PallasFr>(inv, tot[i]);
    return fr_mul<PallasFr>(inv, others);
}
// backward: peels the inverses off, pre[u] becomes the weight W_u = w^(j_u) / (z - w^(j_u))  (0 past n); w: w^(tid + K T) in, w^tid out
FR_HD void lag_peel(const fr_t& z, fr_t& w, const fr_t& w_step_inv, uint32_t tid, uint32_t T, uint32_t n, fr_t inv, fr_t (&pre)[kLagK]) {
#pragma unroll
    for (int u = kLagK - 1; u >= 0; --u) {
        const bool live = tid + (uint32_t)u * T < n;
        w = fr_mul<PallasFr>(w, w_step_inv);                                                          // back to w^(j_u)
        const fr_t dinv = u ? fr_mul<PallasFr>(inv, pre[u]) : inv;                                    // 1 / d_u
        if (u) inv = fr_mul<PallasFr>(inv, live ? fr_sub<PallasFr>(z, w) : fr_one<PallasFr>());
        pre[u] = live ? fr_mul<PallasFr>(w, dinv) : fr_zero<PallasFr>();
    }
}
// sum_u col[j_u] W_u.  WIDE: K multiplications into the lazy accumulator and one reduction (inputs below r, K <= 27 terms: fr.hpp); else K
// products and K additions.  Both are fully reduced, hence the same bits.
// ROT (a member of a coset class; n a power of two, the whole domain): the column is read at (j + shift) mod n where it was read at j; j, shift < n <= 2^30.
template <bool WIDE, bool ROT = false>
FR_HD fr_t lag_lane_dot(const fr_t* __restrict__ col, uint32_t tid, uint32_t T, uint32_t n, const fr_t (&W)[kLagK], uint32_t shift = 0) {
    if constexpr (WIDE) {
        fr_wide acc; fr_wide_zero(acc);
#pragma unroll
        for (int u = 0; u < kLagK; ++u) { const uint32_t j = tid + (uint32_t)u * T; fr_wide_mac_f<PallasFr>(acc, j < n ? ldg(col + (ROT ? (j + shift) & (n - 1) : j)) : fr_zero<PallasFr>(), W[u]); }
        return fr_wide_reduce<PallasFr>(acc);
    } else {
        fr_t acc = fr_zero<PallasFr>();
#pragma unroll
        for (int u = 0; u < kLagK; ++u) { const uint32_t j = tid + (uint32_t)u * T; if (j < n) acc = fr_add<PallasFr>(acc, fr_mul<PallasFr>(ldg(col + (ROT ? (j + shift) & (n - 1) : j)), W[u])); }
        return acc;
    }
}
FR_HD fr_t lag_sum4(const fr_t (&w)[4]) { return fr_add<PallasFr>(fr_add<PallasFr>(w[0], w[1]), fr_add<PallasFr>(w[2], w[3])); }
FR_HD fr_t lag_mul4(const fr_t (&w)[4]) { return fr_mul<PallasFr>(fr_mul<PallasFr>(fr_mul<PallasFr>(w[0], w[1]), w[2]), w[3]); }

// k_lagrange_invert: lane t of the one workgroup of a point owns the contiguous totals [lo, hi) of the point's `grid` (1 .. 2^19, so a lane may own many
// or none).  Forward: inv[i] = the product of the lane's totals before i, returns the product of all of them (one for a lane that owns none).
struct LagChunk { uint64_t lo, hi; };
FR_HD LagChunk lag_chunk(uint32_t lane, uint64_t grid) {
    const uint64_t ch = (grid + 255) / 256, lo = (uint64_t)lane * ch < grid ? (uint64_t)lane * ch : grid;
    LagChunk c; c.lo = lo; c.hi = lo + ch < grid ? lo + ch : grid; return c;
}
FR_HD fr_t lag_chunk_prefix(const fr_t* totals, const LagChunk& c, fr_t* inv) {
    fr_t run = fr_one<PallasFr>();
    for (uint64_t i = c.lo; i < c.hi; ++i) { stg(inv + i, run); run = fr_mul<PallasFr>(run, ldg(totals + i)); }
    return run;
}
// backward, from linv = 1 / (the lane's product): inv[i] = 1 / totals[i]
FR_HD void lag_chunk_peel(const fr_t* totals, const LagChunk& c, fr_t linv, fr_t* inv) {
    for (uint64_t i = c.hi; i-- > c.lo;) { stg(inv + i, fr_mul<PallasFr>(linv, ldg(inv + i))); linv = fr_mul<PallasFr>(linv, ldg(totals + i)); }
}

// The classes of a launch under "lagrange_share_cosets": class k has the representative's point zs[k] and the members [off[k], off[k + 1]) of
// `member` (the member's point index in the pass: the row of its partials) and `shift` (z_member = z_rep w^shift).  off null: class k is the point k
// alone, shift 0.
struct LagEntries { const uint32_t* off; const uint32_t* member; const uint32_t* shift; };
// The points outside H (zo, with zn[p] = zo[p]^n) in the caller's order: rep[p] = the first earlier point of p's coset of H, or p itself (a
// representative); shift[p] = the s with zo[p] = zo[rep[p]] w^s (0 for a representative and for an exact duplicate).  (z_p / z_q)^n = 1 iff
// z_p^n = z_q^n, so a class is found by its n-th power; z^n = 0 only for z = 0, whose class holds duplicates alone, so no zero is inverted.
inline void lag_classes(const std::vector<fr_t>& zo, const std::vector<fr_t>& zn, const std::vector<fr_t>& winv2, int k, std::vector<uint32_t>* rep, std::vector<uint32_t>* shift) {
    std::map<std::array<uint32_t, 8>, uint32_t> first;
    rep->assign(zo.size(), 0); shift->assign(zo.size(), 0);
    for (size_t p = 0; p < zo.size(); ++p) {
        std::array<uint32_t, 8> key; for (int i = 0; i < 8; ++i) key[(size_t)i] = zn[p].v[i];
        const auto it = first.emplace(key, (uint32_t)p).first;
        const uint32_t q = it->second; (*rep)[p] = q;
        if (q != p && !fr_eq(zo[p], zo[q])) (*shift)[p] = (uint32_t)lag_dlog(fr_mul<PallasFr>(zo[p], fr_inv<PallasFr>(zo[q])), winv2, k);
    }
}

// ---- the driver ------------------------------------------------------------------------------------------------------------------------
// The whole domain (B = lag_whole(n)): out[p * ncols + c] = lagrange_eval_on_h(cols[c], z[p], omega).  A block: out[p * ncols + c] = the block's
// unscaled share, sum over its rows of cols[c][j] w^(j0 + j) / (z[p] - w^(j0 + j)), or for z[p] = w^(j*) inside H the row j* - j0 if the block holds
// it and zero if not.  For the executor's memory (device: capi_fri.hip; host: hostcheck.cpp); cols[c] = the block's n_local rows.  The arguments
// have passed lag_check_domain and the null / overlap checks; ncols, npoints >= 1.  passes (may be null) = the partial passes taken.
// col_groups: the option "lagrange_col_groups" (lag_col_groups).
// An executor is an arena (alloc, put: DevArena in ctx.hpp, HostArena in hostcheck.cpp) plus  pow_table(omega, n, LagPow*)  gather(...)  totals(...)  invert(...)
// partials(...)  finish(...)  combine(...).
// shared_inverse, share_cosets: the options "lagrange_shared_inverse" and "lagrange_share_cosets" (1: on; the header comment).  Neither changes a byte
// of out, an error, a refusal or *passes.
template <class Exec>
int32_t lagrange_eval_batch(Exec& X, size_t ncols, const fr_t* const* cols, const LagBlock& B, const fr_t& omega, size_t npoints, const fr_t* z, size_t max_partials,
                            int col_groups, int shared_inverse, int share_cosets, fr_t* out, size_t* passes) {
    const size_t n = B.n_global;
    const fr_t one = fr_one<PallasFr>(), n_inv = fr_inv<PallasFr>(fr_from_u64<PallasFr>((uint64_t)n));
    int k = 0; while (((size_t)1 << k) < n) ++k;
    std::vector<fr_t> winv2((size_t)k);
    if (k) { winv2[0] = fr_inv<PallasFr>(omega); for (int i = 1; i < k; ++i) winv2[(size_t)i] = fr_sqr<PallasFr>(winv2[(size_t)i - 1]); }
    bool cosets = share_cosets == 1 && B.scaled && B.j0 == 0 && B.n_local == B.n_global && npoints <= 0xFFFFFFFFull;      // the whole-domain form only: a rotation leaves a block
    const bool shared = shared_inverse == 1;
    std::vector<fr_t> zo, zno, scale; std::vector<uint64_t> slot_o, jin, slot_i;     // outside H: point, its n-th power, scale, index of the point in the call; inside: local row (or kLagNoRow), index
    for (size_t p = 0; p < npoints; ++p) {
        const fr_t zn = fr_pow_u64<PallasFr>(z[p], (uint64_t)n);
        if (fr_eq(zn, one)) {
            const uint64_t j = lag_dlog(z[p], winv2, k);
            jin.push_back(j >= B.j0 && j - B.j0 < B.n_local ? j - B.j0 : kLagNoRow); slot_i.push_back((uint64_t)p);
        } else { zo.push_back(z[p]); if (cosets) zno.push_back(zn); if (B.scaled) scale.push_back(fr_mul<PallasFr>(fr_sub<PallasFr>(zn, one), n_inv)); slot_o.push_back((uint64_t)p); }
    }
    if (passes) *passes = 0;
    const fr_t** d_cols = nullptr;
    { std::vector<const fr_t*> h(cols, cols + ncols); int32_t rc = X.put(h, &d_cols); if (rc) return rc; }
    if (!jin.empty()) {
        uint64_t *d_j = nullptr, *d_slot = nullptr;
        int32_t rc = X.put(jin, &d_j); if (rc) return rc;
        rc = X.put(slot_i, &d_slot); if (rc) return rc;
        rc = X.gather((const fr_t* const*)d_cols, ncols, d_j, d_slot, jin.size(), out); if (rc) return rc;
    }
    if (zo.empty()) return 0;
    const LagGeom G = lag_geom(B.n_local);
    const size_t per_pass = std::min(lag_pass_points(max_partials, ncols, G.grid), zo.size());
    if (passes) *passes = (zo.size() + per_pass - 1) / per_pass;
    // The classes of every pass, side by side: pass i has the classes [cls0[i], cls0[i + 1]) of ez (the representative's point; it may lie in an earlier
    // pass), their member ranges at coff[cls0[i] + i ..] and its points' entries at [p0, p0 + pp) of member / mshift, sorted by class in order of appearance.
    std::vector<fr_t> ez; std::vector<uint32_t> coff, member, mshift; std::vector<size_t> cls0;
    std::vector<uint32_t> rep, shift;
    if (cosets) {                                                                             // no two points in one coset: nothing to share, the call takes the plain form
        lag_classes(zo, zno, winv2, k, &rep, &shift);
        cosets = false; for (size_t p = 0; p < zo.size(); ++p) cosets = cosets || rep[p] != p;
    }
    if (cosets) {
        member.resize(zo.size()); mshift.resize(zo.size());
        for (size_t p0 = 0; p0 < zo.size(); p0 += per_pass) {
            const size_t pp = std::min(per_pass, zo.size() - p0), c0 = ez.size(), o0 = coff.size();
            std::map<uint32_t, uint32_t> idx; std::vector<uint32_t> local(pp);
            for (size_t i = 0; i < pp; ++i) {
                const auto it = idx.emplace(rep[p0 + i], (uint32_t)idx.size());
                if (it.second) ez.push_back(zo[rep[p0 + i]]);
                local[i] = it.first->second;
            }
            const size_t nc = ez.size() - c0;
            cls0.push_back(c0); coff.resize(o0 + nc + 1, 0);
            for (size_t i = 0; i < pp; ++i) ++coff[o0 + local[i] + 1];
            for (size_t c = 0; c < nc; ++c) coff[o0 + c + 1] += coff[o0 + c];
            std::vector<uint32_t> at(coff.begin() + (ptrdiff_t)o0, coff.begin() + (ptrdiff_t)(o0 + nc));
            for (size_t i = 0; i < pp; ++i) { const uint32_t m = at[local[i]]++; member[p0 + m] = (uint32_t)i; mshift[p0 + m] = shift[p0 + i]; }
        }
        cls0.push_back(ez.size());
    }
    fr_t *d_z = nullptr, *d_scale = nullptr, *d_ez = nullptr; uint64_t* d_slot = nullptr; uint32_t *d_coff = nullptr, *d_member = nullptr, *d_mshift = nullptr;
    void *d_part = nullptr, *d_tot = nullptr, *d_inv = nullptr; LagPow wp;
    int32_t rc = X.put(zo, &d_z); if (rc) return rc;
    if (B.scaled) { rc = X.put(scale, &d_scale); if (rc) return rc; }
    rc = X.put(slot_o, &d_slot); if (rc) return rc;
    if (cosets) {
        rc = X.put(ez, &d_ez); if (rc) return rc;
        rc = X.put(coff, &d_coff); if (rc) return rc;
        rc = X.put(member, &d_member); if (rc) return rc;
        rc = X.put(mshift, &d_mshift); if (rc) return rc;
    }
    rc = X.alloc(per_pass * ncols * G.grid * sizeof(fr_t), &d_part); if (rc) return rc;       // reused by every pass: they are ordered on one stream
    if (shared) {                                                                             // the totals and their inverses of the largest pass, reused like the partials
        rc = X.alloc(per_pass * G.grid * sizeof(fr_t), &d_tot); if (rc) return rc;
        rc = X.alloc(per_pass * G.grid * sizeof(fr_t), &d_inv); if (rc) return rc;
    }
    rc = X.pow_table(omega, n, &wp); if (rc) return rc;
    const fr_t w_step = fr_pow_u64<PallasFr>(omega, G.T), w_step_inv = fr_inv<PallasFr>(w_step);
    for (size_t p0 = 0, pass = 0; p0 < zo.size(); p0 += per_pass, ++pass) {
        const size_t pp = std::min(per_pass, zo.size() - p0);
        const size_t nc = cosets ? cls0[pass + 1] - cls0[pass] : pp;                          // the classes of the pass: what a point group hands out
        const fr_t* cz = cosets ? d_ez + cls0[pass] : d_z + p0;
        const LagEntries E = cosets ? LagEntries{d_coff + cls0[pass] + pass, d_member + p0, d_mshift + p0} : LagEntries{nullptr, nullptr, nullptr};
        const unsigned pg = lag_point_groups(nc, G.grid); unsigned cg = 1;
        const size_t group_cols = lag_col_groups(col_groups, ncols, G.grid, pg, &cg);
        if (shared) {
            rc = X.totals(B.n_local, B.j0, wp, w_step, cz, nc, G.grid, (fr_t*)d_tot); if (rc) return rc;
            rc = X.invert((const fr_t*)d_tot, nc, G.grid, (fr_t*)d_inv); if (rc) return rc;
        }
        rc = X.partials((const fr_t* const*)d_cols, ncols, B.n_local, B.j0, wp, w_step, w_step_inv, cz, nc, E, (const fr_t*)d_inv, pg, cg, group_cols, G.grid, (fr_t*)d_part); if (rc) return rc;
        rc = X.finish((const fr_t*)d_part, G.grid, B.scaled ? d_scale + p0 : nullptr, d_slot + p0, pp, ncols, out); if (rc) return rc;     // no scale: the unscaled finish
    }
    return 0;
}
// out[p * ncols + c] = scale[p] * sum over q < nparts of partials[(q * npoints + p) * ncols + c], scale = (z^n - 1)/n outside H and one inside:
// lagrange_eval_on_h of the whole columns when the parts are the blocks' shares of a partition of [0, n).
template <class Exec>
int32_t lagrange_combine(Exec& X, size_t nparts, const fr_t* partials, size_t ncols, size_t n, size_t npoints, const fr_t* z, fr_t* out) {
    const fr_t one = fr_one<PallasFr>(), n_inv = fr_inv<PallasFr>(fr_from_u64<PallasFr>((uint64_t)n));
    std::vector<fr_t> scale(npoints);
    for (size_t p = 0; p < npoints; ++p) {
        const fr_t zn = fr_pow_u64<PallasFr>(z[p], (uint64_t)n);
        scale[p] = fr_eq(zn, one) ? one : fr_mul<PallasFr>(fr_sub<PallasFr>(zn, one), n_inv);
    }
    fr_t* d_scale = nullptr;
    int32_t rc = X.put(scale, &d_scale); if (rc) return rc;
    return X.combine(partials, nparts, (const fr_t*)d_scale, npoints, ncols, out);
}

#if defined(__HIPCC__)
__device__ __forceinline__ void lag_st_lds(uint4* p, int i, const fr_t& x) { p[2 * i] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]); p[2 * i + 1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]); }
__device__ __forceinline__ fr_t lag_ld_lds(const uint4* p, int i) {
    const uint4 lo = p[2 * i], hi = p[2 * i + 1]; fr_t x;
    x.v[0] = lo.x; x.v[1] = lo.y; x.v[2] = lo.z; x.v[3] = lo.w; x.v[4] = hi.x; x.v[5] = hi.y; x.v[6] = hi.z; x.v[7] = hi.w; return x;
}
// Workgroup blockIdx.x of gridDim.x tiles, point group blockIdx.y: the classes blockIdx.y, blockIdx.y + gridDim.y, ... < npts of zs (a class is one
// point unless COSETS); column group blockIdx.z: the columns [blockIdx.z * group_cols, + group_cols) below ncols;
// partials[(p * ncols + c) * gridDim.x + blockIdx.x] = this workgroup's share of sum_j cols[c][j] W_(j0 + j)(z_p) over the n64 local rows.
// A lane past the block (tid >= n) reads no power: j0 + tid may lie past the table of the global domain.  The scan-and-invert step is the
// one of ali_merge_block (fri_dev.hpp), whose comment says why one inversion per lane would dwarf the useful work; it is a copy, not a shared
// helper, so that the merge kernels' code does not move (open unification).
// SHARED: 1 / (the workgroup's product) is inv[k * gridDim.x + blockIdx.x] (k_lagrange_totals, k_lagrange_invert) and no wave inverts.
// COSETS: zs[k] is the representative of class k; its weights serve the members E.off[k] .. E.off[k + 1]: member m writes the partials of the point
// E.member[m] from the columns read at the shift E.shift[m] (whole domain: j0 = 0, n a power of two).
template <bool WIDE, bool SHARED, bool COSETS>
__global__ void __launch_bounds__(256, 3) k_lagrange_partials(const fr_t* const* __restrict__ cols, uint64_t ncols, uint64_t n64, uint64_t j0, LagPow wp, fr_t w_step, fr_t w_step_inv,
                                                           const fr_t* __restrict__ zs, uint64_t npts, LagEntries E, const fr_t* __restrict__ inv, uint64_t group_cols, fr_t* __restrict__ partials) {
    __shared__ uint4 tot[2 * 4], pinv[2], red[2][2 * 4];
    const uint32_t T = gridDim.x * 256, tid = blockIdx.x * 256 + threadIdx.x, n = (uint32_t)n64;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const uint64_t c_lo = (uint64_t)blockIdx.z * group_cols, c_hi = c_lo + group_cols < ncols ? c_lo + group_cols : ncols;
    fr_t w = COSETS || tid >= n ? fr_one<PallasFr>() : lag_pow(wp, j0 + tid); // w^(j0 + tid); every point leaves it there again
    uint32_t half = 0;                                              // COSETS: which half of red[] the next column sum takes
    for (uint64_t p = blockIdx.y; p < npts; p += gridDim.y) {
        const fr_t z = ldg(zs + p);
        fr_t W[kLagK];
        if constexpr (COSETS) w = tid < n ? lag_pow(wp, j0 + tid) : fr_one<PallasFr>();          // read per class, not kept: eight registers less across the members' columns
        const fr_t run = lag_prefix(z, w, w_step, tid, T, n, W);
        fr_t pre_i = run, suf_i = run;                              // inclusive prefix / suffix products of the lanes' `run` over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const fr_t a = shfl_up_fr(pre_i, d), b = shfl_dn_fr(suf_i, d);
            if (ln >= d) pre_i = fr_mul<PallasFr>(pre_i, a);
            if (ln + d < 64) suf_i = fr_mul<PallasFr>(suf_i, b);
        }
        fr_t before = shfl_up_fr(pre_i, 1), after = shfl_dn_fr(suf_i, 1);
        if (ln == 0) before = fr_one<PallasFr>();
        if (ln == 63) after = fr_one<PallasFr>();
        if (ln == 63) lag_st_lds(tot, wv, pre_i);
        const fr_t others = fr_mul<PallasFr>(before, after);
        __syncthreads();
        if constexpr (!SHARED) {
            // ONE Fermat inversion per workgroup and point, by one wave while the other three wait.  Which wave rotates with the workgroup, so that the
            // workgroups resident on a CU (three fit: launch bound) tend to invert on different SIMDs instead of all on wave 0's.
            if (wv == (int)((blockIdx.x + (blockIdx.x >> 8) + p) & 3)) {
                fr_t P = lag_ld_lds(tot, 0);
                for (int i = 1; i < 4; ++i) P = fr_mul<PallasFr>(P, lag_ld_lds(tot, i));
                const fr_t Pi = fr_inv<PallasFr>(P);
                if (ln == 0) lag_st_lds(pinv, 0, Pi);
            }
            __syncthreads();
        }
        {
            const fr_t t4[4] = {lag_ld_lds(tot, 0), lag_ld_lds(tot, 1), lag_ld_lds(tot, 2), lag_ld_lds(tot, 3)};
            const fr_t Pinv = SHARED ? ldg(inv + (p * gridDim.x + blockIdx.x)) : lag_ld_lds(pinv, 0);
            lag_peel(z, w, w_step_inv, tid, T, n, lag_lane_inverse(Pinv, t4, wv, others), W);
        }
        // The columns: the pointer table is indexed, never a register array.  red[] alternates between two halves, so one barrier per column
        // orders thread 0's reads of a half before its next writers; tot and pinv of the next point are written behind at least that barrier.
        // (COSETS: the halves alternate over the members' columns, since a group of one column would meet the same half again in the next member.)
        const uint32_t m_lo = COSETS ? E.off[p] : 0, m_hi = COSETS ? E.off[p + 1] : 1;
        for (uint32_t m = m_lo; m < m_hi; ++m) {
            const uint64_t q = COSETS ? (uint64_t)E.member[m] : p;  // the point whose partials these are
            const uint32_t shift = COSETS ? E.shift[m] : 0;
            for (uint64_t c = c_lo; c < c_hi; ++c) {
                fr_t acc = lag_lane_dot<WIDE, COSETS>(cols[c], tid, T, n, W, shift);
#pragma unroll
                for (int sft = 1; sft < 64; sft <<= 1) acc = fr_add<PallasFr>(acc, shfl_xor_fr(acc, sft));
                uint4* r = red[COSETS ? half++ & 1 : c & 1];
                if (ln == 0) lag_st_lds(r, wv, acc);
                __syncthreads();
                if (threadIdx.x == 0) {
                    const fr_t w4[4] = {lag_ld_lds(r, 0), lag_ld_lds(r, 1), lag_ld_lds(r, 2), lag_ld_lds(r, 3)};
                    stg(partials + ((q * ncols + c) * gridDim.x + blockIdx.x), lag_sum4(w4));
                }
            }
        }
    }
}
// "lagrange_shared_inverse", step 1.  Workgroup blockIdx.x of gridDim.x tiles, the points blockIdx.y, blockIdx.y + gridDim.y, ... < npts:
// totals[p * gridDim.x + blockIdx.x] = the product of the workgroup's differences z_p - w^(j0 + j) over its live positions (a dead position
// contributes one), in the geometry of k_lagrange_partials: what that kernel's own scan would invert.  No inversion here.
static __global__ void __launch_bounds__(256) k_lagrange_totals(uint64_t n64, uint64_t j0, LagPow wp, fr_t w_step, const fr_t* __restrict__ zs, uint64_t npts, fr_t* __restrict__ totals) {
    __shared__ uint4 tot[2 * 4];
    const uint32_t T = gridDim.x * 256, tid = blockIdx.x * 256 + threadIdx.x, n = (uint32_t)n64;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const fr_t w0 = tid < n ? lag_pow(wp, j0 + tid) : fr_one<PallasFr>();
    for (uint64_t p = blockIdx.y; p < npts; p += gridDim.y) {
        fr_t w = w0, pre[kLagK];
        fr_t run = lag_prefix(ldg(zs + p), w, w_step, tid, T, n, pre);
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) run = fr_mul<PallasFr>(run, shfl_xor_fr(run, sft));
        if (ln == 0) lag_st_lds(tot, wv, run);
        __syncthreads();
        if (threadIdx.x == 0) {
            const fr_t t4[4] = {lag_ld_lds(tot, 0), lag_ld_lds(tot, 1), lag_ld_lds(tot, 2), lag_ld_lds(tot, 3)};
            stg(totals + (p * gridDim.x + blockIdx.x), lag_mul4(t4));
        }
        __syncthreads();                                            // tot is read before the next point writes it
    }
}
// "lagrange_shared_inverse", step 2.  One workgroup per point: inv[p * grid + i] = 1 / totals[p * grid + i], i < grid, with ONE Fermat inversion.  A lane
// owns a contiguous chunk of the totals (lag_chunk) and passes over it twice: forward it leaves its running products in inv and keeps their
// product; the lanes' products go through the two-level scan of k_lagrange_partials and one wave inverts the grand product; backward the lane peels
// its chunk.  A lane reads back only what it wrote itself, so inv is no __restrict__ pointer and nothing else orders the two passes.
static __global__ void __launch_bounds__(256) k_lagrange_invert(const fr_t* __restrict__ totals, uint64_t grid, fr_t* inv) {
    __shared__ uint4 tot[2 * 4], pinv[2];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const fr_t* t = totals + (uint64_t)blockIdx.x * grid; fr_t* o = inv + (uint64_t)blockIdx.x * grid;
    const LagChunk ch = lag_chunk(threadIdx.x, grid);
    const fr_t run = lag_chunk_prefix(t, ch, o);
    fr_t pre_i = run, suf_i = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const fr_t a = shfl_up_fr(pre_i, d), b = shfl_dn_fr(suf_i, d);
        if (ln >= d) pre_i = fr_mul<PallasFr>(pre_i, a);
        if (ln + d < 64) suf_i = fr_mul<PallasFr>(suf_i, b);
    }
    fr_t before = shfl_up_fr(pre_i, 1), after = shfl_dn_fr(suf_i, 1);
    if (ln == 0) before = fr_one<PallasFr>();
    if (ln == 63) after = fr_one<PallasFr>();
    if (ln == 63) lag_st_lds(tot, wv, pre_i);
    const fr_t others = fr_mul<PallasFr>(before, after);
    __syncthreads();
    if (wv == 0) {
        const fr_t t4[4] = {lag_ld_lds(tot, 0), lag_ld_lds(tot, 1), lag_ld_lds(tot, 2), lag_ld_lds(tot, 3)};
        const fr_t Pi = fr_inv<PallasFr>(lag_mul4(t4));
        if (ln == 0) lag_st_lds(pinv, 0, Pi);
    }
    __syncthreads();
    const fr_t t4[4] = {lag_ld_lds(tot, 0), lag_ld_lds(tot, 1), lag_ld_lds(tot, 2), lag_ld_lds(tot, 3)};
    lag_chunk_peel(t, ch, lag_lane_inverse(lag_ld_lds(pinv, 0), t4, wv, others), o);
}
// One block per (point, column) of a pass, in the shape of k_sum_single_block: out[slot[p] * ncols + c] = scale[p] * the sum of the pair's `grid` partials
// (scale null: the sum itself, a block's unscaled share).
static __global__ void __launch_bounds__(256) k_lagrange_finish(const fr_t* __restrict__ partials, uint64_t grid, const fr_t* __restrict__ scale, const uint64_t* __restrict__ slot,
                                                                uint64_t ncols, fr_t* __restrict__ out) {
    __shared__ uint4 red[2 * 4];
    const uint64_t p = blockIdx.x / ncols, c = blockIdx.x % ncols;
    const fr_t* v = partials + (uint64_t)blockIdx.x * grid;
    fr_t acc = fr_zero<PallasFr>();
    for (uint64_t i = threadIdx.x; i < grid; i += 256) acc = fr_add<PallasFr>(acc, ldg(v + i));
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) acc = fr_add<PallasFr>(acc, shfl_xor_fr(acc, sft));
    if ((threadIdx.x & 63) == 0) lag_st_lds(red, threadIdx.x >> 6, acc);
    __syncthreads();
    if (threadIdx.x == 0) {
        const fr_t w4[4] = {lag_ld_lds(red, 0), lag_ld_lds(red, 1), lag_ld_lds(red, 2), lag_ld_lds(red, 3)};
        const fr_t sum = lag_sum4(w4);
        stg(out + slot[p] * ncols + c, scale ? fr_mul<PallasFr>(sum, ldg(scale + p)) : sum);
    }
}
// The points inside H: out[slot[q] * ncols + c] = cols[c][j[q]] for the `cnt` such points and all columns, copied; j[q] = kLagNoRow (the row belongs to
// another block): zero.
static __global__ void __launch_bounds__(256) k_lagrange_gather(const fr_t* const* __restrict__ cols, uint64_t ncols, const uint64_t* __restrict__ j, const uint64_t* __restrict__ slot,
                                                                uint64_t cnt, fr_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt * ncols) return;
    const uint64_t q = i / ncols, c = i % ncols;
    stg(out + slot[q] * ncols + c, j[q] == kLagNoRow ? fr_zero<PallasFr>() : ldg(cols[c] + j[q]));
}
// The combine of the blocks' shares, one lane per result (nparts is a rank count): out[i] = scale[i / ncols] * sum_q partials[q * total + i].
static __global__ void __launch_bounds__(256) k_lagrange_combine(const fr_t* __restrict__ partials, uint64_t nparts, const fr_t* __restrict__ scale, uint64_t total, uint64_t ncols,
                                                                 fr_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    fr_t acc = ldg(partials + i);
    for (uint64_t q = 1; q < nparts; ++q) acc = fr_add<PallasFr>(acc, ldg(partials + q * total + i));
    stg(out + i, fr_mul<PallasFr>(acc, ldg(scale + i / ncols)));
}
#endif  // __HIPCC__

}  // namespace stark
