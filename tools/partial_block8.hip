// tools/partial_block8.hip — PROTOTYPE, not product code: 8 partial rounds of the t = 17 Poseidon permutation for 64 sponges per wave pair, in several forms.
//   form 4      : the shipped block-of-4 code, twice — pair_permute<17> of poseidon_pair.hpp itself, run with rf = 0 and rp = 8 (no full rounds);
//   former 8    : one block of 8 rounds whose E-product (8 rows x 16 lanes) and lane product (16 rows x 8 S-box outputs, plus the base lane as a ninth
//                 K-step) run on the matrix cores through residue tables, the 28 Gamma terms of the block on the vector ALU (namespace former below: the
//                 product's form until the Gamma terms moved; kept here as the comparison);
//   form 8      : the product's pair_block8 (poseidon_pair.hpp, where the schedule is described): the Gamma terms as q further K-steps of row q's tile,
//                 X posting y_q recoded, the chain SCALED (s0 = lambda_q X_q, no a_q y_q product; tables blk8s_*) and carried as a LAZY RESIDUE: H_q handed
//                 over as its nine finish limbs with the next round's constant in them, no field element formed inside the block.  Instantiated for several
//                 shares of the lane rows (NLX).  The one product by 1 / lambda_8 that brings X_8 back runs in the checked repetition only: a permutation
//                 pays it once per eight blocks;
//   canonical 8 : the same schedule with a canonical chain value in every round (namespace canonical below: the product's form until the chain became a lazy
//                 residue; kept here as the comparison) — fr_add with the constant, fr_pow5_r29, recode, and after the barrier fr_add with a canonical H_q;
//   unscaled 8  : the same schedule with the chain unscaled, a_q y_q as a nine-limb product in every round of X (namespace unscaled below: the product's
//                 form until the chain was scaled; kept here as the comparison; tables blk8_*);
//   form 8 piped: the scaled form with wave Y software-pipelined across the round barrier (namespace piped below), measured and not adopted.
//   between two blocks: form 8 as a block that is NOT the permutation's last, its lanes left as the digits of their signed residue — the product's byte-domain
//                 finish (mfma_post_bytes: word columns folded per lane, 8 swaps, one pass over eight words) beside the finish through nine 29-bit limbs
//                 (namespace limbfinish below: the product's form until the byte finish; kept here as the comparison).  The host decodes the digits.
//   word columns: the rows that end as nine limbs — wave Y's H_q rows and, in a permutation's last block, the lane rows handed to the next S-box — by the product's
//                 mfma_post_limbs (multiply-add fold per lane, 8 swaps, one pass over eight words) beside the finish through nine limb columns (namespace limbrows
//                 below: the product's form until then; kept here as the comparison), as a block between two blocks and as a permutation's last block.
//   LDS stays at PairCfg<17>::lds_bytes() = 40 KiB.  The host checks every form against the sparse rounds in the portable field code (0 and r - 1 among
//   the inputs) and requires zero mismatches; then the forms are timed alternately in one process, the state reloaded from memory for every repetition.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I stark_mlwe_amd/csrc tools/partial_block8.hip -o tools/bin/partial_block8
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "host_util.hpp"
#include "poseidon_pair.hpp"
using namespace stark;
constexpr int T = 17, W = 2 * T - 1, B8 = 8;

// ---- the FORMER form of the block, kept here as the comparison: the Gamma terms on the vector ALU (Y the YG youngest per round, X the older ones, each
// term a nine-limb unpack and 81 MACs, a wide reduction and an add per round in Y), the y held as field elements by both waves and brought to the B layout
// at the end of the block.  The product no longer contains it.
namespace former {
struct Tabs {
    const mfma_v4i* efrag;     // [8][16][64]   row q, lane j = 1..16
    const mfma_v4i* lfrag;     // [16][8][64]   lane j = 1..16, S-box output p
    const mfma_v4i* unit;      // [64]          the constant 1
    const uint32_t* a29;       // a_q at c29(a29, q * (2 T - 1)): the block's first row of sparse29
    const uint32_t* g29;       // [28][9]       Gamma_{q,p} at q (q - 1) / 2 + p
    const fr_t* rc;            // [8]
};
struct Cfg {
    // Y's share of a round's gamma terms (the YG youngest) and X's share of the lane rows: 5 / 8 measured best, the neighbours within 1.5 %
    // (YG 6 with NLX 8: +1.5 %, YG 6 with NLX 7: +0.2 %, YG 7 with NLX 9: +1.1 %; run-to-run spread 1.5 %)
    static constexpr int YG = 5, NLX = 8;
    __host__ __device__ static constexpr int ymail(int q) { return 17 + (q & 1); }
    __host__ __device__ static constexpr int hmail(int q) { return (q & 1) ? 19 : 0; }
};
template <int Q, int P, int LO, int HI>
__device__ __forceinline__ void gterm(fr_wide29& acc, const Tabs& Tb, const fr_t (&yk)[8]) {          // gamma term p of round Q, if p is in [LO, HI)
    if constexpr (P < Q && P >= LO && P < HI) fr_wide29_mac(acc, c29(Tb.g29, Q * (Q - 1) / 2 + P), fr29_unpack(yk[P]));
}
template <int Q, int LO, int HI>
__device__ __forceinline__ void gterms(fr_wide29& acc, const Tabs& Tb, const fr_t (&yk)[8]) {
    gterm<Q, 0, LO, HI>(acc, Tb, yk); gterm<Q, 1, LO, HI>(acc, Tb, yk); gterm<Q, 2, LO, HI>(acc, Tb, yk); gterm<Q, 3, LO, HI>(acc, Tb, yk);
    gterm<Q, 4, LO, HI>(acc, Tb, yk); gterm<Q, 5, LO, HI>(acc, Tb, yk); gterm<Q, 6, LO, HI>(acc, Tb, yk);
}
// round Q in wave X: at most 1 + 7 - YG terms, within fr29_max_terms
template <int Q, int YG>
__device__ __forceinline__ void round_x(const PairState& s, const Tabs& Tb, fr_t& s0, fr_t (&yk)[8]) {
    __builtin_amdgcn_sched_barrier(0);                     // keep the rounds apart: less register pressure
    yk[Q] = fr_pow5_r29<PF>(fr_add<PF>(s0, Tb.rc[Q]));
    s.sto(Cfg::ymail(Q), yk[Q]);
    fr_wide29 acc; fr_wide29_zero(acc);
    fr_wide29_mac(acc, c29(Tb.a29, (size_t)Q * (2 * 17 - 1)), fr29_unpack(yk[Q]));
    gterms<Q, 0, (Q - YG > 0 ? Q - YG : 0)>(acc, Tb, yk);
    const fr_t part = fr_wide29_reduce<PF>(acc);
    __syncthreads();                                       // barrier_Q: H_Q is posted
    s0 = fr_add<PF>(part, s.ld(Cfg::hmail(Q)));
}
// round Q in wave Y.  a: the fragments of E row Q on entry, of row Q + 1 on exit
template <int Q, int YG>
__device__ __forceinline__ void round_y(const PairState& s, const Tabs& Tb, fr_t (&yk)[8], mfma_v4i (&a)[16]) {
    __builtin_amdgcn_sched_barrier(0);
    const int lane = s.lane, h = lane >> 5;
    mfma_v16i acc[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const uint4 u = s.st[(2 * (e + 1) + h) * 64 + 32 * ct + (lane & 31)];
            acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[e], mfma_v4i{(int)u.x, (int)u.y, (int)u.z, (int)u.w}, acc[ct], 0, 0, 0);
        }
    if constexpr (Q < 7) blk8_load_frags16(a, Tb.efrag + (size_t)(Q + 1) * 16 * 64, lane);
    fr_t hq = mfma_post(acc);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (Q > 0) {
        fr_wide29 w; fr_wide29_zero(w);
        gterms<Q, (Q - YG > 0 ? Q - YG : 0), Q>(w, Tb, yk);
        hq = fr_add<PF>(hq, fr_wide29_reduce<PF>(w));
    }
    s.sto(Cfg::hmail(Q), hq);
    __syncthreads();                                       // barrier_Q: y_Q is posted
    yk[Q] = s.ld(Cfg::ymail(Q));
}
// One block.  Precondition: lanes 1..16 RECODED in their slots and a barrier since; s0 = X_0 in wave X.  Ends with a barrier, the lanes recoded again,
// or canonical after the permutation's last block.
template <int YG, int NLX>
__device__ __forceinline__ void pair_block8(const PairState& s, const Tabs& Tb, fr_t& s0, bool last) {
    static_assert(YG >= 1 && YG <= 7 && NLX >= 1 && NLX <= 15, "shares");
    static_assert(YG <= fr29_max_terms<PF>() && 1 + 7 - YG <= fr29_max_terms<PF>(), "Y sums YG terms, X up to 1 + 7 - YG, without a carry pass in between");
    const int lane = s.lane, h = lane >> 5;
    fr_t yk[8];
    if (!s.isY) {
        round_x<0, YG>(s, Tb, s0, yk); round_x<1, YG>(s, Tb, s0, yk); round_x<2, YG>(s, Tb, s0, yk); round_x<3, YG>(s, Tb, s0, yk);
        round_x<4, YG>(s, Tb, s0, yk); round_x<5, YG>(s, Tb, s0, yk); round_x<6, YG>(s, Tb, s0, yk); round_x<7, YG>(s, Tb, s0, yk);
    } else {
        mfma_v4i a[16];
        blk8_load_frags16(a, Tb.efrag, lane);
        round_y<0, YG>(s, Tb, yk, a); round_y<1, YG>(s, Tb, yk, a); round_y<2, YG>(s, Tb, yk, a); round_y<3, YG>(s, Tb, yk, a);
        round_y<4, YG>(s, Tb, yk, a); round_y<5, YG>(s, Tb, yk, a); round_y<6, YG>(s, Tb, yk, a); round_y<7, YG>(s, Tb, yk, a);
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma_v4i b[8][2];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const fr_t yr = recode_signed(yk[p]);
#pragma unroll
        for (int w = 0; w < 4; ++w) {      // afterwards b[p][ct] = half (lane >> 5) of y_p of sponge 32 ct + (lane & 31)
            const auto sw = __builtin_amdgcn_permlane32_swap(yr.v[w], yr.v[4 + w], false, false);
            b[p][0][w] = (int)sw[0]; b[p][1][w] = (int)sw[1];
        }
    }
    const int j0 = s.isY ? NLX + 1 : 1, j1 = s.isY ? 16 : NLX;
    const mfma_v4i aunit = Tb.unit[lane];
    mfma_v4i a[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) a[p] = (Tb.lfrag + ((size_t)(j0 - 1) * 8 + p) * 64)[lane];
#pragma unroll 1
    for (int j = j0; j <= j1; ++j) {
        mfma_v16i acc[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[p], b[p][ct], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const uint4 u = s.st[(2 * j + h) * 64 + 32 * ct + (lane & 31)];
            acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aunit, mfma_v4i{(int)u.x, (int)u.y, (int)u.z, (int)u.w}, acc[ct], 0, 0, 0);
        }
        const int jn = j < j1 ? j + 1 : j1;                // the last row fetches its own fragments again: in bounds, unused
#pragma unroll
        for (int p = 0; p < 8; ++p) a[p] = (Tb.lfrag + ((size_t)(jn - 1) * 8 + p) * 64)[lane];
        const fr_t z = mfma_post(acc);
        s.sto(j, last ? z : recode_signed(z));             // slot j is read by this wave alone, before this write
    }
    __syncthreads();
}
}  // namespace former

// ---- the product's schedule with a CANONICAL chain value in every round, kept here as the comparison: wave X adds the scaled constant (fr_add), runs
// fr_pow5_r29 (unpack, three products, pack, conditional subtraction), posts the recoded y and adds the canonical H_q (mfma_post: pack and two conditional
// subtractions in wave Y) after the barrier.  The lane rows are the product's.  The product no longer contains it.
namespace canonical {
struct Tabs { const mfma_v4i* efrag; const mfma_v4i* lfrag; const mfma_v4i* unit; const mfma_v4i* gfrag; const fr_t* rc; };      // rc [8]: lambda_q c_q, or c_q for the unscaled chain
template <int Q>
__device__ __forceinline__ void round_x(const PairState& s, const Tabs& Tb, fr_t& s0, mfma_v4i (&b)[8][2]) {
    __builtin_amdgcn_sched_barrier(0);
    const fr_t y = fr_pow5_r29<PF>(fr_add<PF>(s0, Tb.rc[Q]));   // yt_Q: canonical
    s.sto(Blk8Cfg::ymail(Q), recode_signed(y));
    __syncthreads();                                       // barrier_Q: H_Q is posted (canonical: mfma_post)
    s0 = fr_add<PF>(y, s.ld(Blk8Cfg::hmail(Q)));
    b[Q][0] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 0); b[Q][1] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 1);
}
template <int Q>
__device__ __forceinline__ void round_y(const PairState& s, const Tabs& Tb, mfma_v4i (&b)[8][2], mfma_v4i (&a)[16], mfma_v4i (&g)[7]) {
    __builtin_amdgcn_sched_barrier(0);
    const int lane = s.lane;
    mfma_v16i acc[2];
    mfma_zero_tile(acc);
#pragma unroll
    for (int e = 0; e < 16; ++e)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[e], blk8_b_of_slot(s, e + 1, ct), acc[ct], 0, 0, 0);
    if constexpr (Q > 0) {
#pragma unroll
        for (int p = 0; p < Q; ++p)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(g[p], b[p][ct], acc[ct], 0, 0, 0);
    }
    if constexpr (Q < 7) {
        blk8_load_frags16(a, Tb.efrag + (size_t)(Q + 1) * 16 * 64, lane);
#pragma unroll
        for (int p = 0; p <= Q; ++p) g[p] = (Tb.gfrag + (size_t)((Q + 1) * Q / 2 + p) * 64)[lane];
    }
    s.sto(Blk8Cfg::hmail(Q), mfma_post(acc));
    __syncthreads();                                       // barrier_Q: y_Q is posted
    b[Q][0] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 0); b[Q][1] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 1);
}
template <int NLX>
__device__ __forceinline__ void lane_rows(const PairState& s, const Tabs& Tb, const mfma_v4i (&b)[8][2], bool last) {
    const Blk8Tabs T8{Tb.efrag, Tb.lfrag, Tb.unit, Tb.gfrag, nullptr};
    blk8_lane_rows<NLX>(s, T8, b, last);
}
template <int NLX>
__device__ __forceinline__ void pair_block8(const PairState& s, const Tabs& Tb, fr_t& s0, bool last) {
    mfma_v4i b[8][2];
    if (!s.isY) {
        round_x<0>(s, Tb, s0, b); round_x<1>(s, Tb, s0, b); round_x<2>(s, Tb, s0, b); round_x<3>(s, Tb, s0, b);
        round_x<4>(s, Tb, s0, b); round_x<5>(s, Tb, s0, b); round_x<6>(s, Tb, s0, b); round_x<7>(s, Tb, s0, b);
    } else {
        mfma_v4i a[16], g[7];
        blk8_load_frags16(a, Tb.efrag, s.lane);
        round_y<0>(s, Tb, b, a, g); round_y<1>(s, Tb, b, a, g); round_y<2>(s, Tb, b, a, g); round_y<3>(s, Tb, b, a, g);
        round_y<4>(s, Tb, b, a, g); round_y<5>(s, Tb, b, a, g); round_y<6>(s, Tb, b, a, g); round_y<7>(s, Tb, b, a, g);
    }
    __builtin_amdgcn_sched_barrier(0);
    lane_rows<NLX>(s, Tb, b, last);
}
}  // namespace canonical

// ---- the product's schedule with the chain UNSCALED, kept here as the comparison: X_{q+1} = H_q + a_q y_q, the product a nine-limb unpack, 81 MACs and a wide
// reduction in every round of wave X.  Wave Y is the canonical form's, the lane rows are the product's, fed the unscaled tables.  The product no longer contains it.
namespace unscaled {
template <int Q>
__device__ __forceinline__ void round_x(const PairState& s, const canonical::Tabs& Tb, const uint32_t* a29, fr_t& s0, mfma_v4i (&b)[8][2]) {
    __builtin_amdgcn_sched_barrier(0);
    const fr_t y = fr_pow5_r29<PF>(fr_add<PF>(s0, Tb.rc[Q]));
    fr_wide29 acc; fr_wide29_zero(acc);
    fr_wide29_mac(acc, c29(a29, (size_t)Q * (2 * 17 - 1)), fr29_unpack(y));
    const fr_t part = fr_wide29_reduce<PF>(acc);
    s.sto(Blk8Cfg::ymail(Q), recode_signed(y));
    __syncthreads();                                       // barrier_Q: H_Q is posted
    s0 = fr_add<PF>(part, s.ld(Blk8Cfg::hmail(Q)));
    b[Q][0] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 0); b[Q][1] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 1);
}
template <int NLX>
__device__ __forceinline__ void pair_block8(const PairState& s, const canonical::Tabs& Tb, const uint32_t* a29, fr_t& s0, bool last) {
    mfma_v4i b[8][2];
    if (!s.isY) {
        round_x<0>(s, Tb, a29, s0, b); round_x<1>(s, Tb, a29, s0, b); round_x<2>(s, Tb, a29, s0, b); round_x<3>(s, Tb, a29, s0, b);
        round_x<4>(s, Tb, a29, s0, b); round_x<5>(s, Tb, a29, s0, b); round_x<6>(s, Tb, a29, s0, b); round_x<7>(s, Tb, a29, s0, b);
    } else {
        mfma_v4i a[16], g[7];
        blk8_load_frags16(a, Tb.efrag, s.lane);
        canonical::round_y<0>(s, Tb, b, a, g); canonical::round_y<1>(s, Tb, b, a, g); canonical::round_y<2>(s, Tb, b, a, g); canonical::round_y<3>(s, Tb, b, a, g);
        canonical::round_y<4>(s, Tb, b, a, g); canonical::round_y<5>(s, Tb, b, a, g); canonical::round_y<6>(s, Tb, b, a, g); canonical::round_y<7>(s, Tb, b, a, g);
    }
    __builtin_amdgcn_sched_barrier(0);
    canonical::lane_rows<NLX>(s, Tb, b, last);
}
}  // namespace unscaled

// ---- the canonical form with wave Y SOFTWARE-PIPELINED across the round barrier, measured here and not in the product unless it wins: of row Q only the
// K-step of y_{Q-1} depends on barrier_{Q-1}, so the 16 lane steps and the steps of y_p, p <= Q - 2, are issued before that barrier, after H_{Q-1} is
// posted (the accumulator pair is free again by then: no second pair).  Wave X and the lane product are the product's.
namespace piped {
template <int Q>
__device__ __forceinline__ void round_y(const PairState& s, const canonical::Tabs& Tb, mfma_v4i (&b)[8][2], mfma_v4i (&a)[16], mfma_v4i (&g)[7], mfma_v16i (&acc)[2]) {
    __builtin_amdgcn_sched_barrier(0);
    const int lane = s.lane;
    if constexpr (Q > 0) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(g[Q - 1], b[Q - 1][ct], acc[ct], 0, 0, 0);
    }
    if constexpr (Q < 7) {
        blk8_load_frags16(a, Tb.efrag + (size_t)(Q + 1) * 16 * 64, lane);
#pragma unroll
        for (int p = 0; p <= Q; ++p) g[p] = (Tb.gfrag + (size_t)((Q + 1) * Q / 2 + p) * 64)[lane];
    }
    s.sto(Blk8Cfg::hmail(Q), mfma_post(acc));
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (Q < 7) {                                 // row Q + 1 up to the step of y_{Q-1}
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[e], blk8_b_of_slot(s, e + 1, ct), acc[ct], 0, 0, 0);
        if constexpr (Q > 0) {
#pragma unroll
            for (int p = 0; p < Q; ++p)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(g[p], b[p][ct], acc[ct], 0, 0, 0);
        }
    }
    __syncthreads();                                       // barrier_Q: y_Q is posted
    b[Q][0] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 0); b[Q][1] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 1);
}
template <int NLX>
__device__ __forceinline__ void pair_block8(const PairState& s, const canonical::Tabs& Tb, fr_t& s0, bool last) {
    mfma_v4i b[8][2];
    if (!s.isY) {
        canonical::round_x<0>(s, Tb, s0, b); canonical::round_x<1>(s, Tb, s0, b); canonical::round_x<2>(s, Tb, s0, b); canonical::round_x<3>(s, Tb, s0, b);
        canonical::round_x<4>(s, Tb, s0, b); canonical::round_x<5>(s, Tb, s0, b); canonical::round_x<6>(s, Tb, s0, b); canonical::round_x<7>(s, Tb, s0, b);
    } else {
        mfma_v4i a[16], g[7]; mfma_v16i acc[2];
        blk8_load_frags16(a, Tb.efrag, s.lane);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[e], blk8_b_of_slot(s, e + 1, ct), acc[ct], 0, 0, 0);
        round_y<0>(s, Tb, b, a, g, acc); round_y<1>(s, Tb, b, a, g, acc); round_y<2>(s, Tb, b, a, g, acc); round_y<3>(s, Tb, b, a, g, acc);
        round_y<4>(s, Tb, b, a, g, acc); round_y<5>(s, Tb, b, a, g, acc); round_y<6>(s, Tb, b, a, g, acc); round_y<7>(s, Tb, b, a, g, acc);
    }
    __builtin_amdgcn_sched_barrier(0);
    canonical::lane_rows<NLX>(s, Tb, b, last);
}
}  // namespace piped

// ---- the lanes between two blocks finished through NINE 29-BIT LIMBS, kept here as the comparison: exchange of all 32 sums (16 swaps), fold into nine
// columns, carry pass, floor quotient, pack and recode (mfma_finish_recoded).  The rounds are the product's.  The product no longer runs it on the device.
namespace limbfinish {
template <int NLX>
__device__ __forceinline__ void lane_rows(const PairState& s, const Blk8Tabs& Tb, const mfma_v4i (&b)[8][2]) {
    const int lane = s.lane;
    const int j0 = s.isY ? NLX + 1 : 1, j1 = s.isY ? 16 : NLX;
    const mfma_v4i aunit = Tb.unit[lane];
    mfma_v4i a[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) a[p] = (Tb.lfrag + ((size_t)(j0 - 1) * 8 + p) * 64)[lane];
#pragma unroll 1
    for (int j = j0; j <= j1; ++j) {
        mfma_v16i acc[2];
        mfma_zero_tile(acc);
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[p], b[p][ct], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aunit, blk8_b_of_slot(s, j, ct), acc[ct], 0, 0, 0);
        const int jn = j < j1 ? j + 1 : j1;                // the last row fetches its own fragments again: in bounds, unused
#pragma unroll
        for (int p = 0; p < 8; ++p) a[p] = (Tb.lfrag + ((size_t)(jn - 1) * 8 + p) * 64)[lane];
        int64_t col[9]; mfma_post_cols(acc, col); s.sto(j, mfma_finish_recoded(col));      // slot j is read by this wave alone, before this write
    }
    __syncthreads();
}
template <int NLX>
__device__ __forceinline__ void pair_block8(const PairState& s, const Blk8Tabs& Tb, fr29_t& u) {
    mfma_v4i b[8][2];
    if (!s.isY) {
        blk8_round_x<0>(s, Tb, u, b); blk8_round_x<1>(s, Tb, u, b); blk8_round_x<2>(s, Tb, u, b); blk8_round_x<3>(s, Tb, u, b);
        blk8_round_x<4>(s, Tb, u, b); blk8_round_x<5>(s, Tb, u, b); blk8_round_x<6>(s, Tb, u, b); blk8_round_x<7>(s, Tb, u, b);
    } else {
        mfma_v4i a[16], g[7];
        blk8_load_frags16(a, Tb.efrag, s.lane);
        blk8_round_y<0>(s, Tb, b, a, g); blk8_round_y<1>(s, Tb, b, a, g); blk8_round_y<2>(s, Tb, b, a, g); blk8_round_y<3>(s, Tb, b, a, g);
        blk8_round_y<4>(s, Tb, b, a, g); blk8_round_y<5>(s, Tb, b, a, g); blk8_round_y<6>(s, Tb, b, a, g); blk8_round_y<7>(s, Tb, b, a, g);
    }
    __builtin_amdgcn_sched_barrier(0);
    lane_rows<NLX>(s, Tb, b);
}
}  // namespace limbfinish

// ---- the rows that end as nine limbs finished through NINE 29-BIT COLUMNS, kept here as the comparison: wave Y's H_q rows and the last block's fused lane rows
// by the exchange of all 32 sums (16 swaps), zeroed columns, mfma_fold_rows, the constant's limbs into the columns, carry pass and mfma_finish_limbs (the
// product's form until the word-column finish, mfma_post_limbs).  Wave X's rounds and the lane rows between two blocks are the product's.
namespace limbrows {
template <int Q>
__device__ __forceinline__ void blk8_round_y(const PairState& s, const Blk8Tabs& Tb, mfma_v4i (&b)[8][2], mfma_v4i (&a)[16], mfma_v4i (&g)[7]) {
    __builtin_amdgcn_sched_barrier(0);
    const int lane = s.lane;
    mfma_v16i acc[2];
    mfma_zero_tile(acc);
#pragma unroll
    for (int e = 0; e < 16; ++e)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[e], blk8_b_of_slot(s, e + 1, ct), acc[ct], 0, 0, 0);
    if constexpr (Q > 0) {
#pragma unroll
        for (int p = 0; p < Q; ++p)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(g[p], b[p][ct], acc[ct], 0, 0, 0);
    }
    if constexpr (Q < 7) {
        blk8_load_frags16(a, Tb.efrag + (size_t)(Q + 1) * 16 * 64, lane);
#pragma unroll
        for (int p = 0; p <= Q; ++p) g[p] = (Tb.gfrag + (size_t)((Q + 1) * Q / 2 + p) * 64)[lane];
    }
    { int64_t col[9]; uint32_t l[9]; mfma_post_cols(acc, col); { int64_t cc[9]; mfma_cols_set(cc, c29(Tb.rc29, Q)); _Pragma("unroll") for (int k = 0; k < 9; ++k) col[k] += cc[k]; } mfma_finish_limbs(col, l); s.sto(Blk8Cfg::hmail(Q), lazy29_to_slot(l)); }
    __syncthreads();                                       // barrier_Q: y_Q is posted
    b[Q][0] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 0); b[Q][1] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 1);
}
// a slot as the shipped hand-over leaves it (recode_lazy29: the signed digits of an unreduced S-box output below 1.04 r) -> the canonical value, for the comparison
__device__ __forceinline__ fr_t unrecode_reduce(const fr_t& y) {
    fr_t x; int64_t b = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int64_t t = (int64_t)(y.v[i] ^ 0x80808080u) - (int64_t)0x80808080u + b; x.v[i] = (uint32_t)t; b = t >> 32; }
    fr_cond_sub<PF>(x.v, 0u);
    return x;
}
// the hand-over with the canonical store this comparison form measures (the shipped pair_sto_sbox29 always recodes: the squeeze row runs on the matrix cores now)
__device__ __forceinline__ void proto_sto_sbox29(const PairState& s, int j, const uint32_t* l, const uint32_t* rc29, bool recode) {
    const fr29_t x5 = pow5_lazy29(lazy29_add_c29(l, rc29));
    s.sto(j, recode ? recode_lazy29(x5) : fr29_pack_reduce<PF>(x5.l));
}
template <int NLX>
__device__ __forceinline__ void lane_rows_fused(const PairState& s, const Blk8Tabs& Tb, const mfma_v4i (&b)[8][2], const uint32_t* rc29_next, bool recode_next) {
    const int lane = s.lane;
    const int j0 = s.isY ? NLX + 1 : 1, j1 = s.isY ? 16 : NLX;
    const mfma_v4i aunit = Tb.unit[lane];
    mfma_v4i a[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) a[p] = (Tb.lfrag + ((size_t)(j0 - 1) * 8 + p) * 64)[lane];
#pragma unroll 1
    for (int j = j0; j <= j1; ++j) {
        mfma_v16i acc[2];
        mfma_zero_tile(acc);
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[p], b[p][ct], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aunit, blk8_b_of_slot(s, j, ct), acc[ct], 0, 0, 0);
        const int jn = j < j1 ? j + 1 : j1;                // the last row fetches its own fragments again: in bounds, unused
#pragma unroll
        for (int p = 0; p < 8; ++p) a[p] = (Tb.lfrag + ((size_t)(jn - 1) * 8 + p) * 64)[lane];
        { int64_t col[9]; uint32_t l[9]; mfma_post_cols(acc, col); mfma_finish_limbs(col, l); proto_sto_sbox29(s, j, l, c29(rc29_next, j), recode_next); }
    }
    __syncthreads();
}
// rc29_next == nullptr: a block between two blocks (the product's lane rows, byte-domain finish); else the permutation's last block, fused with the next S-box
template <int NLX>
__device__ __forceinline__ void pair_block8(const PairState& s, const Blk8Tabs& Tb, fr29_t& u, const uint32_t* rc29_next, const uint32_t* unscale29) {
    mfma_v4i b[8][2];
    if (!s.isY) {
        blk8_round_x<0>(s, Tb, u, b); blk8_round_x<1>(s, Tb, u, b); blk8_round_x<2>(s, Tb, u, b); blk8_round_x<3>(s, Tb, u, b);
        blk8_round_x<4>(s, Tb, u, b); blk8_round_x<5>(s, Tb, u, b); blk8_round_x<6>(s, Tb, u, b); blk8_round_x<7>(s, Tb, u, b);
    } else {
        mfma_v4i a[16], g[7];
        blk8_load_frags16(a, Tb.efrag, s.lane);
        limbrows::blk8_round_y<0>(s, Tb, b, a, g); limbrows::blk8_round_y<1>(s, Tb, b, a, g); limbrows::blk8_round_y<2>(s, Tb, b, a, g); limbrows::blk8_round_y<3>(s, Tb, b, a, g);
        limbrows::blk8_round_y<4>(s, Tb, b, a, g); limbrows::blk8_round_y<5>(s, Tb, b, a, g); limbrows::blk8_round_y<6>(s, Tb, b, a, g); limbrows::blk8_round_y<7>(s, Tb, b, a, g);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (rc29_next) {
        if (!s.isY) { const fr29_t x = fr29_mul_c29(unscale29, u); proto_sto_sbox29(s, 0, x.l, c29(rc29_next, 0), false); }
        lane_rows_fused<NLX>(s, Tb, b, rc29_next, false);
    } else blk8_lane_rows<NLX, true>(s, Tb, b, false);
}
}  // namespace limbrows

// The tables of "block rep & blkmask" (always block 0): as in a permutation's loop over its blocks the fragment addresses change from one pass to the
// next, so the compiler cannot hoist all of them out of the repetition loop (it did, and spilled 200 registers for them).
// efrag / lfrag / gfrag / rc: the unscaled family (blk8_*, rc_partial); sefrag / slfrag / sgfrag / src: the scaled one (blk8s_*, rc_partial_scaled);
// unscale8: 1 / lambda_8 as a multiplier-table entry (block 0 ends at round 8; the product's table holds 1 / lambda_rp);
// zero29: 17 x 9 zero limbs, the constants of the S-box that follows a block run as a permutation's last;
// src29: lambda_q c_q of rounds 0..7 as nine limbs each and a ninth entry of zeros (the block is followed by no round here: rc_partial_scaled29 of an rp = 8 set)
struct ProtoTabs { const mfma_v4i* efrag; const mfma_v4i* lfrag; const mfma_v4i* unit; const mfma_v4i* gfrag; const uint32_t* sparse29; const uint32_t* gamma8_29; const fr_t* rc;
                   const mfma_v4i* sefrag; const mfma_v4i* slfrag; const mfma_v4i* sgfrag; const fr_t* src; const uint32_t* src29; const uint32_t* unscale8; const uint32_t* zero29; int blkmask; };

template <int YG, int NLX>                                 // YG > 0: the former form with these shares; YG = 0: the product's pair_block8<NLX>; YG = -1: piped::pair_block8<NLX>; YG = -2: unscaled::pair_block8<NLX>; YG = -3: canonical::pair_block8<NLX>; YG = -4 / -5: a block between two blocks (lanes left as signed digits), limbfinish::pair_block8<NLX> / the product's pair_block8<NLX, true> with last = false; YG = -6: the same with the H_q rows through nine limb columns (limbrows); YG = -7 / -8: the block as a permutation's LAST, every slot ending as fr_pow5_r29 of its element (the next S-box with zero constants, not recoded), limbrows / the product
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) k_block8(ProtoTabs Tp, const fr_t* __restrict__ X, fr_t* __restrict__ Y, int reps) {
    extern __shared__ uint4 lds[];
    PairState s = pair_setup(lds);
    const size_t b0 = (size_t)blockIdx.x * T * 64;
    for (int rep = 0; rep < reps; ++rep) {
        fr_t s0 = fr_zero<PF>();
        if (!s.isY) s0 = ldg(X + b0 + s.lane);
        for (int j = s.isY ? 9 : 1; j <= (s.isY ? 16 : 8); ++j) s.sto(j, recode_signed(ldg(X + b0 + (size_t)j * 64 + s.lane)));
        __syncthreads();
        const int blk = rep & Tp.blkmask;
        if constexpr (YG > 0) {
            const former::Tabs Tb{Tp.efrag + (size_t)blk * 8 * 16 * 64, Tp.lfrag + (size_t)blk * 16 * 8 * 64, Tp.unit, Tp.sparse29, Tp.gamma8_29, Tp.rc};
            former::pair_block8<YG, NLX>(s, Tb, s0, true);  // last: the lanes end canonical in their slots
        } else if constexpr (YG == -2) {
            const canonical::Tabs Tb{Tp.efrag + (size_t)blk * 8 * 16 * 64, Tp.lfrag + (size_t)blk * 16 * 8 * 64, Tp.unit, Tp.gfrag + (size_t)blk * 28 * 64, Tp.rc};
            unscaled::pair_block8<NLX>(s, Tb, Tp.sparse29, s0, true);
        } else if constexpr (YG == 0) {
            const Blk8Tabs Tb{Tp.sefrag + (size_t)blk * 8 * 16 * 64, Tp.slfrag + (size_t)blk * 16 * 8 * 64, Tp.unit, Tp.sgfrag + (size_t)blk * 28 * 64, c29(Tp.src29, 1)};
            fr29_t u = fr29_unpack(s0);
            if (!s.isY) u = lazy29_add_c29(u.l, c29(Tp.src29, 0));          // as pair_permute enters the partial rounds
            pair_block8<NLX>(s, Tb, u, true);
            if (rep == 0 && !s.isY) s0 = fr29_pack_reduce<PF>(fr29_mul_c29(Tp.unscale8, u).l);      // lambda_8 X_8 (lazy) -> X_8
        } else if constexpr (YG == -4 || YG == -5) {
            const Blk8Tabs Tb{Tp.sefrag + (size_t)blk * 8 * 16 * 64, Tp.slfrag + (size_t)blk * 16 * 8 * 64, Tp.unit, Tp.sgfrag + (size_t)blk * 28 * 64, c29(Tp.src29, 1)};
            fr29_t u = fr29_unpack(s0);
            if (!s.isY) u = lazy29_add_c29(u.l, c29(Tp.src29, 0));
            if constexpr (YG == -5) pair_block8<NLX, true>(s, Tb, u, false); else limbfinish::pair_block8<NLX>(s, Tb, u);
            if (rep == 0 && !s.isY) s0 = fr29_pack_reduce<PF>(fr29_mul_c29(Tp.unscale8, u).l);
        } else if constexpr (YG == -6 || YG == -7 || YG == -8) {
            const Blk8Tabs Tb{Tp.sefrag + (size_t)blk * 8 * 16 * 64, Tp.slfrag + (size_t)blk * 16 * 8 * 64, Tp.unit, Tp.sgfrag + (size_t)blk * 28 * 64, c29(Tp.src29, 1)};
            fr29_t u = fr29_unpack(s0);
            if (!s.isY) u = lazy29_add_c29(u.l, c29(Tp.src29, 0));
            if constexpr (YG == -8) {
                pair_block8<NLX, true>(s, Tb, u, true, Tp.zero29, Tp.unscale8);
                if (rep == 0) for (int j = s.isY ? 9 : 0; j <= (s.isY ? 16 : 8); ++j) s.sto(j, limbrows::unrecode_reduce(s.ld(j)));      // each wave its own slots, read back by itself below
            } else limbrows::pair_block8<NLX>(s, Tb, u, YG == -7 ? Tp.zero29 : nullptr, Tp.unscale8);
            if constexpr (YG == -6) { if (rep == 0 && !s.isY) s0 = fr29_pack_reduce<PF>(fr29_mul_c29(Tp.unscale8, u).l); }
            else if (rep == 0 && !s.isY) s0 = s.ld(0);          // the closing barrier of the lane rows published slot 0
        } else {
            const canonical::Tabs Tb{Tp.sefrag + (size_t)blk * 8 * 16 * 64, Tp.slfrag + (size_t)blk * 16 * 8 * 64, Tp.unit, Tp.sgfrag + (size_t)blk * 28 * 64, Tp.src};
            if constexpr (YG == -3) canonical::pair_block8<NLX>(s, Tb, s0, true); else piped::pair_block8<NLX>(s, Tb, s0, true);
            if (rep == 0 && !s.isY) s0 = fr_mul_c29(Tp.unscale8, s0);      // lambda_8 X_8 -> X_8
        }
        if (rep == 0) {
            if (!s.isY) stg(Y + b0 + s.lane, s0);
            for (int j = s.isY ? 9 : 1; j <= (s.isY ? 16 : 8); ++j) stg(Y + b0 + (size_t)j * 64 + s.lane, s.ld(j));
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) k_block4x2(PoseidonDev P, const fr_t* __restrict__ X, fr_t* __restrict__ Y, int reps) {
    extern __shared__ uint4 lds[];
    PairState s = pair_setup(lds);
    const size_t b0 = (size_t)blockIdx.x * T * 64;
    for (int rep = 0; rep < reps; ++rep) {
        for (int j = s.isY ? 9 : 0; j <= (s.isY ? 16 : 8); ++j) s.sto(j, ldg(X + b0 + (size_t)j * 64 + s.lane));
        __syncthreads();
        pair_permute<17>(s, P, false);                 // rf = 0, rp = 8: two blocks of 4 partial rounds, ends with a barrier
        if (rep == 0) for (int j = s.isY ? 9 : 0; j <= (s.isY ? 16 : 8); ++j) stg(Y + b0 + (size_t)j * 64 + s.lane, s.ld(j));
        __syncthreads();
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------
static fr_t canon(fr_t x) { for (int k = 0; k < 3; ++k) fr_cond_sub<host::PF>(x.v, 0u); return x; }   // form 4 leaves its lanes below 2.7 r (pair_lane_update)
template <class Tp> static Tp* to_dev(const void* p, size_t bytes) { void* d = nullptr; if (hipMalloc(&d, bytes) != hipSuccess || hipMemcpy(d, p, bytes, hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "device copy failed\n"); exit(1); } return (Tp*)d; }

struct Form { const char* name; void (*launch)(int batches, int reps); bool digits = false; bool sbox = false; };      // digits: lanes 1..16 come back as signed digits of a residue; sbox: every element comes back as fr_pow5_r29 of its value
// 32 signed digits -> the canonical value of sum_b d_b 256^b mod r, through the field code
static fr_t of_digits(const fr_t& d) {
    const int8_t* b = reinterpret_cast<const int8_t*>(d.v);
    fr_t acc = host::h_zero(), w = host::h_one(); const fr_t k256 = fr_from_u64<host::PF>(256);
    for (int c = 0; c < 32; ++c, w = host::h_mul(w, k256)) {
        const fr_t term = host::h_mul(fr_from_u64<host::PF>((uint64_t)(b[c] < 0 ? -(int)b[c] : (int)b[c])), w);
        acc = b[c] < 0 ? host::h_sub(acc, term) : host::h_add(acc, term);
    }
    return fr_to_canonical<host::PF>(acc);
}
static ProtoTabs g_tb; static PoseidonDev g_p; static const fr_t* g_x; static fr_t* g_y;
template <int YG, int NLX> static void launch8(int batches, int reps) { hipLaunchKernelGGL((k_block8<YG, NLX>), dim3(batches), dim3(128), PairCfg<17>::lds_bytes(), 0, g_tb, g_x, g_y, reps); }
static void launch4(int batches, int reps) { hipLaunchKernelGGL(k_block4x2, dim3(batches), dim3(128), PairCfg<17>::lds_bytes(), 0, g_p, g_x, g_y, reps); }

int main() {
    hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
    const int cus = prop.multiProcessorCount;
    const host::KernelConsts K = host::make_kernel_consts(host::consts_for_width(T));
    if (!K.ok) { fprintf(stderr, "constants failed\n"); return 1; }
    // the product's tables (host_util.hpp blk8_*); block 0 = rounds 0..7
    if (K.blk8_efrag.empty()) { fprintf(stderr, "no block-8 tables\n"); return 1; }
    g_tb.efrag = to_dev<mfma_v4i>(K.blk8_efrag.data(), K.blk8_efrag.size()); g_tb.lfrag = to_dev<mfma_v4i>(K.blk8_lfrag.data(), K.blk8_lfrag.size());
    g_tb.unit = g_tb.lfrag + (K.blk8_lfrag.size() - 1024) / 16; g_tb.gfrag = to_dev<mfma_v4i>(K.blk8_gfrag.data(), K.blk8_gfrag.size());
    g_tb.sparse29 = to_dev<uint32_t>(K.sparse29.data(), K.sparse29.size() * 4); g_tb.gamma8_29 = to_dev<uint32_t>(K.gamma8_29.data(), K.gamma8_29.size() * 4);
    g_tb.sefrag = to_dev<mfma_v4i>(K.blk8s_efrag.data(), K.blk8s_efrag.size()); g_tb.slfrag = to_dev<mfma_v4i>(K.blk8s_lfrag.data(), K.blk8s_lfrag.size());
    g_tb.sgfrag = to_dev<mfma_v4i>(K.blk8s_gfrag.data(), K.blk8s_gfrag.size()); g_tb.src = to_dev<fr_t>(K.rc_partial_scaled.data(), K.rc_partial_scaled.size() * sizeof(fr_t));
    { std::vector<uint32_t> c29v(K.rc_partial_scaled29.begin(), K.rc_partial_scaled29.begin() + 9 * 9); for (int i = 0; i < 9; ++i) c29v[72 + i] = 0; g_tb.src29 = to_dev<uint32_t>(c29v.data(), c29v.size() * 4); }
    { uint32_t u8[9]; fr29_const_from<host::PF>(fr_inv<host::PF>(K.blk8_lambda[8]), u8); g_tb.unscale8 = to_dev<uint32_t>(u8, sizeof u8); }
    { const std::vector<uint32_t> z(17 * 9, 0u); g_tb.zero29 = to_dev<uint32_t>(z.data(), z.size() * 4); }
    g_tb.blkmask = 0;
    g_tb.rc = to_dev<fr_t>(K.rc_partial.data(), K.rc_partial.size() * sizeof(fr_t));
    memset(&g_p, 0, sizeof g_p);
    g_p.t = T; g_p.rf = 0; g_p.rp = 8; g_p.rc_partial = g_tb.rc; g_p.sparse29 = g_tb.sparse29; g_p.gamma29 = to_dev<uint32_t>(K.gamma29.data(), K.gamma29.size() * 4);

    const int batches = cus * 8;
    uint64_t sd = 0x243f6a8885a308d3ull; auto rnd = [&]() { sd ^= sd << 13; sd ^= sd >> 7; sd ^= sd << 17; return (uint32_t)(sd >> 16); };
    std::vector<fr_t> X((size_t)batches * T * 64);
    for (auto& x : X) { for (int i = 0; i < 8; ++i) x.v[i] = rnd(); x.v[7] &= 0x3fffffffu; }
    for (int e = 0; e < T; ++e) {                       // sponge 3 of batch 0: every element r - 1; sponge 5: every element 0; sponge 7: alternating
        fr_t rm1; for (int i = 0; i < 8; ++i) rm1.v[i] = host::PF::P(i); rm1.v[0] -= 1;
        X[(size_t)e * 64 + 3] = rm1; X[(size_t)e * 64 + 5] = host::h_zero(); X[(size_t)e * 64 + 7] = (e & 1) ? rm1 : host::h_zero();
    }
    g_x = to_dev<fr_t>(X.data(), X.size() * sizeof(fr_t));
    if (hipMalloc((void**)&g_y, X.size() * sizeof(fr_t)) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }

    const Form forms[] = {
        {"block4 x 2 (shipped pair_permute<17>, rf = 0, rp = 8)", launch4},
        {"block8, Gamma terms on the vector ALU, YG=5 NLX=8 (the former product form)", launch8<5, 8>},
        {"block8, Gamma K-steps, chain unscaled (a_q y_q product per round), NLX=8 (the former product form)", launch8<-2, 8>},
        {"block8, Gamma K-steps, chain scaled, canonical value in every round, NLX=8 (the former product form)", launch8<-3, 8>},
        {"block8, Gamma K-steps, chain scaled, lazy residues, NLX=8", launch8<0, 8>},
        {"block8, Gamma K-steps, chain scaled, canonical, NLX=8, wave Y pipelined across the round barrier", launch8<-1, 8>},
        {"block8, Gamma K-steps, chain scaled, lazy residues, NLX=7", launch8<0, 7>},
        {"block8, Gamma K-steps, chain scaled, lazy residues, NLX=9", launch8<0, 9>},
        {"block8 between two blocks, lanes as signed digits through nine 29-bit limbs, NLX=8 (the former product form)", launch8<-4, 8>, true},
        {"block8 between two blocks, byte-domain lanes, H rows through nine limb columns, NLX=8 (the former product form)", launch8<-6, 8>, true},
        {"block8 between two blocks, byte-domain lanes, H rows from word columns, NLX=8", launch8<-5, 8>, true},
        {"block8 as the last block, fused with the next S-box, H and lane rows through nine limb columns, NLX=8 (the former product form)", launch8<-7, 8>, false, true},
        {"block8 as the last block, fused with the next S-box, H and lane rows from word columns, NLX=8", launch8<-8, 8>, false, true},
    };
    const int nforms = (int)(sizeof forms / sizeof forms[0]);
    // reference: the sparse rounds in the portable field code, sampled batches
    std::vector<int> sample; for (int bt = 0; bt < batches; bt += 97) sample.push_back(bt);
    std::vector<fr_t> ref(sample.size() * T * 64);
    for (size_t si = 0; si < sample.size(); ++si) for (int n = 0; n < 64; ++n) {
        fr_t st[T]; for (int e = 0; e < T; ++e) st[e] = X[((size_t)sample[si] * T + e) * 64 + n];
        for (int q = 0; q < B8; ++q) {
            const fr_t* sp = &K.sparse[(size_t)q * W];
            const fr_t y = fr_pow5<host::PF>(host::h_add(st[0], K.rc_partial[q]));
            fr_t n0 = host::h_mul(sp[0], y);
            for (int j = 1; j < T; ++j) n0 = host::h_add(n0, host::h_mul(sp[j], st[j]));
            for (int j = 1; j < T; ++j) st[j] = host::h_add(st[j], host::h_mul(sp[T - 1 + j], y));
            st[0] = n0;
        }
        for (int e = 0; e < T; ++e) ref[(si * T + e) * 64 + n] = canon(st[e]);
    }
    std::vector<fr_t> Y(X.size());
    for (int f = 0; f < nforms; ++f) {
        if (hipMemset(g_y, 0xff, Y.size() * sizeof(fr_t)) != hipSuccess) return 1;
        forms[f].launch(batches, 1);
        if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed: %s\n", forms[f].name); return 1; }
        if (hipMemcpy(Y.data(), g_y, Y.size() * sizeof(fr_t), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        long bad = 0;
        for (size_t si = 0; si < sample.size(); ++si) for (int n = 0; n < 64; ++n) for (int e = 0; e < T; ++e)
            if (!fr_eq(forms[f].sbox ? fr_pow5_r29<host::PF>(ref[(si * T + e) * 64 + n]) : ref[(si * T + e) * 64 + n], (forms[f].digits && e > 0) ? of_digits(Y[((size_t)sample[si] * T + e) * 64 + n]) : canon(Y[((size_t)sample[si] * T + e) * 64 + n]))) { if (bad < 5) fprintf(stderr, "%s: mismatch batch %d sponge %d element %d\n", forms[f].name, sample[si], n, e); ++bad; }
        printf("{\"check\": \"8 partial rounds of 64 sponges against the sparse rounds in the portable field code, sampled batches, incl. states of 0 and r-1\", \"form\": \"%s\", \"mismatches\": %ld}\n", forms[f].name, bad);
        if (bad) return 1;
    }
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int reps = 128, rounds = 8;
    std::vector<std::vector<double>> cyc(nforms);
    for (int r = 0; r < rounds; ++r)
        for (int f = 0; f < nforms; ++f) {
            (void)hipEventRecord(e0); forms[f].launch(batches, reps); (void)hipEventRecord(e1);
            if (hipEventSynchronize(e1) != hipSuccess) { fprintf(stderr, "kernel failed: %s\n", forms[f].name); return 1; }
            float ms; (void)hipEventElapsedTime(&ms, e0, e1);
            cyc[f].push_back(ms * 1e-3 * 2.4e9 * cus * 4 / ((double)batches * reps));
        }
    for (int f = 0; f < nforms; ++f) {
        std::vector<double> v(cyc[f].begin() + 1, cyc[f].end());     // the first pass warms the tables
        std::sort(v.begin(), v.end());
        printf("{\"form\": \"%s\", \"simd_cycles_per_8_rounds_at_2.4GHz\": {\"median\": %.0f, \"min\": %.0f, \"max\": %.0f}, \"runs\": %d, \"workgroups\": %d, \"reps\": %d}\n",
               forms[f].name, v[v.size() / 2], v.front(), v.back(), (int)v.size(), batches, reps);
    }
    return 0;
}
