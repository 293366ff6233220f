// stark_mlwe_amd/csrc/poseidon_pair.hpp — Poseidon sponges with TWO waves per batch of 64 states (gfx950).
//
// Why: one lane per sponge with the state in LDS (poseidon_dev.hpp) is capped by LDS capacity at
// 160 KiB / (t*32 B) = 301 states per CU for t = 17, i.e. ONE wave per SIMD, and a lone wave issues a
// VALU instruction only every ~5 cycles (measured: v_mad_u64_u32 11.0 vs 5.4 cycles/instr at 1 vs 2
// waves per SIMD).  Here a workgroup is a pair of waves (X, Y) that share the 64 LDS-resident states of
// the batch: lane l of both waves works on state l, each wave on its own part of the linear algebra.
// Same LDS per state, twice the waves per SIMD (4 workgroups of 40 KiB per CU for t = 17).
// Results are the same field values as poseidon_dev.hpp / the reference's dense rounds.
//
// The file by layer; each permutation can be read from its entry down without the other two:
//   state and config   PairCfg, PairState, pair_setup;
//   full rounds        S-box on the wave's own elements (pair_sbox_full); the dense product for t = 9 as in-place L*(U*x) on the VALU (pair_apply_lu), for t = 17 on
//                      the MATRIX CORES through the row pipeline: zeroed tile -> int8 MFMAs of a residue table with the operands' signed radix-256 digits -> fold,
//                      exchange -> a named row end (RowEnd of pair_mds_sbox_mfma, LaneEnd of blk8_lane_rows);
//   8-round block      t = 17 partial rounds whose u-rows and lane updates are two matrix-core products (pair_block8), wave X's S-box chain scaled and lazy;
//   block of 4         partial rounds on the vector ALU (pair_blocks4; permute_core in poseidon_dev.hpp has the algebra);
//   the permutations   three entries over shared stages (pair_first_rounds, pair_blocks4, pair_blocks8, pair_last_rounds):
//       pair_permute_blk4<T>        full rounds with canonical ends, partial rounds in blocks of 4: t = 9, and t = 17 with the context option poseidon_block8 off;
//       pair_permute_blk8           t = 17: the same full rounds, 8-round blocks with canonical hand-overs at both ends of the partial rounds (k_hash_ds2);
//       pair_permute_fused<SBOXED>  t = 17: 8-round blocks, every row handed on in limb, byte or entry form (k_leaf_pair2, k_node16_pair);
//   kernels            k_leaf_pair2, k_hash_ds2, k_node16_pair.
#pragma once
#include "fr.hpp"
#include "dev_common.hpp"
#include "poseidon_params.hpp"
#include "poseidon_dev.hpp"
#include "poseidon_streams.hpp"
#include "mfma_digits.hpp"

#if defined(__HIPCC__)
namespace stark {

template <int T> struct PairCfg {
#ifndef STARK_NXD17
#define STARK_NXD17 5
#endif
    // X's share of the lanes in the per-round dot products: lanes 1..NXD, Y the other T - 1 - NXD.  Between two barriers X runs the S-box (three products),
    // a_q x_q, up to three gamma terms and its NXD lane terms, Y its lane terms: NXD = 5 balances the two for t = 17 (measured, 2^22 leaves: 61.0 ms at 3,
    // 60.2 at 4, 59.3 at 5, 60.5 at 6; a share that shrinks with the round as X's gamma terms grow — 6,5,5,4 / 6,6,5,4 / 7,6,5,4 — 61.4 / 61.2 / 60.7);
    // from eight terms on X's sum takes one carry pass in between (rounds 2 and 3 of a block).
    static constexpr int NXD = T == 17 ? STARK_NXD17 : 2;
#ifndef STARK_NXU17
#define STARK_NXU17 8
#endif
    static constexpr int NXU = T == 17 ? STARK_NXU17 : (T - 1) / 2;   // X updates lanes 1..NXU, Y lanes NXU+1..T-1
    static constexpr int NX = (T - 1) / 2;             // full rounds: X owns elements 0..NX-1 (S-box, absorb), Y the rest
    static constexpr int EXTRA = 3;                    // slots beyond the state: x mailboxes 1..3
    __host__ __device__ static constexpr int xslot(int p) { return p == 0 ? 0 : T + (p - 1); }
    // Dy mailboxes alias the state slots X preloaded (1..NXD), reused round-robin: Dy_q is read before barrier_{q+1},
    // Dy_{q+NXD} is written after barrier_{q+NXD-1} >= barrier_{q+1}
    __host__ __device__ static constexpr int dslot(int q) { return 1 + (q % NXD); }
    __host__ __device__ static constexpr size_t lds_bytes() { return (size_t)(T + EXTRA) * 2 * 64 * 16; }
};
static inline size_t pair_lds_bytes(int t) { return t == 17 ? PairCfg<17>::lds_bytes() : PairCfg<9>::lds_bytes(); }

struct PairState {
    uint4* st;      // [T + EXTRA][2][64]
    int lane; bool isY;
    __device__ __forceinline__ fr_t ld(int j) const {
        uint4 lo = st[(2 * j) * 64 + lane], hi = st[(2 * j + 1) * 64 + lane];
        fr_t x; x.v[0] = lo.x; x.v[1] = lo.y; x.v[2] = lo.z; x.v[3] = lo.w; x.v[4] = hi.x; x.v[5] = hi.y; x.v[6] = hi.z; x.v[7] = hi.w; return x;
    }
    __device__ __forceinline__ void sto(int j, const fr_t& x) const {
        st[(2 * j) * 64 + lane] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
        st[(2 * j + 1) * 64 + lane] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
    }
};
__device__ __forceinline__ PairState pair_setup(uint4* lds) {
    PairState s; s.st = lds; s.lane = threadIdx.x & 63;
    s.isY = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) != 0;      // wave-uniform by construction: tell the compiler (scalar branches, scalar constant loads)
    return s;
}

// ---- full rounds: the S-box pass and the dense product on the VALU (t = 9) ------------------------------------------------------------------------
// In-place y = L*(U*x) over the shared state, X taking the even rows and Y the odd rows of each step (rows 2k / 2k + 1 read only slots >= 2k, so a single barrier
// between the step's reads and its two writes keeps it race-free); one barrier per step.  Ends with the state consistent.
template <int T>
__device__ __forceinline__ void pair_apply_lu(const PairState& s, const uint32_t* lu) {
    const int yo = s.isY ? 1 : 0;
#pragma unroll 1
    for (int k = 0; 2 * k < T; ++k) {                       // U, top-down: rows 2k (X) and 2k+1 (Y)
        const int i = 2 * k + yo; const bool have = i < T;
        fr_t res;
        if (have) { DotAcc w; w.init(); _Pragma("unroll 1") for (int j = i; j < T; ++j) w.mac(c29(lu, i * T + j), s.ld(j)); res = w.finish(); }
        __syncthreads();
        if (have) s.sto(i, res);
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; T - 1 - 2 * k >= 1; ++k) {              // unit-lower L, bottom-up: rows T-1-2k (X) and T-2-2k (Y)
        const int i = T - 1 - 2 * k - yo; const bool have = i >= 1;
        fr_t res;
        if (have) { DotAcc w; w.init(); _Pragma("unroll 1") for (int j = 0; j < i; ++j) w.mac(c29(lu, i * T + j), s.ld(j)); res = fr_add<PF>(s.ld(i), w.finish()); }
        __syncthreads();
        if (have) s.sto(i, res);
    }
    __syncthreads();
}
// The standalone S-box pass of a full round, each wave on its own elements.  t = 17 stores the outputs RECODED: the matrix-core product reads them as operands.
template <int T>
__device__ __forceinline__ void pair_sbox_full(const PairState& s, const fr_t* rc) {
    const int j0 = s.isY ? PairCfg<T>::NX : 0, j1 = s.isY ? T : PairCfg<T>::NX;
    for (int j = j0; j < j1; ++j) { const fr_t x = fr_pow5_r29<PF>(fr_add<PF>(s.ld(j), rc[j])); s.sto(j, T == 17 ? recode_signed(x) : x); }
    __syncthreads();
}

// ---- the row pipeline: the dense full-round product on the matrix cores (T = 17) ---------------------------------------------------------------------
// y = M * x for the 64 sponges of the pair, x = the S-box outputs, stored RECODED (signed digits) in the state slots.  The left factor is the
// RESIDUE TABLE of the matrix (host_util.hpp mfma_frags): for every entry (i, e) and input digit position b the 32 signed radix-256 digits of
// C[i][e][b] = (M[i][e] * 2^20 * 256^b) mod r.  The digit sums S[(i,c)][n] = sum_{e,b} d_{i,e,b}[c] * xd_e[n][b], c = 0..31, are one dense int8
// matrix product (K = 17 * 32, no structural zeros), and V = sum_c S[c] 256^c is congruent to the stored form of (M x)_i: no Montgomery step,
// no 512-bit intermediate — only the bits of V above 2^254 are reduced, without a product (r = 2^254 + t, t < 2^126).
//   * B operand: lane l holds, for element e and column tile ct, the 16 bytes of half (l >> 5) of element e of sponge 32 ct + (l & 31) — exactly one
//     16-byte state slot.  A wave keeps the whole state in registers (17 x 2 x 4 VGPRs): every A fragment then feeds 2 MFMAs (1 KB of L2 traffic per
//     64 cycles of matrix pipe, the same bytes per MFMA as the former two-row-tile form; less reuse is L1-bound, tools/mfma_dense.hip).
//   * X takes the even outputs, Y the odd ones.  Per output: 34 MFMAs into 1 x 2 tiles (digits 0..31 x sponges 0..31 / 32..63).
//   * D layout: lane l, register r = row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of column l & 31: a sponge's 32 digit sums sit in lanes l and l + 32.
//     v_permlane32_swap(tile of sponges 0..31, tile of sponges 32..63) hands the lower lane the upper lane's rows of ITS sponge and vice versa, so
//     that afterwards lane l owns sponge l (the kernels' lane <-> sponge map) with the rows in a lane-uniform order.
//   * fold and finish: mfma_digits.hpp, the statements the host checks run, with the bound of every intermediate.  This product's rows and the rows of the
//     8-round blocks that end as limbs: word columns folded in the lane that holds the sums, exchanged afterwards (mfma_word_cols_mad, mfma_finish_words,
//     sbox_lazy29; mfma_post_words / mfma_post_limbs below), |S_c| <= 17 * 32 * 128 * 128 = 8 912 896 here.  The older pipeline — exchange of all 32 sums, nine
//     limb columns (mfma_fold_rows, mfma_finish_limbs / mfma_finish_cols; any |digit sum| < 2^24) — serves the rows that end canonical elsewhere (mfma_post).
// One row pipeline serves this product and the two of the 8-round blocks: zeroed tile -> MFMAs -> fold, exchange -> a canonical finish or the limb-form
// hand-over to the next S-box (pair_sto_sbox29).
typedef int mfma_v4i __attribute__((ext_vector_type(4)));
typedef int mfma_v16i __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void mfma_zero_tile(mfma_v16i (&acc)[2]) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0;
}
// exchange of all 32 sums, fold into the nine limb columns of the lane's sponge, finish: -> the canonical field element
__device__ __forceinline__ fr_t mfma_post(const mfma_v16i (&acc)[2]) {
    mfma_v16i lo, hi;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const auto sw = __builtin_amdgcn_permlane32_swap((unsigned)acc[0][r], (unsigned)acc[1][r], false, false);
        lo[r] = (int)sw[0]; hi[r] = (int)sw[1];
    }
    int64_t col[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) col[k] = 0;
    mfma_fold_rows(col, lo, hi);
    return mfma_finish_cols(col);
}
// fold, exchange, byte-domain finish: -> the signed residue's digits of the lane's sponge (mfma_digits.hpp mfma_finish_bytes).  Each lane folds the registers it
// holds — four word columns per tile: words 0, 2, 4, 6 of its sponges in the lower lane, 1, 3, 5, 7 in the upper one — and only the four 64-bit columns of
// each tile cross the lane pair: 8 v_permlane32_swap against the 16 of mfma_post.  Rows of at most 9 K-steps (the int32 pairs of mfma_word_cols).
__device__ __forceinline__ fr_t mfma_post_bytes(const mfma_v16i (&acc)[2]) {
    int64_t c0[4], c1[4], col[8];
    mfma_word_cols(acc[0], c0); mfma_word_cols(acc[1], c1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)(uint64_t)c0[q], (unsigned)(uint64_t)c1[q], false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)((uint64_t)c0[q] >> 32), (unsigned)((uint64_t)c1[q] >> 32), false, false);
        col[2 * q] = (int64_t)((uint64_t)lo[0] | ((uint64_t)hi[0] << 32)); col[2 * q + 1] = (int64_t)((uint64_t)lo[1] | ((uint64_t)hi[1] << 32));
    }
    return mfma_finish_bytes(col);
}
// fold, exchange, word-column finish: -> nine limbs of some W == V (+ c) (mod r) for an S-box (mfma_digits.hpp mfma_word_cols_mad, mfma_finish_words: W below
// 3 r + 2^146, limbs 0..7 below 2^29, the top limb below 2^24).  The same exchange as mfma_post_bytes — four finished 64-bit columns per tile, 8 swaps — for rows
// of up to 16 + 7 K-steps.  c29 != nullptr: a stored constant's nine limbs; its eight words enter the columns in front of the quotient.
__device__ __forceinline__ void mfma_post_words(const mfma_v16i (&acc)[2], int64_t* col, const uint32_t* c29 = nullptr) {
    int64_t c0[4], c1[4];
    mfma_word_cols_mad(acc[0], c0); mfma_word_cols_mad(acc[1], c1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)(uint64_t)c0[q], (unsigned)(uint64_t)c1[q], false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)((uint64_t)c0[q] >> 32), (unsigned)((uint64_t)c1[q] >> 32), false, false);
        col[2 * q] = (int64_t)((uint64_t)lo[0] | ((uint64_t)hi[0] << 32)); col[2 * q + 1] = (int64_t)((uint64_t)lo[1] | ((uint64_t)hi[1] << 32));
    }
    if (c29) mfma_words_add_c29(col, c29);
}
__device__ __forceinline__ void mfma_post_limbs(const mfma_v16i (&acc)[2], uint32_t* l, const uint32_t* c29 = nullptr) {
    int64_t col[8];
    mfma_post_words(acc, col, c29);
    mfma_finish_words(col, l);
}
// The limb-form hand-over of a row: its nine finish limbs l (mfma_finish_words) go straight through the next full round's S-box (rc29: that round's constant
// for element j, nine limbs) and into slot j as the next product's operand, recoded — the squeeze round's too: its row runs on the matrix cores
// (pair_squeeze_row_mfma).  No canonical value in between.  The finish itself stays at the two call sites: taken in here as well, k_node16_pair<true> holds one VGPR more than before the merge (245).
__device__ __forceinline__ void pair_sto_sbox29(const PairState& s, int j, const uint32_t* l, const uint32_t* rc29) {
    s.sto(j, recode_lazy29(pow5_lazy29(lazy29_add_c29(l, rc29))));      // recoded from the unreduced x5 (below 1.04 r)
}
// How a row of the full rounds' product ends (wave-uniform, a runtime value):
//   Canonical   the state canonical and consistent (mfma_finish_words_canonical);
//   NextSbox    handed to the NEXT full round's S-box in the wave that formed it (pair_sto_sbox29 with rc29 = that round's constants, 17 x 9 limbs) — X the even
//               elements, Y the odd ones, nothing crosses waves: no LDS round trip, no standalone S-box pass and one barrier less per round;
//   BlockEntry  (the product in front of the partial rounds of pair_permute_fused, frag = mds_pre_frag) as the 8-round blocks take them, no canonical value, no
//               recode pass and no further barrier — rows 1..16, the lanes, as the digits of their signed residue (mfma_finish_bytes on the same word columns:
//               rows of 17 K-steps, |S_c| <= 8 912 896, |col| <= 16 843 009 |S| < 2^47.1, the bound stated there for the wide rows); row 0, the chain value, as
//               its nine finish limbs in the mailbox layout (lazy29_to_slot) in slot kEntrySlot, which wave X — the wave that formed it — reads back as the
//               chain's start.  That slot is H's mailbox of the ODD rounds: Y first writes it in round 1, behind barrier_0, which X passes after its read.
//               (Slot 0, the even rounds' mailbox, is written by Y inside round 0: a read of it with no barrier in between would race.)
constexpr int kEntrySlot = 17 + 2;
// The product.  Precondition: every state slot holds a recoded S-box output and a barrier has passed.  Ends with a barrier.  rc29 is read by NextSbox alone.
__device__ __forceinline__ void pair_mds_sbox_mfma(const PairState& s, const void* frag, RowEnd end, const uint32_t* rc29 = nullptr) {
    constexpr int T = 17;
    const int lane = s.lane, h = lane >> 5;
    mfma_v4i b[T][2];
#pragma unroll
    for (int e = 0; e < T; ++e)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) { const uint4 u = s.st[(2 * e + h) * 64 + 32 * ct + (lane & 31)]; b[e][ct] = mfma_v4i{(int)u.x, (int)u.y, (int)u.z, (int)u.w}; }
    __syncthreads();                                   // both waves hold the state: the slots may be overwritten
    const mfma_v4i* A = reinterpret_cast<const mfma_v4i*>(frag) + lane;
#pragma unroll 1
    for (int i = s.isY ? 1 : 0; i < T; i += 2) {
        mfma_v16i acc[2];
        mfma_zero_tile(acc);
        const mfma_v4i* Ai = A + (size_t)i * T * 64;
#pragma unroll
        for (int e = 0; e < T; ++e) {
            const mfma_v4i a = Ai[(size_t)e * 64];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[e][ct], acc[ct], 0, 0, 0);
        }
        // one fold and exchange in front of all three ends: with the canonical end on its own path (mfma_post) the fused kernels spill
        int64_t col[8];
        mfma_post_words(acc, col);
        if (end == RowEnd::NextSbox) { uint32_t l[9]; mfma_finish_words(col, l); pair_sto_sbox29(s, i, l, c29(rc29, i)); }
        else if (end == RowEnd::BlockEntry) {
            if (i == 0) { uint32_t l[9]; mfma_finish_words(col, l); s.sto(kEntrySlot, lazy29_to_slot(l)); }
            else s.sto(i, mfma_finish_bytes(col));
        }
        else s.sto(i, mfma_finish_words_canonical(col));
    }
    __syncthreads();
}

// slot j (recoded) as the B operand of column tile ct: half (lane >> 5) of the element of sponge 32 ct + (lane & 31)
__device__ __forceinline__ mfma_v4i blk8_b_of_slot(const PairState& s, int j, int ct) {
    const uint4 u = s.st[(2 * j + (s.lane >> 5)) * 64 + 32 * ct + (s.lane & 31)];
    return mfma_v4i{(int)u.x, (int)u.y, (int)u.z, (int)u.w};
}
// The squeeze round's product when only element 0 is wanted: ROW 0 of the same product, one row of the pipeline in the calling wave alone — 34 MFMAs with the
// B operands read from the slots as they are consumed, one fold and exchange, the canonical finish (|S_c| <= 17 * 32 * 128 * 128, the full rounds' bound; W below
// 3 r: mfma_finish_words_canonical).  Precondition as for the product: every slot a recoded S-box output, a barrier since.  No barrier inside: the caller runs it
// in wave X between two barriers that both waves pass.
__device__ __forceinline__ fr_t pair_squeeze_row_mfma(const PairState& s, const void* frag) {
    constexpr int T = 17;
    const mfma_v4i* A = reinterpret_cast<const mfma_v4i*>(frag) + s.lane;      // fragments (0, e)
    mfma_v16i acc[2];
    mfma_zero_tile(acc);
    // eight fragments in flight at a time: with all 17 fragments and 34 operands hoisted above the MFMAs every k_hash_ds2<17> instantiation spilled
#pragma unroll 1
    for (int e0 = 0; e0 < 16; e0 += 8) {
        mfma_v4i a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = A[(size_t)(e0 + k) * 64];
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[k], blk8_b_of_slot(s, e0 + k, ct), acc[ct], 0, 0, 0);
    }
    {
        const mfma_v4i a = A[(size_t)16 * 64];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, blk8_b_of_slot(s, 16, ct), acc[ct], 0, 0, 0);
    }
    int64_t col[8];
    mfma_post_words(acc, col);
    return mfma_finish_words_canonical(col);
}
// Round 0 of the leaf permutation through the same row pipeline with TWO K-steps: 15 of the 17 lanes of hash_leaf_pair's template are constants, so round 0's
// product is K_i + M[i][4] x4 + M[i][5] x5 (host_util.hpp leaf_round0_consts), a dense row with two live columns and a constant.  Precondition: slots 4 and 5 hold
// x4 and x5 RECODED and a barrier has passed.  Row i = fragments (i, 4), (i, 5) of the full rounds' table against the two operands, fold and exchange and finish
// as every fused row (mfma_post_limbs), and the hand-over to round 1's S-box with krc29[i] = (K_i + rc_full[17 + i]) mod r as its constant — X the even rows,
// Y the odd ones.  Ends like pair_sbox_full<17> of round 1: every slot a recoded S-box output, behind a barrier.
//   digit sums  |S_c| <= 2 * 32 * 128 * 128 = 1 048 576 = 2^20, far inside mfma_word_cols_mad's domain (23 K-steps);
//   S-box input u = W + krc29[i] with W < 3 r + 2^146 (mfma_finish_words) and the constant canonical: u < 4 r + 2^146 < 4.0001 r, limbs below 2^30 — the fused
//               rows' bound, inside pow5_lazy29's 4.25 r.
__device__ __forceinline__ void pair_leaf_round0_mfma(const PairState& s, const void* frag, const uint32_t* krc29) {
    constexpr int T = 17;
    mfma_v4i b[2][2];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) b[e][ct] = blk8_b_of_slot(s, 4 + e, ct);
    __syncthreads();                                   // both waves hold x4 and x5: slots 4 and 5 may be overwritten
    const mfma_v4i* A = reinterpret_cast<const mfma_v4i*>(frag) + s.lane;
#pragma unroll 1
    for (int i = s.isY ? 1 : 0; i < T; i += 2) {
        mfma_v16i acc[2];
        mfma_zero_tile(acc);
        const mfma_v4i* Ai = A + ((size_t)i * T + 4) * 64;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const mfma_v4i a = Ai[(size_t)e * 64];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[e][ct], acc[ct], 0, 0, 0);
        }
        uint32_t l[9]; mfma_post_limbs(acc, l);
        pair_sto_sbox29(s, i, l, c29(krc29, i));
    }
    __syncthreads();
}

// ---- partial rounds in BLOCKS OF 8, both long products on the matrix cores (T = 17, rp % 8 == 0) ------------------------------------------------------
// Algebra (host_util.hpp blk8_*): with the lanes s_1..s_16 at their block-start values and y_q = (X_q + c_q)^5,
//     X_{q+1} = E_q + a_q y_q + sum_{p<q} Gamma_{q,p} y_p,   E_q = sum_j u_{q,j} s_j,   and at the end of the block   s_j <- s_j + sum_p w_{p,j} y_p.
// The 8 x 16 E-product and the 16 x 8 lane product are residue-table products like the full rounds' (same tile, exchange, fold and finish):
//   * the lanes live in LDS RECODED (signed digits) between the blocks, so a lane's slot is a B operand as it stands;
//   * E-product: fragments of u_{q,j}, unscaled (the lanes are in stored form); |digit sum| <= 16 * 32 * 128 * 128 = 2^23;
//   * lane product: fragments of w_{p,j} * 2^20 (the y are fr_pow5_r29 outputs) and, as a ninth K-step, the fragment of the constant 1 against the lane's
//     own slot, which adds the base lane inside the tile: |digit sum| <= 9 * 32 * 128 * 128 = 4 718 592 < 2^24.  mfma_finish_cols holds for any
//     |S_c| < 2^24, so both products end canonical and the lazy-lane bound of pair_lane_update does not apply to this form.
// The third product of the block algebra rides in the E rows' tiles: H_q = E_q + sum_{p<q} Gamma_{q,p} y_p is row q of a product with constant left
// factors, and y_0..y_{q-1} are known when round q starts, so row q takes them as q further K-steps (fragments of Gamma_{q,p} * 2^20, blk8_gfrag) before the
// exchange, fold and finish it pays anyway: |digit sum| <= (16 + 7) * 32 * 128 * 128 = 12 058 624 < 2^24.  No Gamma term is left on the vector ALU.
// The chain is SCALED (host_util.hpp blk8s_*): X carries s0 = lambda_q X_q, lambda_0 = 1, lambda_{q+1} = lambda_q^5 kappa / a over all rp rounds (kappa = 2^-20,
// fr_pow5_r29's scale; a = M[0][0] = every a_q).  Then yt_q = fr_pow5_r29(s0 + lambda_q c_q) = kappa lambda_q^5 y_q and
//     lambda_{q+1} X_{q+1} = yt_q + lambda_{q+1} ( E_q + sum_{p<q} Gamma_{q,p} y_p ):
// the S-box output enters with coefficient 1 — no a_q y_q product (unpack, 81 MACs, Montgomery step, carry pass, pack, conditional subtraction) on the chain.
// Every lambda sits on a constant left factor: E fragments u_{q,j} lambda_{q+1}, Gamma fragments Gamma_{q,p} lambda_{q+1} / (kappa lambda_p^5), lane fragments
// w_{p,j} / (kappa lambda_p^5) (the posted yt_p stand for the y_p), constants lambda_q c_q; the unit fragment and the lanes are unscaled.  After the last block ONE
// product by 1 / lambda_rp brings X_rp back (fr_mul_c29).  Exact field arithmetic: the same bits.  The fragments are still digits of residues in [0, r): the digit-sum
// bounds above stand.
// The chain is a LAZY RESIDUE inside a block (mfma_digits.hpp, with the bounds): Y finishes row q to its nine limbs with lambda_{q+1} c_{q+1} as the columns'
// addend and posts the limbs in the 32-byte slot; X adds them limb-wise to x5's limbs and squares the sum as it stands; y_q is posted recoded from the
// packed, unreduced x5.  No conditional subtraction, pack-and-unpack or constant add is left on the chain; canonical values exist only outside the blocks.
// Schedule of a block (two barriers fewer than two blocks of 4, nothing on the chain waits for a lone row):
//   X  runs nothing but the chain, the same in every round: the S-box's three products, recode and post, and after the barrier nine limb adds with H_q's slot;
//   Y  computes H_q INSIDE round q — B operands read from the lanes' slots as the MFMAs consume them (one row per round: 32 KB of LDS reads per about
//      10 k cycles), then the q steps of the y; the fragments of row q + 1 (16 of E, q + 1 of Gamma) are fetched under the fold — and posts it; one barrier per round;
//   both then form their share of the lane product (X lanes 1..NLX, Y the rest), the next row's fragments in flight under the current row's fold.
// X posts y_q RECODED: a recoded slot is a B operand as it stands, and both waves read it as one after the round's barrier (X its own write back), so
// no wave converts a y and none holds one as a field element across rounds.  Four slots are free during a block (slot 0: X holds the chain value; the
// three extra ones): two rings of two, H (written by Y, read by X after the round's barrier) and y (the other way round).
// Measured stand-alone (tools/partial_block8.hip, profiles/partial_block8_gamma_rows_prototype.jsonl): 105.1 / 104.2 k SIMD-cycles per 8 rounds against
// 118.4 / 116.1 k with the Gamma terms on the vector ALU and 209.3 / 206.6 k for two blocks of 4; pipelining wave Y across the round barrier (the lane
// steps and the older Gamma steps of row q + 1 before barrier_q) measured 106.7 / 105.4 k: not adopted.
struct Blk8Tabs {
    const mfma_v4i* efrag;     // [8][16][64]   row q, lane j = 1..16
    const mfma_v4i* lfrag;     // [16][8][64]   lane j = 1..16, S-box output p
    const mfma_v4i* unit;      // [64]          the constant 1
    const mfma_v4i* gfrag;     // [28][64]      Gamma_{q,p} at q (q - 1) / 2 + p
    const uint32_t* rc29;      // [9][9]        lambda_q c_q of rounds 1..8 (the next block's round 0; zero after the last block) as nine limbs (rc_partial_scaled29)
};
struct Blk8Cfg {
    // X's share of the lane rows.  Measured, k SIMD-cycles per 8 rounds in two processes: 6 -> 107.7 / 107.0, 7 -> 105.8 / 106.1, 8 -> 105.1 / 104.2, 9 -> 106.4 / 107.0,
    // 10 -> 111.6 / 111.8 (run-to-run spread 2-5 k)
    static constexpr int NLX = 8;
    __host__ __device__ static constexpr int ymail(int q) { return 17 + (q & 1); }
    __host__ __device__ static constexpr int hmail(int q) { return (q & 1) ? 19 : 0; }
};
static_assert(kEntrySlot == Blk8Cfg::hmail(1) && kEntrySlot != Blk8Cfg::hmail(0) && kEntrySlot != Blk8Cfg::ymail(0), "the entry row's slot is untouched until barrier_0");
// A is wave-uniform and the lane is added at the load: a scalar base plus one 32-bit lane offset
__device__ __forceinline__ void blk8_load_frags16(mfma_v4i (&a)[16], const mfma_v4i* A, int lane) {
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = (A + (size_t)e * 64)[lane];
}
// round Q in wave X: u = lambda_Q X_Q + lambda_Q c_Q on entry, the same of round Q + 1 on exit, as a LAZY residue (nine limbs below 2^30, below 3.05 r:
// mfma_digits.hpp); no field element is formed.  b[Q]: yt_Q as B operands on exit
template <int Q>
__device__ __forceinline__ void blk8_round_x(const PairState& s, const Blk8Tabs& Tb, fr29_t& u, mfma_v4i (&b)[8][2]) {
    __builtin_amdgcn_sched_barrier(0);                     // keep the rounds apart: less register pressure
    const fr29_t x5 = pow5_lazy29(u);                      // yt_Q below 1.04 r
    s.sto(Blk8Cfg::ymail(Q), recode_lazy29(x5));           // off the chain: nothing of X_{Q+1} reads it
    __syncthreads();                                       // barrier_Q: H_Q + lambda_{Q+1} c_{Q+1} is posted as its nine finish limbs
    u = lazy29_add_slot(x5, s.ld(Blk8Cfg::hmail(Q)));
    b[Q][0] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 0); b[Q][1] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 1);
}
// round Q in wave Y.  a, g: the fragments of E row Q and of Gamma row Q on entry, of row Q + 1 on exit; b[Q]: y_Q as B operands on exit
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
    { uint32_t l[9]; mfma_post_limbs(acc, l, c29(Tb.rc29, Q)); s.sto(Blk8Cfg::hmail(Q), lazy29_to_slot(l)); }
    __syncthreads();                                       // barrier_Q: y_Q is posted
    b[Q][0] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 0); b[Q][1] = blk8_b_of_slot(s, Blk8Cfg::ymail(Q), 1);
}
// How a lane row of an 8-round block ends (wave-uniform, a runtime value).  Between two blocks:
//   Bytes      (pair_permute_fused) the digits of the lane's SIGNED residue, finished in the byte domain (mfma_post_bytes: word columns folded where the sums sit,
//              a quotient estimate, one pass over eight words; no 29-bit limbs, no conditional subtraction);
//   Recoded    (pair_permute_blk8) the canonical value, recoded.  k_hash_ds2 keeps it: with the signed form k_hash_ds2<17, DsBatchStream, true> spilled 6 VGPRs
//              (28 B of scratch);
// in the permutation's last block:
//   NextSbox   (pair_permute_fused) lane j goes from its nine finish limbs through the S-box of the full round that follows (rc29_next: that round's constants,
//              17 x 9 limbs) and is stored recoded as the round's operand, like a fused product row;
//   Canonical  (pair_permute_blk8) the canonical value.
// the lane product: s_j <- s_j + sum_p w_{p,j} y_p for this wave's share of the lanes (X lanes 1..NLX, Y the rest), b: y_0..y_7 as B operands.  Ends with a barrier.
template <int NLX>
__device__ __forceinline__ void blk8_lane_rows(const PairState& s, const Blk8Tabs& Tb, const mfma_v4i (&b)[8][2], LaneEnd end, const uint32_t* rc29_next = nullptr) {
    static_assert(NLX >= 1 && NLX <= 15, "shares");
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
        // slot j is read by this wave alone, before this write
        if (end == LaneEnd::NextSbox) { uint32_t l[9]; mfma_post_limbs(acc, l); pair_sto_sbox29(s, j, l, c29(rc29_next, j)); }
        else if (end == LaneEnd::Bytes) s.sto(j, mfma_post_bytes(acc));
        else { const fr_t z = mfma_post(acc); s.sto(j, end == LaneEnd::Canonical ? z : recode_signed(z)); }
    }
    __syncthreads();
}
// One block.  Precondition: lanes 1..16 RECODED in their slots (canonical values or digits of a signed residue) and a barrier since; u = lambda_0 X_0 + lambda_0 c_0
// of the block's first round as nine limbs in wave X.  Ends with a barrier, the lanes as `end` names.
// With LaneEnd::NextSbox every slot ends as the next full round's S-box output — the lanes through blk8_lane_rows, element 0 from the chain's final value
// (lazy, no constant in it), brought back from lambda_rp X_rp by one product with unscale29 = 1 / lambda_rp first and handed to the S-box as limbs.
template <int NLX>
__device__ __forceinline__ void pair_block8(const PairState& s, const Blk8Tabs& Tb, fr29_t& u, LaneEnd end, const uint32_t* rc29_next = nullptr,
                                            const uint32_t* unscale29 = nullptr) {
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
    // slot 0 was H's mailbox in the even rounds, last read by X after barrier_6; the lane rows' closing barrier publishes the store
    if (end == LaneEnd::NextSbox && !s.isY) { const fr29_t x = fr29_mul_c29(unscale29, u); pair_sto_sbox29(s, 0, x.l, c29(rc29_next, 0)); }
    blk8_lane_rows<NLX>(s, Tb, b, end, rc29_next);
}
// The partial rounds in rp / 8 blocks, the lanes ending as `mid` names between two blocks and as `last` names after the last one.
__device__ __forceinline__ void pair_blocks8(const PairState& s, const PoseidonDev& P, fr29_t& u, LaneEnd mid, LaneEnd last) {
    const int nb = P.rp / 8;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
        const Blk8Tabs Tb{reinterpret_cast<const mfma_v4i*>(P.blk8_efrag) + (size_t)b * 8 * 16 * 64, reinterpret_cast<const mfma_v4i*>(P.blk8_lfrag) + (size_t)b * 16 * 8 * 64,
                          reinterpret_cast<const mfma_v4i*>(P.blk8_unit_frag), reinterpret_cast<const mfma_v4i*>(P.blk8_gfrag) + (size_t)b * 28 * 64,
                          c29(P.rc_partial_scaled29, (size_t)8 * b + 1)};
        pair_block8<Blk8Cfg::NLX>(s, Tb, u, b == nb - 1 ? last : mid, c29(P.rc_full29, (size_t)(P.rf / 2) * 17), P.blk8_unscale29());
    }
}

// ---- partial rounds in BLOCKS OF 4 on the vector ALU (permute_core in poseidon_dev.hpp has the algebra) ---------------------------------------------------
//   phase 1  X runs the S-box chain: x_q, then a_q x_q + sum_{p<q} gamma x_p + its share (lanes 1..NXD) of the lane dot product from registers; Y computes the
//            other lanes' part of every round's dot product from the block-start state and posts it in an LDS mailbox (one barrier per round);
//   phase 2  both waves bring their half of the lanes up to date, s_j += sum_p w_{p,j} x_p (one reduction per lane), X from registers, Y from the x mailboxes.
// The mailboxes reuse state slots that are dead during the block (slot 0: X holds s0 in registers; slots 1..NXD: X preloads those lanes), so the LDS budget
// stays at 4 workgroups per CU.
// s_j += w_{0,j} x0 + w_{1,j} x1 + w_{2,j} x2 + w_{3,j} x3   (one reduction)
template <int T>
__device__ __forceinline__ fr_t pair_lane_update(const uint32_t* sp, int j, const fr_t& base, const fr29_t& x0, const fr29_t& x1, const fr29_t& x2, const fr29_t& x3) {
    constexpr int W = 2 * T - 1;
    fr_wide29 u; fr_wide29_zero(u);
    fr_wide29_mac(u, c29(sp, 0 * W + T - 1 + j), x0); fr_wide29_mac(u, c29(sp, 1 * W + T - 1 + j), x1);
    fr_wide29_mac(u, c29(sp, 2 * W + T - 1 + j), x2); fr_wide29_mac(u, c29(sp, 3 * W + T - 1 + j), x3);
    // The lanes are NOT canonical between the blocks: the Montgomery quotient (below 1.1 r) is added as it is and r subtracted once, so a lane grows by
    // at most 0.1 r per block (below 2.7 r after the 16 blocks: eight words hold it); its consumers unpack and multiply (quotient bounds of fr29.hpp hold
    // for operands below 4 r), and the next full round's S-box returns canonical values.
    return fr_add<PF>(base, fr_wide29_reduce_lazy<PF>(u));
}

// All rp partial rounds.  Precondition: state consistent.  Ends with the state consistent; the lanes 1..T-1 are NOT canonical (pair_lane_update), element 0 is.
template <int T>
__device__ __forceinline__ void pair_blocks4(const PairState& s, const PoseidonDev& P) {
    typedef PairCfg<T> Cfg;
    constexpr int NXD = Cfg::NXD, NXU = Cfg::NXU, W = 2 * T - 1;
    fr_t s0 = fr_zero<PF>();
    if (!s.isY) s0 = s.ld(0);
    for (int b = 0; b < P.rp / 4; ++b) {
        const uint32_t* sp = c29(P.sparse29, (size_t)(4 * b) * W);
        const uint32_t* g = c29(P.gamma29, (size_t)b * 6);
        if (!s.isY) {
            // ---- X: the S-box chain ------------------------------------------------------------------------
            fr_t keep[NXD];
#pragma unroll
            for (int j = 0; j < NXD; ++j) keep[j] = s.ld(1 + j);                  // their slots become Y's mailboxes for this block
            __syncthreads();                                           // S: mailboxes may be written from here on
            // x_0..x_3 live in their LDS mailboxes (this wave reads back its own writes in order); keeping them in
            // registers across the four rounds costs 36 VGPRs and pushes the allocator into scratch.
#define STARK_PAIR_ROUND(q)                                                                           \
            {                                                                                         \
                __builtin_amdgcn_sched_barrier(0);                     /* keep the rounds apart: less register pressure */ \
                const fr_t xq = fr_pow5_r29<PF>(fr_add<PF>(s0, P.rc_partial[4 * b + q]));              \
                s.sto(Cfg::xslot(q), xq);                                                             \
                fr_wide29 acc; fr_wide29_zero(acc);                                                   \
                fr_wide29_mac(acc, c29(sp, q * W), fr29_unpack(xq));                                  \
                if (q > 0) fr_wide29_mac(acc, c29(g, q * (q - 1) / 2 + 0), fr29_unpack(s.ld(Cfg::xslot(0)))); \
                if (q > 1) fr_wide29_mac(acc, c29(g, q * (q - 1) / 2 + 1), fr29_unpack(s.ld(Cfg::xslot(1)))); \
                if (q > 2) fr_wide29_mac(acc, c29(g, q * (q - 1) / 2 + 2), fr29_unpack(s.ld(Cfg::xslot(2)))); \
                if (1 + q + NXD > fr29_max_terms<PF>()) fr_wide29_norm(acc);   /* terms between carry passes (fr29.hpp); with NXD = 3 never */ \
                _Pragma("unroll") for (int j = 0; j < NXD; ++j) fr_wide29_mac(acc, c29(sp, q * W + 1 + j), fr29_unpack(keep[j])); \
                const fr_t part = fr_wide29_reduce<PF>(acc);                                          \
                __syncthreads();                                       /* barrier_q: Dy_q is posted */ \
                s0 = fr_add<PF>(part, s.ld(Cfg::dslot(q)));                                           \
            }
            STARK_PAIR_ROUND(0) STARK_PAIR_ROUND(1) STARK_PAIR_ROUND(2) STARK_PAIR_ROUND(3)
#undef STARK_PAIR_ROUND
            // ---- X: lanes 1..NXU up to date -------------------------------------------------------------------
            const fr29_t x0 = fr29_unpack(s.ld(Cfg::xslot(0))), x1 = fr29_unpack(s.ld(Cfg::xslot(1))), x2 = fr29_unpack(s.ld(Cfg::xslot(2))), x3 = fr29_unpack(s.ld(Cfg::xslot(3)));
#pragma unroll
            for (int j = 1; j <= NXD; ++j) { __builtin_amdgcn_sched_barrier(0); s.sto(j, pair_lane_update<T>(sp, j, keep[j - 1], x0, x1, x2, x3)); }
#pragma unroll 1
            for (int j = NXD + 1; j <= NXU; ++j) s.sto(j, pair_lane_update<T>(sp, j, s.ld(j), x0, x1, x2, x3));
        } else {
            // ---- Y: three quarters of every round's dot product, from the block-start state ----------------------
            __syncthreads();                                           // S
            for (int q = 0; q < 4; ++q) {
                DotAcc acc; acc.init();
#pragma unroll 1
                for (int j = NXD + 1; j < T; ++j) acc.mac(c29(sp, q * W + j), s.ld(j));
                const fr_t dy = acc.finish();
                s.sto(Cfg::dslot(q), dy);
                __syncthreads();                                       // barrier_q
            }
            // ---- Y: lanes NXU+1..T-1 up to date (x_0..x_3 were posted before barrier_0..3) ---------------------------
            const fr29_t x0 = fr29_unpack(s.ld(Cfg::xslot(0))), x1 = fr29_unpack(s.ld(Cfg::xslot(1))), x2 = fr29_unpack(s.ld(Cfg::xslot(2))), x3 = fr29_unpack(s.ld(Cfg::xslot(3)));
#pragma unroll 1
            for (int j = NXU + 1; j < T; ++j) s.sto(j, pair_lane_update<T>(sp, j, s.ld(j), x0, x1, x2, x3));
        }
        __syncthreads();                                               // E: lanes 1..T-1 consistent, mailboxes free
    }
    if (!s.isY) s.sto(0, s0);
    __syncthreads();
}

// ---- the permutations -------------------------------------------------------------------------------------------------------------------------------
// Every entry: one permutation by the wave pair.  Precondition: state consistent (a barrier since the last write).  Returns lane 0 of the result; with only0 in
// wave X ALONE (every caller stores it from there), and the rest of the state is dead afterwards; without only0 the state ends canonical behind a barrier.
// The first full rounds with canonical ends, rounds r_begin .. rf / 2 - 1: the standalone S-box pass, then the dense product (the last one with B_1 folded in).
template <int T>
__device__ __forceinline__ void pair_first_rounds(const PairState& s, const PoseidonDev& P, int r_begin) {
    const int half = P.rf / 2;
    for (int r = r_begin; r < half; ++r) {
        pair_sbox_full<T>(s, P.rc_full + r * T);
        if constexpr (T == 17) pair_mds_sbox_mfma(s, (r == half - 1) ? P.mds_pre_frag : P.mds_frag, RowEnd::Canonical);
        else pair_apply_lu<T>(s, (r == half - 1) ? P.lu_pre29 : P.lu29);
    }
}
// The squeeze round's product when only element 0 is wanted: row 0 alone.  Returned in wave X alone for t = 17.
template <int T>
__device__ __forceinline__ fr_t pair_squeeze(const PairState& s, const PoseidonDev& P) {
    fr_t out = fr_zero<PF>();
    if constexpr (T == 17) {                        // one matrix-core row in wave X (X-only work between two barriers both waves pass)
        if (!s.isY) out = pair_squeeze_row_mfma(s, P.mds_frag);
    } else {                                        // split over the two waves
        const int j0 = s.isY ? PairCfg<T>::NX : 0, j1 = s.isY ? T : PairCfg<T>::NX;
        DotAcc acc; acc.init();
#pragma unroll 1
        for (int j = j0; j < j1; ++j) acc.mac(c29(P.row0_29, j), s.ld(j));
        s.sto(T + (s.isY ? 1 : 0), acc.finish());                // two of the extra slots: not part of the state
        __syncthreads();
        out = fr_add<PF>(s.ld(T + 0), s.ld(T + 1));
    }
    __syncthreads();                                // the slots are reused by the next permutation
    return out;
}
// The last full rounds, rf / 2 .. rf - 1, and the squeeze.  HANDED (pair_permute_fused): every slot already holds the recoded S-box output of round rf / 2 behind
// a barrier, and every product but the last hands its rows to the next round's S-box, so no standalone S-box pass runs; otherwise the state is consistent and the
// ends canonical.  The last round stands outside the loop, so every product's end is known where it is inlined: with one loop and a runtime end
// k_leaf_pair2<true> and k_node16_pair<true> spilled 4 VGPRs.
template <int T, bool HANDED>
__device__ __forceinline__ fr_t pair_last_rounds(const PairState& s, const PoseidonDev& P, bool only0) {
    for (int r = P.rf / 2; r < P.rf - 1; ++r) {
        if constexpr (!HANDED) pair_sbox_full<T>(s, P.rc_full + r * T);
        if constexpr (HANDED) pair_mds_sbox_mfma(s, P.mds_frag, RowEnd::NextSbox, c29(P.rc_full29, (size_t)(r + 1) * T));
        else if constexpr (T == 17) pair_mds_sbox_mfma(s, P.mds_frag, RowEnd::Canonical);
        else pair_apply_lu<T>(s, P.lu29);
    }
    if (P.rf > 0) {                                     // the last round: the squeeze, or a product that ends canonical
        if constexpr (!HANDED) pair_sbox_full<T>(s, P.rc_full + (P.rf - 1) * T);
        if (only0) return pair_squeeze<T>(s, P);
        if constexpr (T == 17) pair_mds_sbox_mfma(s, P.mds_frag, RowEnd::Canonical);
        else pair_apply_lu<T>(s, P.lu29);
    }
    return s.ld(0);
}
// Full rounds on the VALU (t = 9) or on the matrix cores with canonical ends (t = 17), partial rounds in blocks of 4.  With r_begin > 0 the caller has run the
// rounds before r_begin itself and left their output consistent in the state.
template <int T>
__device__ __forceinline__ fr_t pair_permute_blk4(const PairState& s, const PoseidonDev& P, bool only0, int r_begin = 0) {
    pair_first_rounds<T>(s, P, r_begin);
    pair_blocks4<T>(s, P);
    return pair_last_rounds<T, false>(s, P, only0);
}
// t = 17 (a parameter set with blk8 tables), 8-round blocks with canonical hand-overs at both ends of the partial rounds.  The full round in front of them leaves
// lanes 1..16 CANONICAL (mfma_finish_words_canonical), which recode_signed needs (x < r); with rf = 0 the caller's stores must be canonical.
// k_hash_ds2 runs this form and not the fused one: its generic stream state is live across the permutation, and with the S-box's columns beside the product's
// operand registers three of its instantiations took 88 / 36 / 52 B of scratch against 44 / 12 / 28 B without.
__device__ __forceinline__ fr_t pair_permute_blk8(const PairState& s, const PoseidonDev& P, bool only0) {
    pair_first_rounds<17>(s, P, 0);
    // the chain as nine limbs from here to the unscale product; the first constant (lambda_0 = 1) enters here, every later one in Y's finish
    fr_t s0 = fr_zero<PF>();
    if (!s.isY) s0 = s.ld(0);
    fr29_t u = fr29_unpack(s0);
    if (!s.isY) u = lazy29_add_c29(u.l, c29(P.rc_partial_scaled29, 0));      // canonical + canonical: below 2 r, limbs below 2^30
    for (int j = s.isY ? 9 : 1; j <= (s.isY ? 16 : 8); ++j) s.sto(j, recode_signed(s.ld(j)));
    __syncthreads();
    pair_blocks8(s, P, u, LaneEnd::Recoded, LaneEnd::Canonical);
    if (!s.isY) s.sto(0, fr29_pack_reduce<PF>(fr29_mul_c29(P.blk8_unscale29(), u).l));      // lambda_rp X_rp (lazy) -> X_rp, canonical
    __syncthreads();
    return pair_last_rounds<17, false>(s, P, only0);
}
// t = 17, 8-round blocks, no canonical value between the first S-box and the last product: every full-round product that is followed by a full round hands its
// rows to that round's S-box in limb form (RowEnd::NextSbox), the product of round rf / 2 - 1 leaves the lanes and the chain value as the first block takes them
// (RowEnd::BlockEntry), and the last block's lane rows hand theirs to the S-box after the partial rounds (LaneEnd::NextSbox).  Needs r_begin < rf / 2 (the entry
// product must run), which the launchers see to: they pick this form only for sets with rf >= 2, k_leaf_pair2 (r_begin = 1) for rf >= 4.
// SBOXED (k_leaf_pair2<true>): the caller's own product in front of round r_begin has handed its rows to that round's S-box already (pair_leaf_round0_mfma), so
// every slot holds a recoded S-box output behind a barrier and the standalone S-box is skipped.
template <bool SBOXED>
__device__ __forceinline__ fr_t pair_permute_fused(const PairState& s, const PoseidonDev& P, bool only0, int r_begin) {
    const int half = P.rf / 2;
    if constexpr (!SBOXED) { if (r_begin < half) pair_sbox_full<17>(s, P.rc_full + r_begin * 17); }
    for (int r = r_begin; r < half; ++r)
        pair_mds_sbox_mfma(s, (r == half - 1) ? P.mds_pre_frag : P.mds_frag, (r == half - 1) ? RowEnd::BlockEntry : RowEnd::NextSbox, c29(P.rc_full29, (size_t)(r + 1) * 17));
    // the entry product left the lanes as digits and row 0 as its finish limbs W (below 3 r + 2^146, limbs below 2^29) behind its closing barrier:
    // u = W + lambda_0 c_0 below 4 r + 2^146 < 4.0001 r with limbs below 2^30, the fused rows' bound, inside pow5_lazy29's 4.25 r
    fr29_t u;
#pragma unroll
    for (int i = 0; i < 9; ++i) u.l[i] = 0;
    if (!s.isY) { u = lazy29_add_slot(u, s.ld(kEntrySlot)); u = lazy29_add_c29(u.l, c29(P.rc_partial_scaled29, 0)); }
    pair_blocks8(s, P, u, LaneEnd::Bytes, LaneEnd::NextSbox);      // the chain value is unscaled inside the last block, in front of element 0's S-box
    return pair_last_rounds<17, true>(s, P, only0);
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------------------------

// K3 (pair form): h[i] = hash_leaf_pair(f[i], f_next[i/m] or 0).  Block = 128 threads = 64 states.
template <bool BLK8>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) k_leaf_pair2(PoseidonDev P, const LeafConsts* __restrict__ lc, const fr_t* __restrict__ f,
                                                    const fr_t* __restrict__ f_next, size_t n, size_t m, fr_t* __restrict__ h) {
    extern __shared__ uint4 lds[];
    PairState s = pair_setup(lds);
    const size_t i = (size_t)blockIdx.x * 64 + s.lane; const bool live = i < n; const size_t ii = live ? i : n - 1;   // tail lanes recompute the last leaf
    // Round 0 in closed form: 15 of the 17 lanes of the transcript template are constants, so after ARK and
    // S-box the MDS output is  K_i + M[i][4]*x4 + M[i][5]*x5  with K precomputed on the host (LeafConsts).
    if constexpr (BLK8) {
        // The 8-round form: X computes x4, Y x5 (the zero input without f_next), each stored recoded; the product is a two-K-step row per element on the
        // matrix cores, handed to round 1's S-box in limb form (pair_leaf_round0_mfma), and the permutation is entered behind that S-box.
        const fr_t in = s.isY ? (f_next ? ldg(f_next + ii / m) : fr_zero<PF>()) : ldg(f + ii);
        s.sto(s.isY ? 5 : 4, recode_signed(fr_pow5_r29<PF>(fr_add<PF>(in, P.rc_full[s.isY ? 5 : 4]))));
        __syncthreads();
        pair_leaf_round0_mfma(s, P.mds_frag, lc->krc29);
        const fr_t out = pair_permute_fused<true>(s, P, true, 1);
        if (live && !s.isY) stg(h + i, out);
    } else {
    // The blocks of 4 (the comparison form): both waves compute x4, x5; each fills its own lanes on the vector ALU.
    const fr_t x4 = fr_pow5_r29<PF>(fr_add<PF>(ldg(f + ii), P.rc_full[4]));
    const fr_t x5 = fr_pow5_r29<PF>(fr_add<PF>(f_next ? ldg(f_next + ii / m) : fr_zero<PF>(), P.rc_full[5]));
    const int j0 = s.isY ? PairCfg<17>::NX : 0, j1 = s.isY ? 17 : PairCfg<17>::NX;
    const fr29_t x4u = fr29_unpack(x4), x5u = fr29_unpack(x5);
    for (int j = j0; j < j1; ++j) {
        fr_wide29 w; fr_wide29_zero(w);
        fr_wide29_mac(w, c29(lc->m45_29, j), x4u); fr_wide29_mac(w, c29(lc->m45_29, 17 + j), x5u);
        s.sto(j, fr_add<PF>(lc->K[j], fr_wide29_reduce<PF>(w)));
    }
    __syncthreads();
    fr_t out = pair_permute_blk4<17>(s, P, true, 1);
    if (live && !s.isY) stg(h + i, out);
    }
}

// K4 (pair form): one Merkle level / the pair-leaf level.
template <int T, class DS, bool BLK8 = false>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) k_hash_ds2(PoseidonDev P, DS D, fr_t* __restrict__ out) {
    extern __shared__ uint4 lds[];
    constexpr int rate = T - 1;
    PairState s = pair_setup(lds);
    const size_t k0 = (size_t)blockIdx.x * 64 + s.lane; const bool live = k0 < D.n_out; const size_t k = live ? k0 : D.n_out - 1;
    const int o0 = s.isY ? PairCfg<T>::NX : 0, o1 = s.isY ? T : PairCfg<T>::NX;      // elements this wave fills / absorbs into
    for (int j = o0; j < o1; ++j) s.sto(j, fr_zero<PF>());
    __syncthreads();
    const size_t total = D.total(k), nperm = (total + rate - 1) / rate;
    // The widest stream in the block decides how many permutations every lane walks through (barriers are wave-level: both waves
    // of the pair must execute the same sequence).  A lane with a SHORTER stream (the ragged last node of a level) sits out the
    // first max_perm - nperm of them — it permutes a dead state, clears it, and starts absorbing late — so that EVERY lane's result
    // is lane 0 of the last permutation: nothing has to be carried in registers across the permutations (the kernel sits at the
    // 256-VGPR limit; carrying a per-lane result across pair_permute spilled 118 VGPRs to scratch).
    const size_t max_perm = (D.max_total() + rate - 1) / rate;
    const size_t skip = max_perm - nperm;
    size_t q = 0; fr_t res = fr_zero<PF>();
    for (size_t pidx = 0; pidx < max_perm; ++pidx) {
        if (pidx >= skip) {
            if (skip && pidx == skip) for (int j = o0; j < o1; ++j) s.sto(j, fr_zero<PF>());       // the dead permutations left garbage behind
            for (int cur = 0; cur < rate && q < total; ++cur, ++q) {
                if (cur < o0 || cur >= o1) continue;
                s.sto(cur, fr_add<PF>(s.ld(cur), D.elem(k, q)));
            }
        }
        __syncthreads();
        if constexpr (BLK8) res = pair_permute_blk8(s, P, pidx + 1 == max_perm);
        else res = pair_permute_blk4<T>(s, P, pidx + 1 == max_perm);
        __syncthreads();
    }
    if (live && !s.isY) stg(out + k0, res);
}

// K4, arity 16 (pair form): one Merkle level of t = 17 whose every node has exactly 16 children, node k = in[16 k .. 16 k + 16) at DS position pos0 + k.
// The node's stream is [arity, level, pos0 + k, label] || 16 children || 1: exactly two permutations, both fixed at compile time — perm 1 over
// elements 0..15 = (DS words, children 0..11) with capacity 0, perm 2 after absorbing children 12..15 and the closing 1 into elements 0..4, squeezed.
// Nothing of k_hash_ds2's generic machinery (element-by-element absorbs through DS::elem, dead permutations for ragged nodes, a runtime squeeze flag)
// is live across a permutation.  Measured (tools/node_rate.py, 2^19 nodes): 17.4 ms against 17.7 for k_hash_ds2<17>, 60 M perm/s against the leaf
// kernel's 69: the rest of the gap is work, not spills — both permutations run round 0 in full (one more MFMA product than k_leaf_pair2's
// closed-form round 0, about 1/8 of a permutation's full-round time).  Two inlined permutations measured faster than one in a loop (17.6 ms).
template <bool BLK8>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) k_node16_pair(PoseidonDev P, fr_t arity_f, fr_t level_f, fr_t label_f, uint64_t pos0,
                                                    const fr_t* __restrict__ in, size_t n_out, fr_t* __restrict__ out) {
    extern __shared__ uint4 lds[];
    PairState s = pair_setup(lds);
    const size_t k0 = (size_t)blockIdx.x * 64 + s.lane; const bool live = k0 < n_out; const size_t k = live ? k0 : n_out - 1;   // tail lanes recompute the last node
    const fr_t* c = in + k * 16;
    // perm 1: each wave fills the elements it owns in the full rounds (X 0..NX-1, Y NX..16), the children straight from global memory
    static_assert(PairCfg<17>::NX == 8, "X fills elements 0..7");
    if (!s.isY) {
        s.sto(0, arity_f); s.sto(1, level_f); s.sto(2, fr_from_u64<PF>(pos0 + k)); s.sto(3, label_f);
#pragma unroll
        for (int j = 4; j < 8; ++j) s.sto(j, ldg(c + (j - 4)));
    } else {
#pragma unroll
        for (int j = 8; j < 16; ++j) s.sto(j, ldg(c + (j - 4)));
        s.sto(16, fr_zero<PF>());
    }
    __syncthreads();
    if constexpr (BLK8) pair_permute_fused<false>(s, P, false, 0); else pair_permute_blk4<17>(s, P, false);      // ends with a barrier: the state is consistent
    // perm 2: children 12..15 and the closing 1 into elements 0..4 (X's)
    if (!s.isY) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s.sto(j, fr_add<PF>(s.ld(j), ldg(c + 12 + j)));
        s.sto(4, fr_add<PF>(s.ld(4), fr_one<PF>()));
    }
    __syncthreads();
    fr_t res;
    if constexpr (BLK8) res = pair_permute_fused<false>(s, P, true, 0); else res = pair_permute_blk4<17>(s, P, true);
    if (live && !s.isY) stg(out + k0, res);
}

}  // namespace stark
#endif
