// stark_mlwe_amd/csrc/mfma_digits.hpp — the scalar pieces of the int8-MFMA field products, ONE definition for device and host: the signed recoding of an
// operand, the fold of a row's 32 digit sums, the product-free finish (to nine limbs, canonical, or the signed residue's digits), the S-box that takes a row over
// in limb form and the lazy chain of the 8-round blocks (slot layout, limb adds, unreduced recode).
// poseidon_pair.hpp includes it for the t = 17 wave-pair kernels (exchange and tile handling stay there); hostcheck.cpp and tools/mfma_finish_check.cpp
// run the same statements on the CPU against the L*U rows and against big integers (tests/test_hostcheck.py,
// tests/test_full_round_residue_tables_host.py, tests/test_limb_handover_host.py, tests/test_lazy_residue_host.py, tests/test_byte_finish_host.py, tests/test_word_fold_host.py, tests/test_permutation_edges_host.py).  The host-only part at the end: the row-order entry of the fold
// (mfma_cols_of_sums, mfma_word_cols_of_sums, mfma_word_cols_mad_of_sums) and the 128-bit column census of the S-box (Lazy29Wide).
#pragma once
#include "fr.hpp"
#include "fr29.hpp"

namespace stark {

typedef PallasFr PF;
// How a row of the pipeline ends, named once for the kernels (poseidon_pair.hpp, where each end is described at its site) and their host mirror (hostcheck.cpp):
// RowEnd for the full rounds' product (pair_mds_sbox_mfma), LaneEnd for the lane rows of an 8-round block (blk8_lane_rows).  Wave-uniform runtime values.
enum class RowEnd { Canonical, NextSbox, BlockEntry };
enum class LaneEnd { Bytes, Recoded, NextSbox, Canonical };
static_assert(fr_p29<PF>(4) < (1u << 10) && fr_p29<PF>(5) == 0 && fr_p29<PF>(6) == 0 && fr_p29<PF>(7) == 0 && fr_p29<PF>(8) == (1u << 22), "r = 2^254 + t with t below 2^126");

// x (canonical) -> signed radix-256 digits in place of its bytes: add 0x80 to every byte with carries, flip every byte's top bit
// (digit b = byte b - 0x80 in [-128, 127]; x < r keeps the top byte below 0x80, so 32 digits hold it).  The int8 operand form of the MFMA product.
FR_HD fr_t recode_signed(const fr_t& x) {
    fr_t y; uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const uint64_t t = (uint64_t)x.v[i] + 0x80808080u + c; y.v[i] = (uint32_t)t ^ 0x80808080u; c = t >> 32; }
    return y;
}
// Fold and finish of one output row, V = sum_c S_c 256^c, with the bound of every intermediate:
//   digit sum   |S_c| <= 17 * 32 * 128 * 128 = 8 912 896 < 2^24 in a full round (the rows of the 8-round blocks: poseidon_pair.hpp): exact in the i32
//               accumulators.  Everything below holds for ANY |S_c| < 2^24.
//   pair        P = S_c + 256 S_{c+1} (c even), |P| < 257 * 2^24 < 2^32.01, goes into the 64-bit column k = floor(8c / 29) of weight 2^(29k)
//               that holds the lower digit, shifted by 8c - 29k <= 28: |P << sh| < 2^60.01.
//   column      nine columns (8 * 30 = 240 = 29 * 8 + 8); bit positions 16 apart: at most two pairs per column, |col| < 2^61.01; with the carry
//               from below (< 2^32.1) still < 2^62.  The signed carry pass leaves limbs 0..7 in [0, 2^29) and top = floor(V / 2^232) in column 8:
//               |V| < 2^24 * (256^32 - 1) / 255 < 2^272.01, |top| < 2^40.01.
//   q           q1 = floor(V / 2^254) - 1 = (top >> 22) - 1, |q1| < 2^18.02; q1 * (a 29-bit limb of t) < 2^47.02.
//   W           W = V - q1 r = (V mod 2^254) + 2^254 - q1 t  (a five-limb multiply and one signed carry pass): V mod 2^254 is in [0, 2^254) and
//               |q1 t| < 2^144.02, so W is in (2^254 - 2^144.02, 2^255 + 2^144.02), inside (0, 3r) and below 2^256: every limb ends non-negative,
//               the top limb below 2^24, and TWO conditional subtractions of r return the canonical value (the second fires only for
//               V mod 2^254 within 2^144 of 2^254; taking q1 one lower than the floor is what keeps W non-negative at the other end).
// The 32 digit sums -> nine 64-bit columns of weight 2^(29k).  lo[reg] = row (reg & 3) + 8 (reg >> 2) of the tile (the rows the lower lane of a
// sponge's lane pair receives), hi[reg] = the same + 4 (the upper lane's rows); row = digit position c.  V: anything indexable with 16 int32 entries
// (the accumulator vector on the device, an array on the host).
template <class V> FR_HD void mfma_fold_rows(int64_t* col, const V& lo, const V& hi) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const V& a = hh ? hi : lo;
                const int64_t pair = (int64_t)a[4 * q + 2 * p] + (int64_t)a[4 * q + 2 * p + 1] * 256;
                const int c = 8 * q + 4 * hh + 2 * p, k = (8 * c) / 29, sh = 8 * c - 29 * k;
                col[k] += pair * ((int64_t)1 << sh);      // pair may be negative: a product, not a shift of a signed value (undefined before C++20)
            }
}
// nine signed columns -> W = V - q1 r as nine limbs: W == V (mod r), limbs 0..7 below 2^29, the top limb below 2^24
FR_HD void mfma_finish_limbs(int64_t* col, uint32_t* l) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { col[k + 1] += col[k] >> 29; l[k] = (uint32_t)col[k] & FR_M29; }
    const int64_t top = col[8];
    const int32_t q1 = (int32_t)(top >> 22) - 1;
    l[8] = ((uint32_t)top & ((1u << 22) - 1)) + (1u << 22);
    int64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) { const int64_t d = (int64_t)l[i] - (int64_t)q1 * (int64_t)fr_p29<PF>(i) + carry; l[i] = (uint32_t)d & FR_M29; carry = d >> 29; }
    int32_t c32 = (int32_t)carry;                            // |carry| < 2^19 from here on
#pragma unroll
    for (int i = 5; i < 9; ++i) { const int32_t d = (int32_t)l[i] + c32; if (i < 8) { l[i] = (uint32_t)d & FR_M29; c32 = d >> 29; } else l[8] = (uint32_t)d; }
}
// the same -> the canonical representative of V mod r: W is below 3r, so the pack's conditional subtraction is followed by a second one
FR_HD fr_t mfma_finish_cols(int64_t* col) {
    uint32_t l[9];
    mfma_finish_limbs(col, l);
    fr_t z = fr29_pack_reduce<PF>(l);
    fr_cond_sub<PF>(z.v, 0u);
    return z;
}
// The S-box on the finish's nine limbs, with no canonical value in between: u = W + c limb by limb (c = the next round's constant as nine 29-bit limbs
// of its stored value, PoseidonDev::rc_full29), then x^5 as in fr_pow5_r29.  Bounds, for ANY u of value below 4.25 r whose limbs are below 2^30 (here
// W < 3 r + 2^146 with limbs below 2^29, the wider of the two finishes' ranges (mfma_finish_words below), and c < r with limbs below 2^29: u < 4.0001 r):
//   u^2     a doubled limb is below 2^31 (fits the 32-bit operand), a doubled cross product below 2^61, a square below 2^60; the fullest column (8) holds
//           four doubled cross products and one square: 4 * 2^61 + 2^60 = 2^63 + 2^60, and the reduction adds at most 6 * 2^58 (five non-zero limbs of r
//           above limb 0, the carry): below 2^63 + 2^60 + 2^60.6 < 2^64.  The Montgomery step leaves x2 < u^2 / 2^261 + r < (4.25^2 / 128 + 1) r < 1.15 r.
//   x2^2    limbs below 2^29: the bounds of fr29.hpp; x4 < (1.15^2 / 128 + 1) r < 1.02 r.
//   u * x4  nine products below 2^30 * 2^29 per column: 9 * 2^59 + 6 * 2^58 < 2^63; x5 < (4.25 * 1.02 / 128 + 1) r < 1.04 r: fr29_pack_reduce's ONE conditional
//           subtraction returns the canonical x^5 / 2^20 of fr_pow5_r29.
FR_HD fr29_t pow5_lazy29(const fr29_t& u) {                  // the three products alone: x5 as nine limbs, below 1.04 r, limbs below 2^29, the top limb below 2^23
    const fr29_t x2 = fr29_sqr_mont<PF>(u), x4 = fr29_sqr_mont<PF>(x2);
    return fr29_mul_mont<PF>(u, x4);
}
FR_HD fr29_t lazy29_add_c29(const uint32_t* l, const uint32_t* __restrict__ c_) {      // l + c limb by limb
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) uint32_t* cptr_t;      // wave-uniform constants on the scalar data path, as in fr_wide29_mac
    cptr_t c = (cptr_t)c_;
#else
    const uint32_t* c = c_;
#endif
    fr29_t u;
#pragma unroll
    for (int i = 0; i < 9; ++i) u.l[i] = l[i] + c[i];
    return u;
}
FR_HD fr_t sbox_lazy29(const uint32_t* l, const uint32_t* __restrict__ c) { return fr29_pack_reduce<PF>(pow5_lazy29(lazy29_add_c29(l, c)).l); }
// ---- the chain of the 8-round blocks as LAZY RESIDUES (poseidon_pair.hpp blk8_round_x / blk8_round_y): no canonical value between two S-boxes ----
// Row q's finish takes the scaled constant of the round that consumes the row INTO the nine columns (c = nine 29-bit limbs of the stored
// lambda_{q+1} c_{q+1}, KernelConsts::rc_partial_scaled29; limbs below 2^29, c < r), so the constant is off the chain.  It is added to the folded columns in
// front of the carry pass (from a temporary filled by mfma_cols_set), which is the same sum as columns that start from c.  The register allocator decides the
// form: with c as the columns' initial value, and also with the nine adds written straight from the scalars, k_hash_ds2<17, DsBatchStream, true> held 256 VGPRs
// with 2 spilled (12 B of scratch); in this form it held 252 and spilled none.
//   column      |col| < 2^61.01 + 2^29, with the carry still < 2^62; top = floor((V + c) / 2^232), |top| < 2^40.01 + 1;
//   q1          floor((V + c) / 2^254) - 1, |q1| < 2^18.02 + 1;
//   W'          V + c - q1 r = ((V + c) mod 2^254) + 2^254 - q1 t: the range of W above, (2^254 - 2^144.02, 2^255 + 2^144.02), below 2.0001 r and below 2^256,
//               limbs 0..7 below 2^29, the top limb below 2^24.
// mfma_finish_limbs is the finish as it stands: only the columns it starts from differ.  (The kernels have since moved H_q to WORD columns — mfma_finish_words
// below, the constant's eight words in front of the quotient, W' below 3 r; this limb-column form stays for the host checks and as the comparison in
// tools/partial_block8.hip.  The slot and X's side are unchanged.)
// The mailbox slot (32 bytes) holds W' as its nine limbs: limb k in bits 0..28 of word k, bits 3k..3k+2 of the top limb (24 bits = 8 x 3) in bits 29..31 of
// word k.  Two instructions per word on either side (bit-field extract + shift-or; and + shift-or), against a pack (8 words of two or three shift-ors) and an
// unpack (nine limbs of two shifts, an or and a mask) for the packed 256-bit form: the cheaper of the two layouts.
FR_HD void mfma_cols_set(int64_t* col, const uint32_t* __restrict__ c) {      // the host checks' form of the limb-column finish with a constant; no kernel calls it
#pragma unroll
    for (int k = 0; k < 9; ++k) col[k] = (int64_t)c[k];
}
FR_HD fr_t lazy29_to_slot(const uint32_t* l) {               // limbs 0..7 below 2^29, the top limb below 2^24
    fr_t z;
#pragma unroll
    for (int k = 0; k < 8; ++k) z.v[k] = l[k] | (((l[8] >> (3 * k)) & 7u) << 29);
    return z;
}
// X's side of the hand-over: u = x5 + W' limb by limb.  x5 < 1.04 r (limbs below 2^29, top below 2^23) and W' < 3.0001 r from the word-column finish
// (mfma_finish_words; 2.0001 r from mfma_finish_limbs): u < 4.05 r with limbs below 2^30, inside pow5_lazy29's contract (below 4.25 r, limbs below 2^30);
// then x2 < (4.05^2 / 128 + 1) r < 1.13 r, x4 < 1.01 r, x5 < (4.05 * 1.01 / 128 + 1) r < 1.04 r.
FR_HD fr29_t lazy29_add_slot(const fr29_t& x5, const fr_t& slot) {
    fr29_t u; uint32_t top = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { u.l[k] = x5.l[k] + (slot.v[k] & FR_M29); top |= (slot.v[k] >> 29) << (3 * k); }
    u.l[8] = x5.l[8] + top;
    return u;
}
// An S-box output as a B operand WITHOUT the conditional subtraction: x5 < 1.04 r < 1.04 (2^254 + 2^126), so byte 31 of the packed integer is at most
// floor(1.04 * 64) = 66 = 0x42; recode_signed adds 0x80 and a carry to it: at most 0xc3, no carry out of the top byte, so the 32 digits in [-128, 127] sum
// (weighted) to the integer x5 itself, which is congruent to the canonical value.  The digit-sum bounds of the products depend on the digit range alone.
FR_HD fr_t recode_lazy29(const fr29_t& x5) { return recode_signed(fr29_pack(x5.l)); }
// the fused rows' S-box with the output recoded unreduced: what a slot holds when the next product reads it as a B operand
FR_HD fr_t sbox_lazy29_recoded(const uint32_t* l, const uint32_t* __restrict__ c) { return recode_lazy29(pow5_lazy29(lazy29_add_c29(l, c))); }
// ---- the lanes between two 8-round blocks from the SIGNED residue (poseidon_pair.hpp blk8_lane_rows): a B operand needs signed bytes of SOME integer
// congruent to the lane, not the canonical one.  First the form through nine limbs (the kernels' form until the byte-domain finish below; the host checks and
// tools/partial_block8.hip keep it as the comparison).  The finish with the FLOOR quotient:
//   q           floor(V / 2^254) = top >> 22, |q| < 2^18.02 + 1;
//   W           V - q r = (V mod 2^254) - q t in (-2^144.02, 2^254 + 2^144.02): limbs 0..7 in [0, 2^29), the top limb in [-1, 2^22] as a signed word.
// fr29_pack takes bits 232..255 from the low 24 bits of the top limb, so the eight words are W's two's complement (sign-extended), and recode_signed on it
// returns W's digits: with K = 0x8080...80 it forms t = (W + K) mod 2^256 and digits t_b - 128, whose weighted sum is t - K; W + K lies in [0, 2^256) for
// -K <= W < 2^256 - K (K > 2^255, and W's top byte is at most 0x40), so t = W + K without wrap-around for either sign and the digits sum to W exactly.
FR_HD void mfma_finish_limbs_floor(int64_t* col, uint32_t* l) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { col[k + 1] += col[k] >> 29; l[k] = (uint32_t)col[k] & FR_M29; }
    const int64_t top = col[8];
    const int32_t q = (int32_t)(top >> 22);
    l[8] = (uint32_t)top & ((1u << 22) - 1);
    int64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) { const int64_t d = (int64_t)l[i] - (int64_t)q * (int64_t)fr_p29<PF>(i) + carry; l[i] = (uint32_t)d & FR_M29; carry = d >> 29; }
    int32_t c32 = (int32_t)carry;                            // |carry| < 2^19 from here on
#pragma unroll
    for (int i = 5; i < 9; ++i) { const int32_t d = (int32_t)l[i] + c32; if (i < 8) { l[i] = (uint32_t)d & FR_M29; c32 = d >> 29; } else l[8] = (uint32_t)d; }
}
FR_HD fr_t mfma_finish_recoded(int64_t* col) { uint32_t l[9]; mfma_finish_limbs_floor(col, l); return recode_signed(fr29_pack(l)); }
// ---- the same lanes finished in the BYTE domain (what blk8_lane_rows runs between two blocks): the digit sums are byte-indexed and so is the consumer, so
// the row never passes through 29-bit limbs.  Same contract as mfma_finish_recoded: eight words whose bytes, read as signed digits, sum to some W == V (mod r).
//   fold        word column k = P0 + 2^16 P1 with P0 = S_{4k} + 256 S_{4k+1}, P1 = S_{4k+2} + 256 S_{4k+3}, V = sum_k col_k 2^(32k).  The four sums of a word
//               are registers 4q..4q+3 of ONE lane's tile (rows 8q + 4h + 0..3, h = the lane's half: word 2q + h), so a lane folds what it holds and only
//               finished columns are exchanged.  Lane rows (9 K-steps): |S_c| <= 9 * 32 * 128 * 128 = 4 718 592 < 2^22.17, |P| <= 257 |S| < 2^30.18: an int32;
//               |col| <= 65537 |P| < 2^46.2.  WIDE (rows of up to 17 K-steps): |S_c| <= 8 912 896 < 2^23.09, |P| < 2^31.1: pairs in 64 bits, |col| < 2^47.1.
//   quotient    x = col_7 + (col_6 >> 32), V / 2^224 = x + f, where f in (-2^-17, 1 + 2^-17) is what the columns below contribute (col_6's low word
//               below 1, col_5 and lower |col_k| 2^(32k - 224) < 2^(47.1 - 64) each); q^ = (x + 2) >> 30.  With q = floor(V / 2^254): q <= q^ <= q + 1, and
//               |q^| < 2^17.2 (WIDE: 2^18.2).
//   one pass    t = col_k + carry + 0x80808080 - q^ t_k (k < 4: r = 2^254 + t, t below 2^126, t_k its words) - q^ 2^30 (k = 7); word_k = lo32(t) ^ 0x80808080,
//               carry = t >> 32.  |q^ t_k| < 2^50.2, |carry| < 2^19: every t inside an int64.  W = V - q^ r is in (-r - 2^145, 2^254 + 2^145), so with
//               K = 0x8080...80 > 2^255, W + K is in [0, 2^256): no carry leaves word 7 and the digits byte - 128 sum to W exactly.
// qh / carry_out (host checks): the quotient estimate and the carry out of word 7 (zero by the bound above).
template <bool WIDE = false, class V> FR_HD void mfma_word_cols(const V& a, int64_t* wc) {      // one tile's 16 sums in a lane -> its four word columns
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if constexpr (WIDE) wc[q] = ((int64_t)a[4 * q] + (int64_t)a[4 * q + 1] * 256) + ((int64_t)a[4 * q + 2] + (int64_t)a[4 * q + 3] * 256) * 65536;
        else { const int32_t p0 = a[4 * q] + a[4 * q + 1] * 256, p1 = a[4 * q + 2] + a[4 * q + 3] * 256; wc[q] = (int64_t)p0 + (int64_t)p1 * 65536; }
    }
}
FR_HD fr_t mfma_finish_bytes(const int64_t* col, int32_t* qh_out = nullptr, int64_t* carry_out = nullptr) {
    const int64_t x = col[7] + (col[6] >> 32);
    const int32_t qh = (int32_t)((x + 2) >> 30);
    fr_t z; int64_t carry = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int64_t t = col[k] + carry + (int64_t)0x80808080u;
        if (k < 4) t -= (int64_t)qh * (int64_t)PF::P(k);
        if (k == 7) t -= (int64_t)qh * ((int64_t)1 << 30);
        z.v[k] = (uint32_t)t ^ 0x80808080u; carry = t >> 32;
    }
    if (qh_out) *qh_out = qh;
    if (carry_out) *carry_out = carry;
    return z;
}
// ---- rows that end as nine limbs for an S-box, from WORD columns (poseidon_pair.hpp mfma_post_limbs: the fused full-round rows, the H_q rows, the last
// block's lane rows): folded where the sums sit like the byte-domain rows, so only finished columns cross the lane pair, and finished in one pass.
//   fold        word column k = ((S_{4k+3} 2^24 + S_{4k+2} 2^16) + S_{4k+1} 2^8) + S_{4k} as a chain of 64-bit multiply-adds (v_mad_i64_i32 on the device).  The three
//               multipliers are made opaque to the device compiler (an empty asm on scalar registers); with plain constants it rewrites the products into
//               sign extensions and 64-bit shift-adds, which is what mfma_word_cols<true> compiles to.  Rows of up to 16 + 7 K-steps:
//               |S_c| <= 23 * 32 * 128 * 128 = 12 058 624 < 2^23.53, |col| <= 16 843 009 |S| < 2^47.6.
//   constant    (the H_q rows) the eight words of a stored constant c < r are added to the columns in front of the quotient: |col| < 2^47.6 + 2^32.
//   quotient    x = col_7 + (col_6 >> 32), q^ = (x + 2) >> 30 as in mfma_finish_bytes: (V + c) / 2^224 = x + f with f in (-2^-16, 1 + 2^-16), so q <= q^ <= q + 1
//               for q = floor((V + c) / 2^254); q1 = q^ - 2 in {q - 2, q - 1}, |q1| < 2^18.6.
//   one pass    t = col_k + carry - q1 t_k (k < 4: r = 2^254 + t, t_k its words) - q1 2^30 (k = 7); word_k = lo32(t), carry = t >> 32.  |q1 t_k| < 2^50.6,
//               |q1 2^30| < 2^48.6, |carry| < 2^19.6: every t inside an int64.
//   W           V + c - q1 r = ((V + c) mod 2^254) - q t + (q - q1) r with q - q1 in {1, 2} and |q t| < 2^145: W in (r - 2^146, 3 r + 2^146), inside [0, 2^256)
//               (3 r + 2^146 = 3 * 2^254 + 3 t + 2^146 < 2^256): no carry leaves word 7 and the eight words are W itself.  fr29_unpack: limbs 0..7 below 2^29, the
//               top limb (bits 232..255) below 2^24.  One r wider at the top than mfma_finish_limbs' range; the consumers' bounds with it:
//   S-box       a fused row adds a constant below r: u < 4 r + 2^146 < 4.0001 r; the chain forms u = x5 + W' < 1.04 r + 3.0001 r < 4.05 r; limbs below 2^30
//               either way.  pow5_lazy29's column bounds depend on the limb sizes alone (unchanged); its values for ANY u below 4.25 r:
//               x2 < (4.25^2 / 128 + 1) r < 1.15 r, x4 < (1.15^2 / 128 + 1) r < 1.02 r, x5 < (4.25 * 1.02 / 128 + 1) r < 1.04 r: the packed x5's top byte is still
//               at most 0x42 (recode_lazy29) and fr29_pack_reduce's one conditional subtraction still returns the canonical value.
// qh / carry_out (host checks): the quotient estimate and the carry out of word 7 (zero by the range above).
template <class V> FR_HD void mfma_word_cols_mad(const V& a, int64_t* wc) {      // one tile's 16 sums in a lane -> its four word columns
    int32_t m8 = 1 << 8, m16 = 1 << 16, m24 = 1 << 24;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(m8), "+s"(m16), "+s"(m24));
#endif
#pragma unroll
    for (int q = 0; q < 4; ++q)
        wc[q] = (((int64_t)a[4 * q + 3] * m24 + (int64_t)a[4 * q + 2] * m16) + (int64_t)a[4 * q + 1] * m8) + (int64_t)a[4 * q];
}
FR_HD void mfma_words_add_c29(int64_t* col, const uint32_t* __restrict__ c_) {      // col += the eight words of a stored constant given as its nine 29-bit limbs
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) uint32_t* cptr_t;      // wave-uniform: the pack runs on the scalar unit
    cptr_t c = (cptr_t)c_;
#else
    const uint32_t* c = c_;
#endif
    uint32_t l[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) l[i] = c[i];
    const fr_t w = fr29_pack(l);
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k] += (int64_t)w.v[k];
}
FR_HD fr_t mfma_finish_words_packed(const int64_t* col, int32_t* qh_out = nullptr, int64_t* carry_out = nullptr) {      // -> the eight words of W
    const int64_t x = col[7] + (col[6] >> 32);
    const int32_t qh = (int32_t)((x + 2) >> 30), q1 = qh - 2;
    fr_t z; int64_t carry = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int64_t t = col[k] + carry;
        if (k < 4) t -= (int64_t)q1 * (int64_t)PF::P(k);
        if (k == 7) t -= (int64_t)q1 * ((int64_t)1 << 30);
        z.v[k] = (uint32_t)t; carry = t >> 32;
    }
    if (qh_out) *qh_out = qh;
    if (carry_out) *carry_out = carry;
    return z;
}
FR_HD void mfma_finish_words(const int64_t* col, uint32_t* l, int32_t* qh_out = nullptr, int64_t* carry_out = nullptr) {
    const fr29_t u = fr29_unpack(mfma_finish_words_packed(col, qh_out, carry_out));
#pragma unroll
    for (int i = 0; i < 9; ++i) l[i] = u.l[i];
}
// the same -> the canonical representative (the products that end canonical: one fold and exchange serves both ends of a row).  The range above is the coarse
// one; the estimate's two outcomes taken apart give W below 3 r, so TWO conditional subtractions suffice, as in mfma_finish_cols:
//   q^ = q + 1   W = (V mod 2^254) - q t + r < 2^254 + 2^145 + r < 3 r;
//   q^ = q       (x + 2) >> 30 = q means x <= (q + 1) 2^30 - 3, so V / 2^224 = x + f < (q + 1) 2^30 - 2 + 2^-16 and V mod 2^254 < 2^254 - 2^224 (2 - 2^-16);
//                W = (V mod 2^254) - q t + 2 r < 2^254 - 2^225 + 2^209 + 2^145 + 2 r < 3 r.
// (At the other end W is above 2 r - 2^226: q^ = q + 1 needs x >= (q + 1) 2^30 - 2, i.e. V mod 2^254 > 2^254 - 2^224 (2 + 2^-16).)
FR_HD fr_t mfma_finish_words_canonical(const int64_t* col) {
    fr_t z = mfma_finish_words_packed(col);
    fr_cond_sub<PF>(z.v, 0u); fr_cond_sub<PF>(z.v, 0u);
    return z;
}
// c * u for a multiplier-table entry c (nine limbs of c R' mod r, fr29_const_from) and a lazy u (limbs below 2^30, below 4 r): a column holds nine products
// below 2^59 and the reduction's 6 * 2^58: below 2^63; the result is below (4 / 128 + 1) r < 1.04 r with limbs below 2^29.
FR_HD fr29_t fr29_mul_c29(const uint32_t* __restrict__ c, const fr29_t& u) { fr_wide29 w; fr_wide29_zero(w); fr_wide29_mac(w, c, u); fr29_t r; fr_wide29_mont<PF>(w, r.l); return r; }
#if !defined(__HIP_DEVICE_COMPILE__)
// 32 digit sums in ROW order (S[c] = digit position c) -> the nine columns, as a lane of the kernels forms them: the D layout's register order of the
// rows a sponge's two lanes hold after the exchange (lo / hi above), zeroed columns, fold.
// c29 != nullptr: a constant's nine limbs are added to the folded columns, as blk8_round_y does.
inline void mfma_cols_of_sums(const int32_t* S, int64_t* col, const uint32_t* c29 = nullptr) {
    int32_t lo[16], hi[16];
    for (int reg = 0; reg < 16; ++reg) { const int row = (reg & 3) + 8 * (reg >> 2); lo[reg] = S[row]; hi[reg] = S[row + 4]; }
    for (int k = 0; k < 9; ++k) col[k] = 0;
    mfma_fold_rows(col, lo, hi);
    if (c29) { int64_t cc[9]; mfma_cols_set(cc, c29); for (int k = 0; k < 9; ++k) col[k] += cc[k]; }
}
// 32 digit sums in ROW order -> the eight word columns of the byte-domain finish, as the two lanes of a sponge form them: each lane folds the 16 registers of
// its own tile (h = 0 the lower lane, h = 1 the upper one), the lanes then exchange finished columns (word 2q + h from half h)
template <bool WIDE = false> inline void mfma_word_cols_of_sums(const int32_t* S, int64_t* col) {
    for (int h = 0; h < 2; ++h) {
        int32_t a[16]; int64_t wc[4];
        for (int reg = 0; reg < 16; ++reg) a[reg] = S[(reg & 3) + 8 * (reg >> 2) + 4 * h];
        mfma_word_cols<WIDE>(a, wc);
        for (int q = 0; q < 4; ++q) col[2 * q + h] = wc[q];
    }
}
// 32 digit sums in ROW order -> the eight word columns of the word-column finish to limbs (mfma_finish_words), in the lanes' own order: each half folds its 16
// registers by the multiply-add chain, the finished columns are exchanged, then a constant's words (c29: its nine limbs; nullptr: none) are added
inline void mfma_word_cols_mad_of_sums(const int32_t* S, int64_t* col, const uint32_t* c29 = nullptr) {
    for (int h = 0; h < 2; ++h) {
        int32_t a[16]; int64_t wc[4];
        for (int reg = 0; reg < 16; ++reg) a[reg] = S[(reg & 3) + 8 * (reg >> 2) + 4 * h];
        mfma_word_cols_mad(a, wc);
        for (int q = 0; q < 4; ++q) col[2 * q + h] = wc[q];
    }
    if (c29) mfma_words_add_c29(col, c29);
}
// sbox_lazy29's three steps with 128-bit columns, statement by statement after fr29_sqr_mont / fr29_mul_mont / fr_wide29_mont, recording the largest value any
// column holds when it is consumed (a column only grows until then): what the 64-bit columns of the kernels have to hold.  Returns x5's limbs.
struct Lazy29Wide {
    typedef unsigned __int128 u128;
    u128 max_col = 0;
    void mont(u128* w, uint32_t* l) {
        for (int k = 0; k < 9; ++k) {
            const u128 t = w[k]; if (t > max_col) max_col = t;
            const uint32_t m = (0u - (uint32_t)t) & FR_M29;
            w[k + 1] += (t + FR_M29) >> 29;
            for (int j = 1; j < 9; ++j) if (fr_p29<PF>(j) != 0) w[k + j] += (u128)m * fr_p29<PF>(j);
        }
        u128 carry = 0;
        for (int i = 0; i < 9; ++i) { const u128 v = w[9 + i] + carry; if (w[9 + i] > max_col) max_col = w[9 + i]; l[i] = i < 8 ? ((uint32_t)v & FR_M29) : (uint32_t)v; carry = v >> 29; }
    }
    fr29_t sqr(const fr29_t& a) {
        u128 w[18]; for (int k = 0; k < 18; ++k) w[k] = 0;
        for (int i = 0; i < 9; ++i) { w[2 * i] += (u128)a.l[i] * a.l[i]; for (int j = i + 1; j < 9; ++j) w[i + j] += (u128)a.l[i] * ((uint64_t)a.l[j] << 1); }
        fr29_t r; mont(w, r.l); return r;
    }
    fr29_t mul(const fr29_t& a, const fr29_t& b) {
        u128 w[18]; for (int k = 0; k < 18; ++k) w[k] = 0;
        for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) w[i + j] += (u128)a.l[i] * b.l[j];
        fr29_t r; mont(w, r.l); return r;
    }
    fr29_t pow5(const uint32_t* l, const uint32_t* c) {
        fr29_t u; for (int i = 0; i < 9; ++i) u.l[i] = l[i] + c[i];
        x2 = sqr(u); x4 = sqr(x2); return mul(u, x4);
    }
    fr29_t x2, x4;                                            // the intermediates of the last pow5, for the census of their sizes
};
#endif

}  // namespace stark
