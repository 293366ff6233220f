// stark_mlwe_amd/csrc/mfma_digits.hpp — the scalar pieces of the int8-MFMA field products, ONE definition for device and host: the signed recoding of an
// operand, the fold of a row's 32 digit sums, the product-free finish (to nine limbs, or canonical) and the S-box that takes a row over in limb form.
// poseidon_pair.hpp includes it for the t = 17 wave-pair kernels (exchange and tile handling stay there); hostcheck.cpp and tools/mfma_finish_check.cpp
// run the same statements on the CPU against the L*U rows and against big integers (tests/test_hostcheck.py,
// tests/test_full_round_residue_tables_host.py, tests/test_limb_handover_host.py).  The host-only part at the end: the row-order entry of the fold
// (mfma_cols_of_sums) and the 128-bit column census of the S-box (Lazy29Wide).
#pragma once
#include "fr.hpp"
#include "fr29.hpp"

namespace stark {

typedef PallasFr PF;
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
// of its stored value, PoseidonDev::rc_full29), then x^5 as in fr_pow5_r29.  Bounds, for ANY u of value below 4r whose limbs are below 2^30 (here W < 3r
// with limbs below 2^29 and c < r with limbs below 2^29):
//   u^2     a doubled limb is below 2^31 (fits the 32-bit operand), a doubled cross product below 2^61, a square below 2^60; the fullest column (8) holds
//           four doubled cross products and one square: 4 * 2^61 + 2^60 = 2^63 + 2^60, and the reduction adds at most 6 * 2^58 (five non-zero limbs of r
//           above limb 0, the carry): below 2^63 + 2^60 + 2^60.6 < 2^64.  The Montgomery step leaves x2 < u^2 / 2^261 + r < (16 / 128 + 1) r < 1.13 r.
//   x2^2    limbs below 2^29: the bounds of fr29.hpp; x4 < 1.01 r.
//   u * x4  nine products below 2^30 * 2^29 per column: 9 * 2^59 + 6 * 2^58 < 2^63; x5 < (4 * 1.01 / 128 + 1) r < 1.04 r: fr29_pack_reduce's ONE conditional
//           subtraction returns the canonical x^5 / 2^20 of fr_pow5_r29.
FR_HD fr_t sbox_lazy29(const uint32_t* l, const uint32_t* __restrict__ c_) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) uint32_t* cptr_t;      // wave-uniform constants on the scalar data path, as in fr_wide29_mac
    cptr_t c = (cptr_t)c_;
#else
    const uint32_t* c = c_;
#endif
    fr29_t u;
#pragma unroll
    for (int i = 0; i < 9; ++i) u.l[i] = l[i] + c[i];
    const fr29_t x2 = fr29_sqr_mont<PF>(u), x4 = fr29_sqr_mont<PF>(x2), x5 = fr29_mul_mont<PF>(u, x4);
    return fr29_pack_reduce<PF>(x5.l);
}
#if !defined(__HIP_DEVICE_COMPILE__)
// 32 digit sums in ROW order (S[c] = digit position c) -> the nine columns, as a lane of the kernels forms them: the D layout's register order of the
// rows a sponge's two lanes hold after the exchange (lo / hi above), zeroed columns, fold.
inline void mfma_cols_of_sums(const int32_t* S, int64_t* col) {
    int32_t lo[16], hi[16];
    for (int reg = 0; reg < 16; ++reg) { const int row = (reg & 3) + 8 * (reg >> 2); lo[reg] = S[row]; hi[reg] = S[row + 4]; }
    for (int k = 0; k < 9; ++k) col[k] = 0;
    mfma_fold_rows(col, lo, hi);
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
        const fr29_t x2 = sqr(u), x4 = sqr(x2); return mul(u, x4);
    }
};
#endif

}  // namespace stark
