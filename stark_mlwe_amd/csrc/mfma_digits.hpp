// stark_mlwe_amd/csrc/mfma_digits.hpp — HOST MIRROR of the scalar pieces of the int8-MFMA field products (poseidon_pair.hpp: recode_signed,
// mfma_fold_rows, mfma_finish_limbs / mfma_finish_cols, sbox_lazy29: the fold of the 32 digit sums, the signed carry pass, the product-free reduction of
// pair_apply_mds_mfma and the S-box that takes a row over in limb form),
// statement by statement, for the host-check library: the residue fragment tables (host_util.hpp mfma_frags), the fold and the finishing step are
// exercised on the CPU against the L*U rows and against big integers (tests/test_hostcheck.py, tests/test_full_round_residue_tables_host.py).  The
// bounds of every intermediate are written next to the device code.  The device keeps its own copies: routing the kernels through these templates
// compiled to a 2 % slower leaf kernel (same box, A/B), and the kernels' own results are pinned by the GPU parity tests.  Not included by any
// device translation unit.
#pragma once
#include "fr.hpp"
#include "fr29.hpp"

namespace stark {

// x (canonical) -> signed radix-256 digits in place of its bytes: add 0x80 to every byte with carries, flip every byte's top bit
// (digit b = byte b - 0x80 in [-128, 127]; x < r keeps the top byte below 0x80, so 32 digits hold it).  The int8 operand form of the MFMA product.
FR_HD fr_t recode_signed(const fr_t& x) {
    fr_t y; uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const uint64_t t = (uint64_t)x.v[i] + 0x80808080u + c; y.v[i] = (uint32_t)t ^ 0x80808080u; c = t >> 32; }
    return y;
}
// The 32 digit sums of one output -> nine 64-bit columns of weight 2^(29k).  lo[reg] = row (reg & 3) + 8 (reg >> 2) of the tile (the rows the lower lane
// of a sponge's lane pair receives), hi[reg] = the same + 4 (the upper lane's rows); row = digit position c.  Pairs of adjacent digit sums
// (|S0 + 256 S1| < 2^32.01) go into the column that holds the lower digit (shift < 29, at most two pairs per column: below 2^61.01).
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
// nine signed columns (weight 2^(29k), the total any integer V with |V| < 2^272.01) -> W = V - q1 r as nine limbs: signed carry pass,
// q1 = floor(V / 2^254) - 1, W = (V mod 2^254) + 2^254 - q1 t in (2^254 - 2^144.02, 2^255 + 2^144.02), inside (0, 3r); limbs 0..7 below 2^29, the top limb below 2^24
FR_HD void mfma_finish_limbs(int64_t* col, uint32_t* l) {
    typedef PallasFr PF;
    static_assert(fr_p29<PF>(4) < (1u << 10) && fr_p29<PF>(5) == 0 && fr_p29<PF>(6) == 0 && fr_p29<PF>(7) == 0 && fr_p29<PF>(8) == (1u << 22), "r = 2^254 + t with t below 2^126");
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
// the same -> the canonical representative of V mod r: W is below 3r, two conditional subtractions
FR_HD fr_t mfma_finish_cols(int64_t* col) {
    typedef PallasFr PF;
    uint32_t l[9];
    mfma_finish_limbs(col, l);
    fr_t z = fr29_pack_reduce<PF>(l);
    fr_cond_sub<PF>(z.v, 0u);
    return z;
}
// The S-box on the finish's nine limbs (poseidon_pair.hpp sbox_lazy29): u = l + c limb by limb, x^5 as in fr_pow5_r29.  For any u below 4r with limbs
// below 2^30 no 64-bit column overflows (bounds next to the device code) and the result is the canonical fr_pow5_r29 of u mod r.
FR_HD fr_t sbox_lazy29(const uint32_t* l, const uint32_t* c) {
    typedef PallasFr PF;
    fr29_t u;
#pragma unroll
    for (int i = 0; i < 9; ++i) u.l[i] = l[i] + c[i];
    const fr29_t x2 = fr29_sqr_mont<PF>(u), x4 = fr29_sqr_mont<PF>(x2), x5 = fr29_mul_mont<PF>(u, x4);
    return fr29_pack_reduce<PF>(x5.l);
}
#if !defined(__HIP_DEVICE_COMPILE__)
// The same three steps with 128-bit columns, statement by statement after fr29_sqr_mont / fr29_mul_mont / fr_wide29_mont, recording the largest value any
// column holds when it is consumed (a column only grows until then): what the 64-bit columns of the kernels would have to hold.  Returns x5's limbs.
struct Lazy29Wide {
    typedef unsigned __int128 u128;
    u128 max_col = 0;
    void mont(u128* w, uint32_t* l) {
        typedef PallasFr PF;
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
