// tools/mfma_mds.hip — PROTOTYPE, not product code: y = M * x (dense 17 x 17 over Pallas Fr, Montgomery form) for 64 sponges per wave pair
// END TO END on the matrix cores, RESIDUE-TABLE form: signed radix-256 recoding of the state in LDS, v_mfma_i32_32x32x32_i8 against stored fragments
// of C[i][e][b] = (M[i][e] * 256^b) mod r (one 32-row tile per output: 34 MFMAs), the two-lane exchange (v_permlane32_swap), folding of the 32
// digit sums into 29-bit columns, signed carry pass, product-free reduction of the bits above 2^254, canonical store (form "limb columns"); beside it the
// row finished from WORD columns (form "word columns": mfma_digits.hpp mfma_word_cols_mad / mfma_finish_words_canonical — each lane folds the sums it holds by
// a multiply-add chain, four 64-bit columns per tile cross the lane pair, one pass over eight words).  Both forms are host-checked and timed alternately.  The former form (Toeplitz
// fragments of the constants' digits, 68 MFMAs per output, a Montgomery step) measured 95 k SIMD-cycles per product with this same harness
// (profiles/r02_mfma_mds_end_to_end_prototype.jsonl).  The result is checked against sum_e M[i][e] * x_e computed with the product's portable field code.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I stark_mlwe_amd/csrc tools/mfma_mds.hip -o tools/bin/mfma_mds
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "fr.hpp"
#include "fr29.hpp"
#include "mfma_digits.hpp"
using namespace stark;
typedef PallasFr F;
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
constexpr int T = 17;

// After the half exchange a lane holds all 32 digit sums of ITS sponge: lo[reg] = rows (reg&3) + 8(reg>>2) of the tile (the lower lane's
// rows), hi[reg] = the same + 4 (the upper lane's rows); row = digit position c.  Pairs of adjacent digits go into the 64-bit
// column of weight 2^(29k) that holds the lower one (shift < 29, pair below 2^33: no overflow).
__device__ __forceinline__ void fold_rows(int64_t* col, const v16i& lo, const v16i& hi) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const v16i& a = hh ? hi : lo;
                const int64_t pair = (int64_t)a[4 * q + 2 * p] + (int64_t)a[4 * q + 2 * p + 1] * 256;
                const int c = 8 * q + 4 * hh + 2 * p, k = (8 * c) / 29, sh = 8 * c - 29 * k;
                col[k] += pair * ((int64_t)1 << sh);
            }
}
// nine signed columns -> canonical: signed carry pass, q1 = floor(V / 2^254) - 1, W = V - q1 r = (V mod 2^254) + 2^254 - q1 t in (0, 3r) (r = 2^254 + t),
// two conditional subtractions (bounds: poseidon_pair.hpp)
__device__ __forceinline__ fr_t finish_cols(int64_t* col) {
    uint32_t l[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) { col[k + 1] += col[k] >> 29; l[k] = (uint32_t)col[k] & FR_M29; }
    const int64_t top = col[8];
    const int32_t q1 = (int32_t)(top >> 22) - 1;
    l[8] = ((uint32_t)top & ((1u << 22) - 1)) + (1u << 22);
    int64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) { const int64_t d = (int64_t)l[i] - (int64_t)q1 * (int64_t)fr_p29<F>(i) + carry; l[i] = (uint32_t)d & FR_M29; carry = d >> 29; }
    int32_t c32 = (int32_t)carry;
#pragma unroll
    for (int i = 5; i < 9; ++i) { const int32_t d = (int32_t)l[i] + c32; if (i < 8) { l[i] = (uint32_t)d & FR_M29; c32 = d >> 29; } else l[8] = (uint32_t)d; }
    fr_t z = fr29_pack_reduce<F>(l);
    fr_cond_sub<F>(z.v, 0u);
    return z;
}
template <int FORM>                                       // 0: limb columns (16 swaps, fold into nine columns, carry pass); 1: word columns (fold, 8 swaps, one pass)
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) k_mds(const v4i* __restrict__ Atab, const fr_t* __restrict__ X, fr_t* __restrict__ Y, int reps) {
    __shared__ uint4 st[T * 2 * 64];
    const int lane = threadIdx.x & 63, h = lane >> 5; const bool isY = threadIdx.x >= 64;
    const size_t b0 = (size_t)blockIdx.x * T * 64;
    for (int e = isY ? 1 : 0; e < T; e += 2) {       // stage the recoded state: slot (2e + half)[sponge]
        const fr_t x = recode_signed(X[b0 + (size_t)e * 64 + lane]);
        st[(2 * e) * 64 + lane] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]); st[(2 * e + 1) * 64 + lane] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
    }
    __syncthreads();
    v4i b[T][2];
#pragma unroll
    for (int e = 0; e < T; ++e)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) { const uint4 u = st[(2 * e + h) * 64 + 32 * ct + (lane & 31)]; b[e][ct] = v4i{(int)u.x, (int)u.y, (int)u.z, (int)u.w}; }
    __syncthreads();
    for (int rep = 0; rep < reps; ++rep)
#pragma unroll 1
    for (int i = isY ? 1 : 0; i < T; i += 2) {
        v16i acc[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0;
        const v4i* Ai = Atab + (size_t)i * T * 64 + lane;
#pragma unroll
        for (int e = 0; e < T; ++e) {
            const v4i a = Ai[(size_t)e * 64];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[e][ct], acc[ct], 0, 0, 0);
        }
        fr_t y;
        if constexpr (FORM == 1) {
            // each lane folds its own 16 sums of either tile into four word columns; swap(tile 0's column, tile 1's column) hands the lower lane word 2q + 1 of ITS
            // sponge and the upper lane word 2q of its own
            int64_t c0[4], c1[4], col[8];
            mfma_word_cols_mad(acc[0], c0); mfma_word_cols_mad(acc[1], c1);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)(uint64_t)c0[q], (unsigned)(uint64_t)c1[q], false, false);
                const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)((uint64_t)c0[q] >> 32), (unsigned)((uint64_t)c1[q] >> 32), false, false);
                col[2 * q] = (int64_t)((uint64_t)lo[0] | ((uint64_t)hi[0] << 32)); col[2 * q + 1] = (int64_t)((uint64_t)lo[1] | ((uint64_t)hi[1] << 32));
            }
            y = mfma_finish_words_canonical(col);
        } else {
            // half exchange: lane l (< 32) owns sponge l = column tile 0, lane 32 + l owns sponge 32 + l = column tile 1.  swap(vdst = tile 0, src0 = tile 1)
            // gives the lower lane the upper lane's tile-0 rows and the upper lane the lower lane's tile-1 rows: afterwards r[0] = the lower rows, r[1] = the upper rows of the own sponge
            v16i lo, hi;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const auto sw = __builtin_amdgcn_permlane32_swap((unsigned)acc[0][r], (unsigned)acc[1][r], false, false);
                lo[r] = (int)sw[0]; hi[r] = (int)sw[1];
            }
            int64_t col[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) col[k] = 0;
            fold_rows(col, lo, hi);
            y = finish_cols(col);
        }
        if (rep == 0) Y[b0 + (size_t)i * 64 + lane] = y;
    }
}

int main() {
    hipDeviceProp_t prop; (void)hipGetDeviceProperties(&prop, 0); const int cus = prop.multiProcessorCount;
    uint64_t s = 0x243f6a8885a308d3ull; auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); };
    auto rand_fr = [&]() { fr_t x; for (int i = 0; i < 8; ++i) x.v[i] = rnd(); x.v[7] &= 0x3fffffffu; return x; };
    std::vector<fr_t> M((size_t)T * T); for (auto& m : M) m = rand_fr();
    M[0] = fr_zero<F>(); for (int i = 0; i < 8; ++i) M[1].v[i] = F::P(i); M[1].v[0] -= 1;       // edge constants: 0 and r - 1
    // residue fragments: for every (i, e) and input digit position b the signed digits d_b[0..31] of (M[i][e] * 256^b) mod r (M's logical value: the
    // Montgomery form times 256^b, out of Montgomery form); lane (row c = l & 31, k half kh = l >> 5), byte j <-> digit c of position b = 16 kh + j
    std::vector<int8_t> A((size_t)T * T * 64 * 16, 0);
    const fr_t k256 = fr_from_u64<F>(256);
    for (int i = 0; i < T; ++i) for (int e = 0; e < T; ++e) {
        fr_t g = M[(size_t)i * T + e]; int8_t d[32][32];
        for (int b = 0; b < 32; ++b, g = fr_mul_portable<F>(g, k256)) {
            const fr_t c = fr_to_canonical<F>(g); uint8_t by[32]; memcpy(by, c.v, 32); int cy = 0;
            for (int k = 0; k < 32; ++k) { const int v = by[k] + 0x80 + cy; cy = v >> 8; d[b][k] = (int8_t)((v & 0xff) - 0x80); }
            if (cy) { fprintf(stderr, "constant digit overflow\n"); return 1; }
        }
        for (int l = 0; l < 64; ++l) for (int j = 0; j < 16; ++j) A[((((size_t)i * T + e) * 64 + l) * 16) + j] = d[16 * (l >> 5) + j][l & 31];
    }
    const int batches = cus * 8;
    std::vector<fr_t> X((size_t)batches * T * 64); for (auto& x : X) x = rand_fr();
    for (int i = 0; i < 8; ++i) X[5].v[i] = F::P(i); X[5].v[0] -= 1; X[7] = fr_zero<F>();     // r - 1 and 0 among the inputs
    v4i* dA; fr_t *dX, *dY; (void)hipMalloc(&dA, A.size()); (void)hipMalloc(&dX, X.size() * 32); (void)hipMalloc(&dY, X.size() * 32);
    (void)hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice); (void)hipMemcpy(dX, X.data(), X.size() * 32, hipMemcpyHostToDevice);
    struct Form { const char* name; void (*kernel)(const v4i*, const fr_t*, fr_t*, int); };
    const Form forms[] = {{"limb columns: 16 swaps, fold into nine 29-bit columns, carry pass, finish", k_mds<0>}, {"word columns: multiply-add fold, 8 swaps, one pass over eight words", k_mds<1>}};
    std::vector<fr_t> Y(X.size());
    for (const Form& f : forms) {
        if (hipMemset(dY, 0xff, Y.size() * 32) != hipSuccess) return 1;
        hipLaunchKernelGGL(f.kernel, dim3(batches), dim3(128), 0, 0, dA, dX, dY, 1);
        if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); return 1; }
        (void)hipMemcpy(Y.data(), dY, Y.size() * 32, hipMemcpyDeviceToHost);
        long bad = 0;
        for (int bt = 0; bt < batches; bt += 97) for (int n = 0; n < 64; ++n) for (int i = 0; i < T; ++i) {
            fr_t acc = fr_zero<F>();
            for (int e = 0; e < T; ++e) acc = fr_add<F>(acc, fr_mul_portable<F>(M[(size_t)i * T + e], X[((size_t)bt * T + e) * 64 + n]));
            if (!fr_eq(acc, Y[((size_t)bt * T + i) * 64 + n])) { if (bad < 5) fprintf(stderr, "%s: mismatch batch %d sponge %d row %d\n", f.name, bt, n, i); ++bad; }
        }
        printf("{\"check\": \"y = M x (mod r) for all 64 sponges of sampled batches, incl. constants 0 and r-1, inputs 0 and r-1\", \"form\": \"%s\", \"mismatches\": %ld}\n", f.name, bad);
        if (bad) return 1;
    }
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); const int reps = 8, rounds = 6; float best[2] = {1e9f, 1e9f}, worst[2] = {0.f, 0.f};
    for (int r = 0; r < rounds; ++r) for (int f = 0; f < 2; ++f) {       // the forms alternate; the first round warms the tables and is not counted
        (void)hipEventRecord(e0); hipLaunchKernelGGL(forms[f].kernel, dim3(batches), dim3(128), 0, 0, dA, dX, dY, reps); (void)hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) { fprintf(stderr, "kernel failed\n"); return 1; }
        float ms; (void)hipEventElapsedTime(&ms, e0, e1); if (r > 0) { if (ms < best[f]) best[f] = ms; if (ms > worst[f]) worst[f] = ms; } }
    const double products = (double)batches * reps;
    for (int f = 0; f < 2; ++f)
        printf("{\"kernel\": \"dense 17x17 product of 64 sponges END TO END (recode, MFMA of residue tables, exchange, fold, product-free reduction, canonical), wave pair\", \"form\": \"%s\", \"ms\": %.3f, \"us_per_product_per_cu\": %.2f, "
               "\"simd_cycles_per_product_at_2.4GHz\": {\"min\": %.0f, \"max\": %.0f}, \"runs\": %d, \"toeplitz_form_simd_cycles_per_product\": \"~95000\", \"valu_form_simd_cycles_per_product\": \"~180000\"}\n",
               forms[f].name, best[f], best[f] * 1e3 / (products / cus), best[f] * 1e-3 * 2.4e9 * cus * 4 / products, worst[f] * 1e-3 * 2.4e9 * cus * 4 / products, rounds - 1);
    return 0;
}
