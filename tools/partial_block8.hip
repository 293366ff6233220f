// tools/partial_block8.hip — PROTOTYPE, not product code: 8 partial rounds of the t = 17 Poseidon permutation for 64 sponges per wave pair, in the two forms the
// product contains.
//   form 4 : the shipped block-of-4 code, twice — pair_permute_blk4<17> of poseidon_pair.hpp itself, run with rf = 0 and rp = 8 (no full rounds);
//   form 8 : the product's pair_block8 (poseidon_pair.hpp, where the schedule is described), run as a permutation's only block with canonical ends, for several
//            shares of the lane rows (NLX).  The one product by 1 / lambda_8 that brings X_8 back runs in the checked repetition only: a permutation pays it once
//            per eight blocks.
// LDS stays at PairCfg<17>::lds_bytes() = 40 KiB.  The host checks every form against the sparse rounds in the portable field code (0 and r - 1 among the inputs)
// and requires zero mismatches; then the forms are timed alternately in one process, the state reloaded from memory for every repetition.
// Superseded forms this tool once compared, each last held by commit ecb653d, with the file that keeps its numbers:
//   former     (Gamma terms on the vector ALU)                          profiles/partial_block8_gamma_rows_prototype.jsonl
//   piped      (wave Y pipelined across the round barrier)              profiles/partial_block8_gamma_rows_prototype.jsonl
//   unscaled   (a_q y_q product in every round)                         profiles/partial_block8_scaled_chain_prototype.jsonl
//   canonical  (a canonical chain value in every round)                 profiles/partial_block8_lazy_residue_prototype.jsonl
//   limbfinish (lanes between two blocks through nine 29-bit limbs)     profiles/partial_block8_byte_finish_prototype.jsonl
//   limbrows   (H_q and fused lane rows through nine limb columns)      profiles/partial_block8_word_fold_prototype.jsonl
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

// The scaled tables of block 0 (blk8s_*, the unit fragment); src29: lambda_q c_q of rounds 0..7 as nine limbs each and a ninth entry of zeros (the block is
// followed by no round here: rc_partial_scaled29 of an rp = 8 set); unscale8: 1 / lambda_8 as a multiplier-table entry (block 0 ends at round 8; the product's
// table holds 1 / lambda_rp).  "rep & blkmask" (always block 0) keeps the fragment addresses changing from one pass to the next as in a permutation's loop over
// its blocks, so the compiler cannot hoist all of them out of the repetition loop (it did, and spilled 200 registers for them).
struct ProtoTabs { const mfma_v4i* sefrag; const mfma_v4i* slfrag; const mfma_v4i* unit; const mfma_v4i* sgfrag; const uint32_t* src29; const uint32_t* unscale8; int blkmask; };

template <int NLX>
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
        const Blk8Tabs Tb{Tp.sefrag + (size_t)blk * 8 * 16 * 64, Tp.slfrag + (size_t)blk * 16 * 8 * 64, Tp.unit, Tp.sgfrag + (size_t)blk * 28 * 64, c29(Tp.src29, 1)};
        fr29_t u = fr29_unpack(s0);
        if (!s.isY) u = lazy29_add_c29(u.l, c29(Tp.src29, 0));          // as pair_permute_blk8 enters the partial rounds
        pair_block8<NLX>(s, Tb, u, LaneEnd::Canonical);
        if (rep == 0) {
            if (!s.isY) stg(Y + b0 + s.lane, fr29_pack_reduce<PF>(fr29_mul_c29(Tp.unscale8, u).l));      // lambda_8 X_8 (lazy) -> X_8
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
        pair_permute_blk4<17>(s, P, false);            // rf = 0, rp = 8: two blocks of 4 partial rounds, ends with a barrier
        if (rep == 0) for (int j = s.isY ? 9 : 0; j <= (s.isY ? 16 : 8); ++j) stg(Y + b0 + (size_t)j * 64 + s.lane, s.ld(j));
        __syncthreads();
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------
static fr_t canon(fr_t x) { for (int k = 0; k < 3; ++k) fr_cond_sub<host::PF>(x.v, 0u); return x; }   // form 4 leaves its lanes below 2.7 r (pair_lane_update)
template <class Tp> static Tp* to_dev(const void* p, size_t bytes) { void* d = nullptr; if (hipMalloc(&d, bytes) != hipSuccess || hipMemcpy(d, p, bytes, hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "device copy failed\n"); exit(1); } return (Tp*)d; }

struct Form { const char* name; void (*launch)(int batches, int reps); };
static ProtoTabs g_tb; static PoseidonDev g_p; static const fr_t* g_x; static fr_t* g_y;
template <int NLX> static void launch8(int batches, int reps) { hipLaunchKernelGGL((k_block8<NLX>), dim3(batches), dim3(128), PairCfg<17>::lds_bytes(), 0, g_tb, g_x, g_y, reps); }
static void launch4(int batches, int reps) { hipLaunchKernelGGL(k_block4x2, dim3(batches), dim3(128), PairCfg<17>::lds_bytes(), 0, g_p, g_x, g_y, reps); }

int main() {
    hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
    const int cus = prop.multiProcessorCount;
    const host::KernelConsts K = host::make_kernel_consts(host::consts_for_width(T));
    if (!K.ok) { fprintf(stderr, "constants failed\n"); return 1; }
    // the product's tables (host_util.hpp blk8s_*); block 0 = rounds 0..7
    if (K.blk8s_efrag.empty()) { fprintf(stderr, "no block-8 tables\n"); return 1; }
    g_tb.unit = to_dev<mfma_v4i>(K.blk8_lfrag.data() + K.blk8_lfrag.size() - 1024, 1024);
    g_tb.sefrag = to_dev<mfma_v4i>(K.blk8s_efrag.data(), K.blk8s_efrag.size()); g_tb.slfrag = to_dev<mfma_v4i>(K.blk8s_lfrag.data(), K.blk8s_lfrag.size());
    g_tb.sgfrag = to_dev<mfma_v4i>(K.blk8s_gfrag.data(), K.blk8s_gfrag.size());
    { std::vector<uint32_t> c29v(K.rc_partial_scaled29.begin(), K.rc_partial_scaled29.begin() + 9 * 9); for (int i = 0; i < 9; ++i) c29v[72 + i] = 0; g_tb.src29 = to_dev<uint32_t>(c29v.data(), c29v.size() * 4); }
    { uint32_t u8[9]; fr29_const_from<host::PF>(fr_inv<host::PF>(K.blk8_lambda[8]), u8); g_tb.unscale8 = to_dev<uint32_t>(u8, sizeof u8); }
    g_tb.blkmask = 0;
    memset(&g_p, 0, sizeof g_p);
    g_p.t = T; g_p.rf = 0; g_p.rp = 8; g_p.rc_partial = to_dev<fr_t>(K.rc_partial.data(), K.rc_partial.size() * sizeof(fr_t));
    g_p.sparse29 = to_dev<uint32_t>(K.sparse29.data(), K.sparse29.size() * 4); g_p.gamma29 = to_dev<uint32_t>(K.gamma29.data(), K.gamma29.size() * 4);

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
        {"block4 x 2 (shipped pair_permute_blk4<17>, rf = 0, rp = 8)", launch4},
        {"block8, Gamma K-steps, chain scaled, lazy residues, NLX=8", launch8<8>},
        {"block8, Gamma K-steps, chain scaled, lazy residues, NLX=7", launch8<7>},
        {"block8, Gamma K-steps, chain scaled, lazy residues, NLX=9", launch8<9>},
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
            if (!fr_eq(ref[(si * T + e) * 64 + n], canon(Y[((size_t)sample[si] * T + e) * 64 + n]))) { if (bad < 5) fprintf(stderr, "%s: mismatch batch %d sponge %d element %d\n", forms[f].name, sample[si], n, e); ++bad; }
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
