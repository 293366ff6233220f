// stark_mlwe_amd/csrc/mle_dev.hpp — Mle::evaluate (channel/src/lib.rs:279-295) of many tables in a few launches on CDNA4 (gfx950).
//
// The reference folds k times, layer[i] = (1 - r_j) layer[2i] + r_j layer[2i+1], r_0 binding the least significant index bit.  Every r_j of an
// evaluation is known before the first fold, so one launch of k_mle_fold_pass folds t = min(T, rounds left) rounds of every instance: a tile of 2^t
// consecutive elements of the layer becomes ONE element of the layer t rounds on, and an evaluation is ceil(k / T) launches that read the table once.
// The fold of a tile is the multilinear form sum_i table[i] prod_s (bit s of i ? r_s : 1 - r_s), a field element whichever variable is bound first;
// every stored value is fully reduced, so the order changes no bit.  A tile is folded in three stages:
//   * lane-local, in registers: a lane owns 2^c elements (c = max(0, t - 8)) and folds them depth first, c partial results live at a time;
//   * across the lanes of a wave with shfl_xor_fr (up to six rounds): both partners compute, the lane whose bit is clear holds the result;
//   * across the four waves through 256 B of LDS (up to two rounds).
// Which elements a lane owns is the `contig` choice.  Interleaved (0): lane l of a tile owns l, l + 256, ... — every load instruction of a wave reads
// 64 consecutive elements (2 x 1 KiB, fully coalesced) and the lane-local rounds bind the tile's HIGH bits.  Contiguous (1): the lane owns 2^c
// consecutive elements, its 16-byte loads sit at a 2^c * 32 B stride, and the lane-local rounds bind the LOW bits.  tools/mle_timing.py measures one against the other.
// With t < 8 there are no lane-local rounds and a 256-thread workgroup holds 2^(8 - t) tiles.
//
// The pieces below are FR_HD: hostcheck.cpp runs the same lane geometry, local fold and wave stage in lockstep on the CPU (hc_mle_evaluate_batch).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>
#include "fr.hpp"
#include "dev_common.hpp"

namespace stark {

constexpr int kMleLogThreads = 8;                        // a workgroup is 256 threads
constexpr int kMleMinLogTile = 3, kMleMaxLogTile = 12;   // context option "mle_log_tile"
constexpr int kMleDefaultLogTile = 12;                   // fewest launches and fewest products per element; tools/mle_timing.py sweeps it
constexpr int kMleDefaultContig = 0;

// rounds per launch of a k-round evaluation with tile 2^T: T, T, ..., and what is left
inline std::vector<int> mle_pass_rounds(size_t k, int T) {
    std::vector<int> p;
    for (size_t left = k; left; left -= (size_t)p.back()) p.push_back((int)std::min<size_t>((size_t)T, left));
    return p;
}
inline int mle_local_rounds(int t) { return std::max(0, t - kMleLogThreads); }

FR_HD fr_t mle_fold1(const fr_t& a, const fr_t& b, const fr_t& r) { return fr_add<PallasFr>(a, fr_mul<PallasFr>(r, fr_sub<PallasFr>(b, a))); }

// Thread g of a pass (counted over the whole layer) with t rounds, c of them lane-local and x = t - c across threads.
struct MleLane {
    uint64_t tile, first, stride;      // the tile it works on, its first element and the distance between its 2^c elements
    int local0, cross0;                // rounds r[local0 ..] are the lane-local ones, r[cross0 ..] those across threads
};
FR_HD MleLane mle_lane(uint64_t g, int t, int c, bool contig) {
    const int x = t - c; const uint64_t lane = g & ((1ull << x) - 1);
    MleLane L; L.tile = g >> x;
    L.first = (L.tile << t) + (contig ? lane << c : lane); L.stride = contig ? 1 : 1ull << x;
    L.local0 = contig ? 0 : x; L.cross0 = contig ? c : 0;
    return L;
}
// the fold of the 2^C elements p[0], p[stride], ... with r[0 .. C), depth first
template <int C> FR_HD fr_t mle_fold_local(const fr_t* p, uint64_t stride, const fr_t* r) {
    if constexpr (C == 0) return ldg(p);
    else {
        const fr_t a = mle_fold_local<C - 1>(p, stride, r), b = mle_fold_local<C - 1>(p + (stride << (C - 1)), stride, r);
        return mle_fold1(a, b, r[C - 1]);
    }
}
// The wave stage (x > 6): w[0 .. 4) are what lane 0 of each wave holds after six rounds, r6 / r7 the rounds left; output o < 4 >> (x - 6) of the workgroup.
// (selects, not w[2 * o]: an array indexed at run time would live in scratch memory on the device)
FR_HD fr_t mle_fold_waves(const fr_t* w, int x, int o, const fr_t& r6, const fr_t& r7) {
    if (x == 7) return mle_fold1(o ? w[2] : w[0], o ? w[3] : w[1], r6);
    return mle_fold1(mle_fold1(w[0], w[1], r6), mle_fold1(w[2], w[3], r6), r7);
}

#if defined(__HIPCC__)
// One pass: instance b = b0 + blockIdx.y reads its layer of `len` elements at ptrs[b] (the caller's table) or layers + b * len (scratch), folds rounds
// j0 .. j0 + t of its point r[b * k ..] and writes next[b * (len >> t) + tile].  gridDim.x * 256 threads cover the len >> C lanes of a layer.
template <int C, bool CONTIG>
__global__ void __launch_bounds__(256) k_mle_fold_pass(const fr_t* const* __restrict__ ptrs, const fr_t* __restrict__ layers, uint64_t len, int t, uint64_t b0,
                                                       const fr_t* __restrict__ r, uint64_t k, uint64_t j0, fr_t* __restrict__ next) {
    __shared__ uint4 red[2 * 4];
    const int x = t - C;
    const uint64_t b = b0 + blockIdx.y;
    const fr_t* layer = ptrs ? ptrs[b] : layers + b * len;
    const fr_t* rr = r + b * k + j0;
    const MleLane L = mle_lane((uint64_t)blockIdx.x * blockDim.x + threadIdx.x, t, C, CONTIG);
    const bool live = L.first < len;                     // whole tiles: len is a multiple of 2^t
    fr_t rl[C > 0 ? C : 1];
#pragma unroll
    for (int i = 0; i < C; ++i) rl[i] = ldg(rr + L.local0 + i);
    fr_t v = live ? mle_fold_local<C>(layer + L.first, L.stride, rl) : fr_zero<PallasFr>();
#pragma unroll
    for (int s = 0; s < 6; ++s)
        if (s < x) v = mle_fold1(v, shfl_xor_fr(v, 1 << s), ldg(rr + L.cross0 + s));
    fr_t* dst = next + b * (len >> t);
    if (x <= 6) {
        if (live && (threadIdx.x & ((1u << x) - 1)) == 0) stg(dst + L.tile, v);
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { red[2 * wave] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]); red[2 * wave + 1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]); }
    __syncthreads();
    const uint64_t tile = ((uint64_t)blockIdx.x << (kMleLogThreads - x)) + threadIdx.x;      // x = 7: two tiles per workgroup, x = 8: one
    if ((int)threadIdx.x < (4 >> (x - 6)) && (tile << t) < len) {
        fr_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const uint4 lo = red[2 * i], hi = red[2 * i + 1]; w[i].v[0] = lo.x; w[i].v[1] = lo.y; w[i].v[2] = lo.z; w[i].v[3] = lo.w; w[i].v[4] = hi.x; w[i].v[5] = hi.y; w[i].v[6] = hi.z; w[i].v[7] = hi.w; }
        stg(dst + tile, mle_fold_waves(w, x, (int)threadIdx.x, ldg(rr + L.cross0 + 6), x == 8 ? ldg(rr + L.cross0 + 7) : fr_zero<PallasFr>()));
    }
}
#endif  // __HIPCC__

}  // namespace stark
