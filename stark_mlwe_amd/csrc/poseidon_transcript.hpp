// stark_mlwe_amd/csrc/poseidon_transcript.hpp — the streaming transcript (transcript/src/lib.rs:79-101, lazy duplex) as kernels: one device-resident
// transcript (k_tr_stream, k_tr_stream_chain) or a batch of them (k_tr_batch, k_tr_batch_chain: TrBatchStream), each on one wave
// (poseidon_coop.hpp) or on five (poseidon_chain.hpp).  Launched by tr_stream_on / tr_batch_on (capi_poseidon.hip).
#pragma once
#include "poseidon_coop.hpp"
#include "poseidon_chain.hpp"
#include "poseidon_streams.hpp"

#if defined(__HIPCC__)
namespace {
using namespace stark;
// The streaming transcript (transcript/src/lib.rs:79-101) on one wave: state[17] and the rate cursor live in device memory between
// launches; absorbs `n` queued fields with the lazy permute-on-full rule, then (finish) permutes and squeezes state[0].
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) k_tr_stream(PoseidonDev P, fr_t* __restrict__ state, uint32_t* __restrict__ pos_io,
                                                                                           const fr_t* __restrict__ fields, uint64_t n, int finish, fr_t* __restrict__ out) {
    extern __shared__ uint4 lds[];
    CoopLds L = coop_setup<17>(lds, P);
    const int lane = threadIdx.x;
    fr_t s = lane < 17 ? ldg(state + lane) : fr_zero<PF>();
    uint32_t pos = *pos_io;
    for (uint64_t i = 0; i < n;) {
        if (pos == 16) { s = coop_permute<17>(s, P, L, lane); pos = 0; }                 // only before absorbing more (lazy)
        const uint64_t take = (16 - pos) < (n - i) ? (16 - pos) : (n - i);
        if ((uint32_t)lane >= pos && (uint64_t)lane < pos + take) s = fr_add<PF>(s, ldg(fields + i + (lane - pos)));
        pos += (uint32_t)take; i += take;
    }
    if (finish) { s = coop_permute<17>(s, P, L, lane); pos = 0; }
    if (lane < 17) stg(state + lane, s);
    if (lane == 0) { *pos_io = pos; if (out) stg(out, s); }
}

// The same on the five waves of poseidon_chain.hpp (72 us per permutation instead of 142 us): the stored cursor becomes `pos` leading no-op elements of
// the stream, so that the block boundaries — and with them the lazy permutations — fall where k_tr_stream puts them.
__global__ void __launch_bounds__(320) __attribute__((amdgpu_waves_per_eu(1, 2))) k_tr_stream_chain(PoseidonDev P, row::Consts RK, fr_t* __restrict__ state, uint32_t* __restrict__ pos_io,
                                                                                                  const fr_t* __restrict__ fields, uint64_t n, int finish, fr_t* __restrict__ out) {
    extern __shared__ uint4 lds[];
    const uint32_t pos = *pos_io;                                                           // every thread reads it before thread 0 writes it back (barriers in between)
    const size_t total = (size_t)pos + n;
    chain_sponge_ex(P, RK, lds, total, fr_zero<PF>(), [&](size_t q) -> fr_t { return q < pos ? fr_zero<PF>() : ldg(fields + (q - pos)); },
                    finish ? out : (fr_t*)nullptr, state, finish != 0, state);
    if (threadIdx.x == 0) *pos_io = finish ? 0u : (total ? (uint32_t)(total - 16 * ((total - 1) / 16)) : 0u);
}

// B transcripts (TrBatchStream), one wave each: k_tr_stream's absorb loop per segment, the elements gathered from the pools.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) k_tr_batch(PoseidonDev P, TrBatchStream T) {
    extern __shared__ uint4 lds[];
    CoopLds L = coop_setup<17>(lds, P);
    const int lane = threadIdx.x;
    const size_t a = blockIdx.x, b = T.instance(a); const bool fresh = T.resets(a);
    fr_t s = fresh ? (lane == 16 ? T.init_cap : fr_zero<PF>()) : (lane < 17 ? ldg(T.state + 17 * b + lane) : fr_zero<PF>());
    uint32_t pos = fresh ? 0u : T.pos[b];
    for (size_t sg = 0; sg < T.nseg; ++sg) {
        const size_t seg = a * T.nseg + sg;
        const uint64_t e0 = T.el_off[seg], n = T.el_off[seg + 1] - e0;
        for (uint64_t i = 0; i < n;) {
            if (pos == 16) { s = coop_permute<17>(s, P, L, lane); pos = 0; }                 // only before absorbing more (lazy)
            const uint64_t take = (16 - pos) < (n - i) ? (16 - pos) : (n - i);
            if ((uint32_t)lane >= pos && (uint64_t)lane < pos + take) s = fr_add<PF>(s, T.elem(e0 + i + (lane - pos)));
            pos += (uint32_t)take; i += take;
        }
        if (T.finishes(sg)) { s = coop_permute<17>(s, P, L, lane); pos = 0; if (lane == 0) stg(T.out + seg, s); }
    }
    if (lane < 17) stg(T.state + 17 * b + lane, s);
    if (lane == 0) T.pos[b] = pos;
}
// The same on five waves: segment `sg` of every active instance, as k_tr_stream_chain runs it (the stored cursor becomes leading no-op
// elements, so the lazy permutations fall where the one-wave form puts them; a finished segment leaves the cursor at 0).  One launch per
// segment index: a loop over the segments inside this kernel raises it from 159 to 214 VGPRs (k_tr_stream_chain: 157).
__global__ void __launch_bounds__(320) __attribute__((amdgpu_waves_per_eu(1, 2))) k_tr_batch_chain(PoseidonDev P, row::Consts RK, TrBatchStream T, uint32_t sg) {
    extern __shared__ uint4 lds[];
    const size_t a = blockIdx.x, b = T.instance(a), seg = a * T.nseg + sg;
    const bool fresh = T.resets(a) && sg == 0;
    fr_t* st = T.state + 17 * b;
    const uint32_t lead = fresh ? 0u : T.pos[b];                                            // every thread reads it before thread 0 writes it back (barriers in between)
    const uint32_t e0 = T.el_off[seg];
    const size_t total = (size_t)lead + (T.el_off[seg + 1] - e0);
    const bool fin = T.finishes(sg);
    chain_sponge_ex(P, RK, lds, total, T.init_cap, [&](size_t q) -> fr_t { return q < lead ? fr_zero<PF>() : T.elem(e0 + (q - lead)); },
                    fin ? T.out + seg : (fr_t*)nullptr, fresh ? (const fr_t*)nullptr : st, fin, st);
    if (threadIdx.x == 0) T.pos[b] = fin ? 0u : (total ? (uint32_t)(total - 16 * ((total - 1) / 16)) : 0u);
}

}  // namespace
#endif
