// stark_mlwe_amd/csrc/poseidon_dev.hpp — Poseidon x^5 permutation and sponges on CDNA4 (gfx950).
//
// Device replacement for the reference's CPU inner loops
//   permute / permute_dynamic            crates/poseidon/src/lib.rs:31-68, 219-258
//   hash_with_ds_dynamic (eager sponge)  crates/poseidon/src/lib.rs:276-312
//   hash_with_ds (legacy sponge)         crates/poseidon/src/lib.rs:85-100
//   Transcript duplex (lazy permute)     crates/transcript/src/lib.rs:79-101
//   hash_leaf_pair                       crates/deep_ali/src/fri.rs:38-44
//
// Mapping: one lane owns one sponge (all 64 lanes busy in the partial rounds; round constants are
// wave-uniform, so they arrive through the scalar cache).  The t-element state lives in LDS in an
// [element][half][lane] layout (16-byte slots, lane-contiguous => conflict-free ds_read/write_b128),
// which keeps the round loops rolled (small I-cache footprint) and the VGPR count low.
// Dense MDS products are applied IN PLACE through the LU factors prepared on the host, the RP
// partial rounds through the sparse factorisation (host_util.hpp) — the same field values as the
// reference's dense rounds, hence identical bits.
//
// The sponge bodies are written against a state accessor `S` (ld/st) so that the very same code
// can be instantiated with a plain array on the host by the host-check library (CPU unit tests).
#pragma once
#include "fr.hpp"
#include "fr29.hpp"
#include "dev_common.hpp"
#include "poseidon_params.hpp"
#include "poseidon_streams.hpp"

namespace stark {

// Plain-array state (host-check library).
struct ArrayState {
    fr_t* a;
    FR_HD fr_t ld(int j) const { return a[j]; }
    FR_HD void st(int j, const fr_t& x) const { a[j] = x; }
};

// Dot product  sum_i c_i * x_i  with ONE Montgomery reduction: constants as nine 29-bit limbs in the 2^261
// domain, carry-free column sums (fr29.hpp).  A carry pass every 7 terms (Pallas) keeps the 64-bit columns in range;
// rows longer than 60 terms (t = 65, 129) are reduced in chunks.
struct DotAcc {
    fr_wide29 w; fr_t sum; int since, total; bool have_sum;
    FR_HD void init() { fr_wide29_zero(w); since = 0; total = 0; have_sum = false; }
    FR_HD void mac(const uint32_t* __restrict__ c29, const fr_t& x) {
        if (since == fr29_max_terms<PF>()) { fr_wide29_norm(w); since = 0; }
        fr_wide29_mac(w, c29, fr29_unpack(x)); ++since;
        if (++total == 60) { fr_t r = fr_wide29_reduce<PF>(w); sum = have_sum ? fr_add<PF>(sum, r) : r; have_sum = true; fr_wide29_zero(w); since = 0; total = 0; }
    }
    FR_HD fr_t finish() {
        if (!have_sum) return fr_wide29_reduce<PF>(w);
        return total ? fr_add<PF>(sum, fr_wide29_reduce<PF>(w)) : sum;
    }
};
FR_HD const uint32_t* c29(const uint32_t* base, size_t idx) { return base + 9 * idx; }
// One product by an entry of a multiplier table (nine limbs, fr29_const_from): canonical c * x.  The unscale of the 8-round blocks' chain value
// (poseidon_pair.hpp pair_permute), the same statement in the host checks.
FR_HD fr_t fr_mul_c29(const uint32_t* __restrict__ c, const fr_t& x) { fr_wide29 w; fr_wide29_zero(w); fr_wide29_mac(w, c, fr29_unpack(x)); return fr_wide29_reduce<PF>(w); }

// y = L*(U*x) in place.  U: row i needs x[j>=i] (top-down); unit-lower L: row i needs y[j<i] (bottom-up).
// Every row is a dot product with wave-uniform constants: the 64-MAC partial products of all its terms
// are summed in one wide accumulator and reduced once (fr.hpp "wide").
template <class S> FR_HD void apply_lu(const S& s, const uint32_t* lu, int t) {
    for (int i = 0; i < t; ++i) {
        DotAcc d; d.init();
        for (int j = i; j < t; ++j) d.mac(c29(lu, i * t + j), s.ld(j));
        s.st(i, d.finish());
    }
    for (int i = t - 1; i >= 1; --i) {
        DotAcc d; d.init();
        for (int j = 0; j < i; ++j) d.mac(c29(lu, i * t + j), s.ld(j));
        s.st(i, fr_add<PF>(s.ld(i), d.finish()));
    }
}
// One Poseidon permutation of the state behind `s`.  Returns lane 0 of the result.  With `only0`
// the final MDS computes row 0 only (the sponge squeezes state[0]); the rest of the state is then dead.
template <class S> FR_HD fr_t permute_core(const S& s, const PoseidonDev& P, bool only0) {
    const int t = P.t, half = P.rf / 2;
    for (int r = 0; r < half; ++r) {
        for (int j = 0; j < t; ++j) s.st(j, fr_pow5_r29<PF>(fr_add<PF>(s.ld(j), P.rc_full[r * t + j])));   // x^5 / 2^20: the tables carry the 2^20
        apply_lu(s, (r == half - 1) ? P.lu_pre29 : P.lu29, t);
    }
    // Partial rounds in blocks of 4 (rp is a multiple of 4 for every supported width).  Within a block the
    // lanes 1..t-1 stay at their block-start value s_j; round q of the block computes
    //     x_q = (s0 + c_q)^5,   s0 <- a_q x_q + sum_{p<q} gamma_{q,p} x_p + sum_j u_{q,j} s_j      (ONE reduction)
    // and the lanes are brought up to date once per block:  s_j += sum_{p<4} w_{p,j} x_p           (one reduction per lane)
    // — the same values as updating s_j += w_j x after every round, with 20 reductions per block instead of 68.
    fr_t s0 = s.ld(0);
    const int w = 2 * t - 1;
    for (int b = 0; b < P.rp / 4; ++b) {
        const uint32_t* sp = c29(P.sparse29, (size_t)(4 * b) * w);
        const uint32_t* g = c29(P.gamma29, (size_t)b * 6);
        fr_t x0, x1, x2, x3;
#define STARK_PARTIAL_ROUND(q, XQ)                                                              \
        {                                                                                       \
            XQ = fr_pow5_r29<PF>(fr_add<PF>(s0, P.rc_partial[4 * b + q]));                       \
            DotAcc acc; acc.init();                                                             \
            acc.mac(c29(sp, q * w), XQ);                                                        \
            if (q > 0) acc.mac(c29(g, q * (q - 1) / 2 + 0), x0);                                 \
            if (q > 1) acc.mac(c29(g, q * (q - 1) / 2 + 1), x1);                                 \
            if (q > 2) acc.mac(c29(g, q * (q - 1) / 2 + 2), x2);                                 \
            for (int j = 1; j < t; ++j) acc.mac(c29(sp, q * w + j), s.ld(j));                    \
            s0 = acc.finish();                                                                  \
        }
        STARK_PARTIAL_ROUND(0, x0) STARK_PARTIAL_ROUND(1, x1) STARK_PARTIAL_ROUND(2, x2) STARK_PARTIAL_ROUND(3, x3)
#undef STARK_PARTIAL_ROUND
        for (int j = 1; j < t; ++j) {
            DotAcc u; u.init();
            u.mac(c29(sp, 0 * w + t - 1 + j), x0); u.mac(c29(sp, 1 * w + t - 1 + j), x1);
            u.mac(c29(sp, 2 * w + t - 1 + j), x2); u.mac(c29(sp, 3 * w + t - 1 + j), x3);
            s.st(j, fr_add<PF>(s.ld(j), u.finish()));
        }
    }
    s.st(0, s0);
    for (int r = half; r < P.rf; ++r) {
        for (int j = 0; j < t; ++j) s.st(j, fr_pow5_r29<PF>(fr_add<PF>(s.ld(j), P.rc_full[r * t + j])));   // x^5 / 2^20: the tables carry the 2^20
        if (only0 && r == P.rf - 1) {
            DotAcc acc; acc.init();
            for (int j = 0; j < t; ++j) acc.mac(c29(P.row0_29, j), s.ld(j));
            return acc.finish();
        }
        apply_lu(s, P.lu29, t);
    }
    return s.ld(0);
}

// ---- sponge bodies (one call = the work of one lane; the streams of poseidon_streams.hpp) ----------------------
// hash_leaf_pair: one permutation of the template with elements 4, 5 = (f_i, s_i).
template <class S> FR_HD fr_t leaf_pair_body(const S& s, const PoseidonDev& P, const LeafStream& L, size_t i) {
    for (int j = 0; j < 16; ++j) s.st(j, j < 9 ? L.elem(i, j) : fr_zero<PF>());
    s.st(16, L.cap());
    return permute_core(s, P, true);
}
// hash_with_ds_dynamic: eager sponge (permute after every full rate block and after the final one).
template <class S, class DS> FR_HD fr_t hash_ds_body(const S& s, const PoseidonDev& P, const DS& D, size_t k) {   // DS: DsStream or DsGatherStream
    const int t = P.t, rate = t - 1;
    for (int j = 0; j < t; ++j) s.st(j, fr_zero<PF>());
    const size_t total = D.total(k);
    size_t nperm = (total + rate - 1) / rate, done = 0;
    int cur = 0; fr_t res = fr_zero<PF>();
    for (size_t q = 0; q < total; ++q) {
        s.st(cur, fr_add<PF>(s.ld(cur), D.elem(k, q)));
        if (++cur == rate) { cur = 0; ++done; res = permute_core(s, P, done == nperm); }
    }
    if (cur != 0) res = permute_core(s, P, true);
    return res;
}
// Transcript-style duplex (t=17, rate 16, lazy permute: only before absorbing more, once at the end), state[16] = cap.
// RAGGED: the stream's Ragged layout (sponge i is items[i], digest to *slot = items[i].out; otherwise *slot = i).
template <bool RAGGED, class S> FR_HD fr_t tr_hash_body(const S& s, const PoseidonDev& P, const TrStream& T, size_t i, size_t* slot) {
    for (int j = 0; j < 16; ++j) s.st(j, fr_zero<PF>());
    s.st(16, T.cap);
    const TrStream::Sponge sp = T.sponge_as<RAGGED>(i, slot);
    int pos = 0;
    for (size_t q = 0; q < sp.total(); ++q) {
        const fr_t x = sp.elem(q);
        if (pos == 16) { permute_core(s, P, false); pos = 0; }
        s.st(pos, fr_add<PF>(s.ld(pos), x)); ++pos;
    }
    return permute_core(s, P, true);
}
template <class S> FR_HD fr_t tr_hash_body(const S& s, const PoseidonDev& P, const TrStream& T, size_t i) { size_t slot; return tr_hash_body<false>(s, P, T, i, &slot); }
// Active instance a of a TrBatchStream: the stored (or reset) state, the lazy permute before absorbing into a full rate, one permutation
// and squeeze per finished segment; state and cursor written back.
template <class S> FR_HD void tr_batch_body(const S& s, const PoseidonDev& P, const TrBatchStream& T, size_t a) {
    const size_t b = T.instance(a); const bool fresh = T.resets(a);
    for (int j = 0; j < 17; ++j) s.st(j, fresh ? (j == 16 ? T.init_cap : fr_zero<PF>()) : T.state[17 * b + j]);
    uint32_t pos = fresh ? 0u : T.pos[b];
    for (size_t sg = 0; sg < T.nseg; ++sg) {
        const size_t seg = a * T.nseg + sg;
        for (uint32_t j = T.el_off[seg]; j < T.el_off[seg + 1]; ++j) {
            if (pos == 16) { permute_core(s, P, false); pos = 0; }
            s.st((int)pos, fr_add<PF>(s.ld((int)pos), T.elem(j))); ++pos;
        }
        if (T.finishes(sg)) { T.out[seg] = permute_core(s, P, false); pos = 0; }
    }
    for (int j = 0; j < 17; ++j) T.state[17 * b + j] = s.ld(j);
    T.pos[b] = pos;
}
// Generic eager sponge over explicit per-hash streams.
//   mode 0: hash_with_ds_dynamic — stream = a_k || b_k || 1, zero-padded (eager permute on a full rate).
//   mode 1: hash_with_ds (legacy) — state[t-1] = tag, b_k absorbed in rate-sized chunks, one permutation
//           per (possibly short) chunk, no padding.
template <class S> FR_HD fr_t hash_stream_body(const S& s, const PoseidonDev& P, int mode, const fr_t* a, size_t na, const fr_t* b, size_t nb, const fr_t& tag, size_t k) {
    const int t = P.t, rate = t - 1;
    for (int j = 0; j < t; ++j) s.st(j, fr_zero<PF>());
    int cur = 0;
    if (mode == 0) {
        const size_t total = na + nb + 1;
        for (size_t q = 0; q < total; ++q) {
            fr_t x = q < na ? ldg(a + k * na + q) : (q < na + nb ? ldg(b + k * nb + (q - na)) : fr_one<PF>());
            s.st(cur, fr_add<PF>(s.ld(cur), x));
            if (++cur == rate) { cur = 0; permute_core(s, P, false); }
        }
        if (cur != 0) permute_core(s, P, false);
    } else {
        s.st(t - 1, tag);
        for (size_t q = 0; q < nb; ++q) {
            s.st(cur, fr_add<PF>(s.ld(cur), ldg(b + k * nb + q)));
            if (++cur == rate || q + 1 == nb) { cur = 0; permute_core(s, P, false); }
        }
    }
    return s.ld(0);
}

#if defined(__HIPCC__)
// ---- LDS-resident per-lane state ---------------------------------------------------------------------
struct LdsState {
    uint4* base; int nl; int lane;
    __device__ __forceinline__ fr_t ld(int j) const {
        uint4 lo = base[(2 * j) * nl + lane], hi = base[(2 * j + 1) * nl + lane];
        fr_t x; x.v[0] = lo.x; x.v[1] = lo.y; x.v[2] = lo.z; x.v[3] = lo.w; x.v[4] = hi.x; x.v[5] = hi.y; x.v[6] = hi.z; x.v[7] = hi.w; return x;
    }
    __device__ __forceinline__ void st(int j, const fr_t& x) const {
        base[(2 * j) * nl + lane] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
        base[(2 * j + 1) * nl + lane] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
    }
};
// ---- kernels ---------------------------------------------------------------------------------------
// K3: h[i] = hash_leaf_pair(f[i], s_i).
__global__ void __launch_bounds__(64) k_leaf_pair(PoseidonDev P, LeafStream L, fr_t* __restrict__ h) {
    extern __shared__ uint4 lds[];
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n) return;
    LdsState s{lds, (int)blockDim.x, (int)threadIdx.x};
    stg(h + i, leaf_pair_body(s, P, L, i));
}
// K4: one Merkle level / the pair-leaf level.
template <class DS>
__global__ void __launch_bounds__(64) k_hash_ds(PoseidonDev P, DS D, fr_t* __restrict__ out) {
    extern __shared__ uint4 lds[];
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.n_out) return;
    LdsState s{lds, (int)blockDim.x, (int)threadIdx.x};
    stg(out + k, hash_ds_body(s, P, D, k));
}
// permute / permute_dynamic over a batch of AoS states (poseidon/src/lib.rs:31,219).
__global__ void __launch_bounds__(64) k_permute_batch(PoseidonDev P, fr_t* __restrict__ states, size_t n) {
    extern __shared__ uint4 lds[];
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    LdsState s{lds, (int)blockDim.x, (int)threadIdx.x};
    for (int j = 0; j < P.t; ++j) s.st(j, ldg(states + i * P.t + j));
    permute_core(s, P, false);
    for (int j = 0; j < P.t; ++j) stg(states + i * P.t + j, s.ld(j));
}
// Batch of independent transcript hashes (index seeds, z seeds); with n == 1 a whole column
// (the serial sponge of build_f0, fri.rs:551-554).
__global__ void __launch_bounds__(64) k_tr_hash(PoseidonDev P, TrStream T, fr_t* __restrict__ out) {
    extern __shared__ uint4 lds[];
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.n) return;
    LdsState s{lds, (int)blockDim.x, (int)threadIdx.x};
    stg(out + i, tr_hash_body(s, P, T, i));
}
// The Ragged layout, one lane per item.  The lanes of a wave have different lengths and simply leave the absorb loop at different times:
// permute_core over LdsState is lane-local (no shuffle, DPP move or barrier; each lane reads and writes its own LDS column), so a lane that
// is done waits masked off while its neighbours go on.  The driver's longest-first order keeps the lengths within a wave close.
__global__ void __launch_bounds__(64) k_tr_hash_ragged(PoseidonDev P, TrStream T, fr_t* __restrict__ out) {
    extern __shared__ uint4 lds[];
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.n) return;
    LdsState s{lds, (int)blockDim.x, (int)threadIdx.x};
    size_t slot; const fr_t d = tr_hash_body<true>(s, P, T, i, &slot);
    stg(out + slot, d);
}
__global__ void __launch_bounds__(64) k_hash_stream(PoseidonDev P, int mode, const fr_t* __restrict__ a, size_t na, const fr_t* __restrict__ b, size_t nb,
                                                    fr_t tag, size_t n, fr_t* __restrict__ out) {
    extern __shared__ uint4 lds[];
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    LdsState s{lds, (int)blockDim.x, (int)threadIdx.x};
    stg(out + k, hash_stream_body(s, P, mode, a, na, b, nb, tag, k));
}
#endif  // __HIPCC__

}  // namespace stark
