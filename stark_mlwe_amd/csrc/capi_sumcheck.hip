// stark_mlwe_amd/csrc/capi_sumcheck.hip — the sum-check entry points of the C-ABI (its Poseidon work goes through poseidon_launch.hpp; its own kernels are the k_sc_* below)
// "next" row N4: the sum-check consumer of the Merkle / Poseidon / transcript kernels
// (crates/channel/src/lib.rs).  prove_plain / verify_plain (:1045-1128) and the Merkle-folded prove_mf / verify_mf (:1130-1240):
//   * MerkleCommitment::commit (commitment/src/lib.rs:85-90: arity 16, parameters "POSEIDON-T17-X5-SEED") of the witness and of every
//     shrinking folded layer = the level-batched Merkle kernels of the FRI path (merkle_build_on);
//   * round coefficients c0 = sum a_j, c1 = sum (b_j - a_j) (:406-416) and the fold (1-r) a + r b (:456-462) = streaming kernels;
//   * the Fiat-Shamir channel (:7-117) = DEVICE-RESIDENT transcripts:
//     the ABI's transcript object queues absorbs on the host and runs them as ONE launch when a challenge is drawn (DevTranscript); the
//     provers and verifiers lay out what every instance absorbs as pool indices and advance all transcripts of a batch per launch
//     (TrBatchStream), so neither has a host round trip in its rounds.
// Every prove — one witness or many — runs the batched round loops of sumcheck_batch.hpp over the device executor below (ScDevExec); every
// verify — one proof or many — is a plan of sumcheck_verify_batch.hpp run by run_sc_verify_batch, and stark_commitment_verify a Merkle plan
// of one item through capi_verify.hip's runner (verify_dev.hpp).
// Proof bytes = bincode 1.x layout of the reference's serde structs ProofPlain / ProofMF (:925-979), what its bench measures.
#include <memory>
#include "verify_dev.hpp"
#include "sumcheck_impl.hpp"
#include "mle_dev.hpp"

using namespace stark;

namespace {

// ---- kernels ------------------------------------------------------------------------------------------------------------
// block partials of (c0, c1) over pairs (a, b) = (layer[2j], layer[2j+1]); out[2*block], out[2*block+1] (grid-stride over gridDim.x blocks)
__device__ __forceinline__ void sc_coeffs_block(const fr_t* __restrict__ layer, uint64_t npairs, fr_t* __restrict__ out) {
    __shared__ uint4 red[2 * 2 * 4];
    fr_t c0 = fr_zero<PF>(), c1 = fr_zero<PF>();
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < npairs; j += (uint64_t)gridDim.x * blockDim.x) {
        const fr_t a = ldg(layer + 2 * j), b = ldg(layer + 2 * j + 1);
        c0 = fr_add<PF>(c0, a); c1 = fr_add<PF>(c1, fr_sub<PF>(b, a));
    }
    for (int sft = 1; sft < 64; sft <<= 1) { c0 = fr_add<PF>(c0, shfl_xor_fr(c0, sft)); c1 = fr_add<PF>(c1, shfl_xor_fr(c1, sft)); }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { red[4 * wave] = make_uint4(c0.v[0], c0.v[1], c0.v[2], c0.v[3]); red[4 * wave + 1] = make_uint4(c0.v[4], c0.v[5], c0.v[6], c0.v[7]);
                     red[4 * wave + 2] = make_uint4(c1.v[0], c1.v[1], c1.v[2], c1.v[3]); red[4 * wave + 3] = make_uint4(c1.v[4], c1.v[5], c1.v[6], c1.v[7]); }
    __syncthreads();
    if (threadIdx.x == 0) {
        fr_t t0 = fr_zero<PF>(), t1 = fr_zero<PF>();
        for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) {
            fr_t x, y; const uint4 a = red[4 * wv], b = red[4 * wv + 1], c = red[4 * wv + 2], d = red[4 * wv + 3];
            x.v[0] = a.x; x.v[1] = a.y; x.v[2] = a.z; x.v[3] = a.w; x.v[4] = b.x; x.v[5] = b.y; x.v[6] = b.z; x.v[7] = b.w;
            y.v[0] = c.x; y.v[1] = c.y; y.v[2] = c.z; y.v[3] = c.w; y.v[4] = d.x; y.v[5] = d.y; y.v[6] = d.z; y.v[7] = d.w;
            t0 = fr_add<PF>(t0, x); t1 = fr_add<PF>(t1, y);
        }
        stg(out + 2 * blockIdx.x, t0); stg(out + 2 * blockIdx.x + 1, t1);
    }
}
// next[j] = (1 - r) * layer[2j] + r * layer[2j+1]  =  a + r * (b - a)
__global__ void __launch_bounds__(256) k_sc_fold(const fr_t* __restrict__ layer, uint64_t npairs, fr_t r, fr_t* __restrict__ next) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npairs) return;
    const fr_t a = ldg(layer + 2 * j), b = ldg(layer + 2 * j + 1);
    stg(next + j, fr_add<PF>(a, fr_mul<PF>(r, fr_sub<PF>(b, a))));
}
// ---- the batched round kernels (sumcheck_batch.hpp): instance b = b0 + blockIdx.y reads layer ptrs[b] or layers + b * len ----------------
// block partials of (c0, c1) of every layer: part[2 (b gridDim.x + block)], +1
__global__ void __launch_bounds__(256) k_sc_coeffs_batch(const fr_t* const* __restrict__ ptrs, const fr_t* __restrict__ layers, uint64_t len, uint64_t b0, fr_t* __restrict__ part) {
    const uint64_t b = b0 + blockIdx.y;
    sc_coeffs_block(ptrs ? ptrs[b] : layers + b * len, len / 2, part + 2 * (uint64_t)gridDim.x * b);
}
// one block per instance: c01[2b] = sum of its partial c0, c01[2b+1] = of c1; claim != nullptr: claim[b] = 2 c0 + c1 (send_claim, :434-446) for the
// instances b >= claim_from (the ones whose first round this is; an earlier instance's claim is never written again)
__global__ void __launch_bounds__(64) k_sc_coeffs_final_batch(const fr_t* __restrict__ part, uint64_t nblocks, fr_t* __restrict__ c01, fr_t* __restrict__ claim, uint64_t claim_from) {
    const uint64_t b = blockIdx.x; const fr_t* p = part + 2 * nblocks * b;
    fr_t c0 = fr_zero<PF>(), c1 = fr_zero<PF>();
    for (uint64_t i = threadIdx.x; i < nblocks; i += 64) { c0 = fr_add<PF>(c0, ldg(p + 2 * i)); c1 = fr_add<PF>(c1, ldg(p + 2 * i + 1)); }
    for (int sft = 1; sft < 64; sft <<= 1) { c0 = fr_add<PF>(c0, shfl_xor_fr(c0, sft)); c1 = fr_add<PF>(c1, shfl_xor_fr(c1, sft)); }
    if (threadIdx.x == 0) { stg(c01 + 2 * b, c0); stg(c01 + 2 * b + 1, c1); if (claim && b >= claim_from) stg(claim + b, fr_add<PF>(fr_add<PF>(c0, c0), c1)); }
}
// next[b len/2 + j] = a + r_b (b - a) with r_b = r[b], the instance's challenge as the transcript kernel left it in device memory
__global__ void __launch_bounds__(256) k_sc_fold_batch(const fr_t* const* __restrict__ ptrs, const fr_t* __restrict__ layers, uint64_t len, uint64_t b0, const fr_t* __restrict__ r,
                                                       fr_t* __restrict__ next) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = b0 + blockIdx.y, np = len / 2;
    if (j >= np) return;
    const fr_t* layer = ptrs ? ptrs[b] : layers + b * len;
    const fr_t a = ldg(layer + 2 * j), c = ldg(layer + 2 * j + 1), rb = ldg(r + b);
    stg(next + b * np + j, fr_add<PF>(a, fr_mul<PF>(rb, fr_sub<PF>(c, a))));
}
// out[j] = *addr[j]: the roots of one-leaf trees and the openings of prove_mf (addresses built on the host from the known shapes)
__global__ void __launch_bounds__(256) k_sc_gather(const fr_t* const* __restrict__ addr, uint64_t n, fr_t* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) stg(out + j, ldg(addr[j]));
}
// ---- the batched verifiers (sumcheck_verify_batch.hpp) ---------------------------------------------------------------------------
// Decode entry j of a plan -> pool[j]: one lane per field element, its 32 bytes read at any byte offset of the uploaded proofs as the nine
// covering dwords; a value >= r clears the owning proof's flag.
__global__ void __launch_bounds__(256) k_sc_decode_fr(const uint32_t* __restrict__ words, const uint32_t* __restrict__ dec_off, const uint32_t* __restrict__ dec_proof, uint32_t n,
                                                      fr_t* __restrict__ pool, int32_t* __restrict__ flag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t owner = dec_proof[j]; fr_t x;
    if (!sc_decode_fr(words, dec_off[j], owner, x)) flag[owner & ~kScClaim] = 0;
    stg(pool + j, x);
}
// verify_plain's relations, one lane per (proof, round); verify_mf's, one lane per relation.  A failed one clears the proof's flag.
__global__ void __launch_bounds__(256) k_sc_verify_plain_check(const fr_t* __restrict__ pool, const uint32_t* __restrict__ rec, uint32_t n, int32_t* __restrict__ flag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n && !sc_check_plain(pool, rec + 8 * (size_t)j)) flag[rec[8 * (size_t)j]] = 0;
}
__global__ void __launch_bounds__(256) k_sc_verify_mf_check(const fr_t* __restrict__ pool, const uint32_t* __restrict__ rec, uint32_t n, int32_t* __restrict__ flag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n && !sc_check_mf(pool, rec + 8 * (size_t)j)) flag[rec[8 * (size_t)j + 1]] = 0;
}

// ---- device-resident transcript -----------------------------------------------------------------------------------------
struct DevTranscript {
    stark_ctx* ctx; DevBuf state, posb, out; std::vector<fr_t> pending; stark_params* tp = nullptr;
    explicit DevTranscript(stark_ctx* c) : ctx(c) {}
    int32_t init(const uint8_t* label, size_t n) {                                        // Transcript::new (:55-65)
        STARK_TRY(ctx_transcript_params(ctx, &tp));
        STARK_HIP(ctx, state.alloc(ctx, 17 * sizeof(fr_t))); STARK_HIP(ctx, posb.alloc(ctx, 4)); STARK_HIP(ctx, out.alloc(ctx, sizeof(fr_t)));
        fr_t st[17]; for (auto& x : st) x = host::h_zero(); st[16] = host::h_tag("FSv1-TRANSCRIPT-INIT");
        STARK_TRY(ctx_upload_staged(ctx, state.p, st, sizeof(st)));
        STARK_HIP(ctx, hipMemsetAsync(posb.p, 0, 4, ctx->stream));
        absorb_bytes(label, n); return STARK_OK;
    }
    void absorb_field(const fr_t& x) { pending.push_back(x); }
    void absorb_bytes(const uint8_t* b, size_t n) {                                        // :67-73: marker, then 31-byte words
        pending.push_back(host::h_tag("FSv1-ABSORB-BYTES"));
        for (size_t o = 0; o < n; o += 31) pending.push_back(host::h_from_le_bytes_mod_order(b + o, std::min<size_t>(31, n - o)));
    }
    int32_t run(bool finish, fr_t* result) {
        DevBuf f; const size_t n = pending.size();
        if (n) { STARK_HIP(ctx, f.alloc(ctx, n * sizeof(fr_t))); STARK_TRY(ctx_upload_staged(ctx, f.p, pending.data(), n * sizeof(fr_t))); }
        STARK_TRY(tr_stream_on(ctx, tp, state.fr(), (uint32_t*)posb.p, f.fr(), n, finish, out.fr()));
        if (finish && result) STARK_HIP(ctx, hipMemcpyAsync(result, out.p, sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
        STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));                                 // the challenge is needed on the host
        pending.clear(); return STARK_OK;
    }
    int32_t challenge(const uint8_t* label, size_t n, fr_t* r) {                           // :92-101
        pending.push_back(host::h_tag("FSv1-CHALLENGE")); absorb_bytes(label, n);
        return run(true, r);
    }
};

static int32_t fold(stark_ctx* ctx, const fr_t* layer, size_t len, const fr_t& r, fr_t* next) {
    const uint64_t np = len / 2;
    hipLaunchKernelGGL(k_sc_fold, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, layer, np, r, next);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
// The device executor of the batched drivers (sumcheck_batch.hpp): every operation is one launch (or a few, for more than 65535 layers) on
// the context's stream; its memory is the arena's, the host copies of its uploads held until the round's download.
struct ScDevExec : DevArena {
    stark_params* cp; stark_params* tp;
    ScDevExec(stark_ctx* c, stark_params* commit, stark_params* tr) : DevArena(c, true), cp(commit), tp(tr) {}
    template <class DS> int32_t hash_level(const DS& D, fr_t* out) { return hash_ds_on(ctx, ctx->stream, cp, D, out); }
    int32_t coeffs(const fr_t* const* ptrs, const fr_t* layers, size_t len, size_t B, fr_t* c01, fr_t* claim, size_t claim_from) {
        const uint64_t np = len / 2; const unsigned grid = (unsigned)std::min<uint64_t>((np + 255) / 256, 1024);
        DevBuf part; STARK_HIP(ctx, part.alloc(ctx, (size_t)grid * 2 * B * sizeof(fr_t)));
        for (size_t b0 = 0; b0 < B; b0 += 65535)
            hipLaunchKernelGGL(k_sc_coeffs_batch, dim3(grid, (unsigned)std::min<size_t>(65535, B - b0)), dim3(256), 0, ctx->stream, ptrs, layers, (uint64_t)len, (uint64_t)b0, part.fr());
        hipLaunchKernelGGL(k_sc_coeffs_final_batch, dim3((unsigned)B), dim3(64), 0, ctx->stream, (const fr_t*)part.fr(), (uint64_t)grid, c01, claim, (uint64_t)claim_from);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    int32_t fold(const fr_t* const* ptrs, const fr_t* layers, size_t len, size_t B, const fr_t* r, fr_t* next) {
        const uint64_t np = len / 2;
        for (size_t b0 = 0; b0 < B; b0 += 65535)
            hipLaunchKernelGGL(k_sc_fold_batch, dim3((unsigned)((np + 255) / 256), (unsigned)std::min<size_t>(65535, B - b0)), dim3(256), 0, ctx->stream, ptrs, layers, (uint64_t)len, (uint64_t)b0, r, next);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    int32_t transcript(const TrBatchStream& T) { return tr_batch_on(ctx, tp, T, 1); }     // the form one instance would take (poseidon_launch.hpp)
    int32_t gather(const fr_t* const* addr, size_t n, fr_t* out) {
        hipLaunchKernelGGL(k_sc_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, addr, (uint64_t)n, out);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
};
// prove_plain (mf = 0, :1045-1076) / prove_mf (mf = 1, :1130-1172) of `B` device-resident witnesses, witness b of 2^k[b] elements: out[b] = the
// proof of witness b alone.  The same-size batch entry points are this with every k[b] equal, the single ones with B = 1.
static int32_t prove_sumcheck_mixed_impl(stark_ctx* ctx, int mf, size_t B, const uint64_t* const* witnesses, const size_t* k, const uint64_t* tree_labels, size_t qpr, stark_proof** out) {
    for (size_t b = 0; b < B; ++b) out[b] = nullptr;
    for (size_t b = 0; b < B; ++b) if (k[b] > 40) return ctx->fail(STARK_ERR_INVALID_ARG, "k too large");
    if (!B) return STARK_OK;
    stark_params *cp = nullptr, *tp = nullptr; STARK_TRY(ctx_commit_params(ctx, &cp)); STARK_TRY(ctx_transcript_params(ctx, &tp));
    std::vector<const fr_t*> w(B); for (size_t b = 0; b < B; ++b) w[b] = as_fr(witnesses[b]);
    std::vector<std::vector<uint8_t>> proofs;
    {
        ScDevExec X(ctx, cp, tp);
        ScBatch<ScDevExec> S(X, B, w.data(), k, tree_labels);
        const int32_t rc = mf ? S.prove_mf(qpr, proofs) : S.prove_plain(proofs);
        if (rc) return rc;
    }
    std::vector<std::unique_ptr<stark_proof>> pf(B);
    for (size_t b = 0; b < B; ++b) { pf[b].reset(new stark_proof()); pf[b]->bytes.swap(proofs[b]); pf[b]->size_estimate = pf[b]->bytes.size(); }
    hand_out(pf, out); return STARK_OK;
}

// Runs one plan of the batched verifiers: one upload (the proofs' bytes and the plan's index arrays), the decode, the transcript streams,
// the DS groups in depth order, the checks, one download of the flags and one synchronisation.
static int32_t run_sc_verify_batch(stark_ctx* ctx, const ScVerifyPlan& V, int32_t* accepted) {
    if (!V.batch) return STARK_OK;
    stark_params *cp = nullptr, *tp = nullptr; STARK_TRY(ctx_commit_params(ctx, &cp)); STARK_TRY(ctx_transcript_params(ctx, &tp));
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const VerifyBatchPlan& D = V.ds;
    const size_t o_flag = 0, o_blob = al(V.batch * 4), o_doff = al(o_blob + V.blob.size() * 4), o_dpr = al(o_doff + V.n_dec * 4), o_con = al(o_dpr + V.n_dec * 4),
                 o_toff = al(o_con + V.consts.size() * sizeof(fr_t)), o_tidx = al(o_toff + V.tr_off.size() * 4), o_hdr = al(o_tidx + V.tr_idx.size() * 4),
                 o_off = al(o_hdr + D.hdr.size() * 8), o_idx = al(o_off + D.off.size() * 4), o_rec = al(o_idx + D.idx.size() * 4), n_up = al(o_rec + V.rec.size() * 4),
                 o_pool = n_up, o_state = al(o_pool + V.pool_slots * sizeof(fr_t)), o_pos = al(o_state + 17 * V.n_inst * sizeof(fr_t)), total = al(o_pos + 4 * V.n_inst);
    std::vector<uint8_t> h(n_up);                                       // everything the device reads, in one upload
    auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) memcpy(h.data() + o, src, bytes); };
    put(o_flag, V.flag.data(), V.batch * 4); put(o_blob, V.blob.data(), V.blob.size() * 4); put(o_doff, V.dec_off.data(), V.n_dec * 4); put(o_dpr, V.dec_proof.data(), V.n_dec * 4);
    put(o_con, V.consts.data(), V.consts.size() * sizeof(fr_t)); put(o_toff, V.tr_off.data(), V.tr_off.size() * 4); put(o_tidx, V.tr_idx.data(), V.tr_idx.size() * 4);
    put(o_hdr, D.hdr.data(), D.hdr.size() * 8); put(o_off, D.off.data(), D.off.size() * 4); put(o_idx, D.idx.data(), D.idx.size() * 4); put(o_rec, V.rec.data(), V.rec.size() * 4);
    DevBuf d; STARK_HIP(ctx, d.alloc(ctx, total));
    uint8_t* base = (uint8_t*)d.p; fr_t* pool = (fr_t*)(base + o_pool); int32_t* flag = (int32_t*)(base + o_flag);
    hipStream_t st = ctx->stream;
    CallerUploads up(ctx);                                                           // `h` is not copied again: every return below is fenced
    if (up.copy(base, h.data(), h.size()) != hipSuccess) return ctx->fail(STARK_ERR_HIP, "upload");
    if (V.n_dec) hipLaunchKernelGGL(k_sc_decode_fr, dim3((unsigned)((V.n_dec + 255) / 256)), dim3(256), 0, st, (const uint32_t*)(base + o_blob), (const uint32_t*)(base + o_doff),
                                    (const uint32_t*)(base + o_dpr), (uint32_t)V.n_dec, pool, flag);
    for (const ScVerifyPlan::Stream& S : V.tr) {
        TrBatchStream T; T.state = (fr_t*)(base + o_state); T.pos = (uint32_t*)(base + o_pos); T.inst = nullptr; T.inst0 = S.inst0; T.n_active = S.n; T.nseg = S.nseg;
        T.el_off = (const uint32_t*)(base + o_toff) + S.seg0; T.idx = (const uint32_t*)(base + o_tidx); T.pool0 = pool; T.pool1 = (const fr_t*)(base + o_con);
        T.out = pool + V.n_dec + S.seg0; T.init_cap = host::h_tag("FSv1-TRANSCRIPT-INIT"); T.reset_from = 0; T.finish_last = 1;
        for (size_t a0 = 0; a0 < S.n; a0 += 0x7fffffffu / 2) {                       // (a grid's x dimension)
            TrBatchStream Ta = T; Ta.inst0 = S.inst0 + a0; Ta.n_active = std::min<size_t>(S.n - a0, 0x7fffffffu / 2); Ta.el_off = T.el_off + a0 * S.nseg; Ta.out = T.out + a0 * S.nseg;
            STARK_TRY(tr_batch_on(ctx, tp, Ta, Ta.n_active));                            // the form that many instances take
        }
    }
    STARK_TRY(verify_batch_groups_on(ctx, D, (const uint64_t*)(base + o_hdr), (const uint32_t*)(base + o_off), (const uint32_t*)(base + o_idx), pool, cp));
    if (const size_t n = V.n_rec()) {
        const dim3 grid((unsigned)((n + 255) / 256));
        if (V.mf) hipLaunchKernelGGL(k_sc_verify_mf_check, grid, dim3(256), 0, st, (const fr_t*)pool, (const uint32_t*)(base + o_rec), (uint32_t)n, flag);
        else hipLaunchKernelGGL(k_sc_verify_plain_check, grid, dim3(256), 0, st, (const fr_t*)pool, (const uint32_t*)(base + o_rec), (uint32_t)n, flag);
    }
    if (hipGetLastError() != hipSuccess) return ctx->fail(STARK_ERR_HIP, "sum-check batch verification launch");
    STARK_HIP(ctx, up.download_sync(accepted, flag, V.batch * 4));
    return STARK_OK;
}
// verify_plain (mf = 0) / verify_mf (mf = 1) of a batch (the single entry points: B = 1), cut into plans of at most the context's "sumcheck_verify_batch_max_slots" pool slots
static int32_t verify_sumcheck_batch_impl(stark_ctx* ctx, int mf, size_t batch, const uint8_t* const* proofs, const size_t* lens, const uint64_t* tree_labels, int32_t* accepted) {
    size_t b0 = 0;
    while (b0 < batch) {
        ScVerifyPlan V; bool fits = false;
        const size_t b1 = sc_verify_plan_some(mf, b0, batch, proofs, lens, tree_labels, ctx->opt.sumcheck_verify_batch_max_slots, V, fits);
        int32_t rc = fits ? run_sc_verify_batch(ctx, V, accepted + b0) : ctx->fail(STARK_ERR_INVALID_ARG, "a proof of the batch needs more than 2^30 pool slots");
        if (rc) { memset(accepted, 0, batch * sizeof(int32_t)); return rc; }
        b0 = b1;
    }
    return STARK_OK;
}

// ---- Mle::evaluate of device-resident tables (mle_dev.hpp) ----------------------------------------------------------------------------
template <int C, bool CONTIG>
static void mle_launch(stark_ctx* ctx, size_t B, const fr_t* const* ptrs, const fr_t* layers, uint64_t len, int t, const fr_t* r, size_t k, size_t j0, fr_t* next) {
    const unsigned gx = (unsigned)(((len >> C) + 255) / 256);
    for (size_t b0 = 0; b0 < B; b0 += 65535)                                                // (a grid's y dimension)
        hipLaunchKernelGGL((k_mle_fold_pass<C, CONTIG>), dim3(gx, (unsigned)std::min<size_t>(65535, B - b0)), dim3(256), 0, ctx->stream, ptrs, layers, len, t, (uint64_t)b0, r,
                           (uint64_t)k, (uint64_t)j0, next);
}
static int32_t mle_pass(stark_ctx* ctx, bool contig, size_t B, const fr_t* const* ptrs, const fr_t* layers, uint64_t len, int t, const fr_t* r, size_t k, size_t j0, fr_t* next) {
#define STARK_MLE_CASE(C) case C: if (contig) mle_launch<C, true>(ctx, B, ptrs, layers, len, t, r, k, j0, next); else mle_launch<C, false>(ctx, B, ptrs, layers, len, t, r, k, j0, next); break;
    switch (mle_local_rounds(t)) { STARK_MLE_CASE(0) STARK_MLE_CASE(1) STARK_MLE_CASE(2) STARK_MLE_CASE(3) STARK_MLE_CASE(4) default: return ctx->fail(STARK_ERR_UNSUPPORTED, "mle: tile out of range"); }
#undef STARK_MLE_CASE
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
// out[b] = the multilinear extension of tables[b] (2^k elements, device) at r[b * k .. (b + 1) * k) (host).  One upload (the points and the pointer
// table, out of a copy the context owns), ceil(k / T) passes, no synchronisation; the intermediate layers are pooled blocks of B * 2^(k - T) elements
// and less, released in stream order.
static int32_t mle_evaluate_batch_impl(stark_ctx* ctx, size_t B, const uint64_t* const* tables, size_t k, const uint64_t* r, uint64_t* out) {
    const size_t rbytes = B * k * sizeof(fr_t), bytes = rbytes + B * sizeof(void*);
    std::vector<uint8_t> h(bytes);
    if (rbytes) memcpy(h.data(), r, rbytes);
    memcpy(h.data() + rbytes, tables, B * sizeof(void*));
    DevBuf up; STARK_HIP(ctx, up.alloc(ctx, bytes)); STARK_TRY(ctx_upload_staged(ctx, up.p, h.data(), bytes));
    const fr_t* dr = up.fr(); const fr_t* const* ptrs = (const fr_t* const*)((const uint8_t*)up.p + rbytes);
    if (k == 0) {                                                                           // no round: out[b] = tables[b][0]
        hipLaunchKernelGGL(k_sc_gather, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, ctx->stream, ptrs, (uint64_t)B, as_fr(out));
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    const int T = ctx->opt.mle_log_tile < 0 ? kMleDefaultLogTile : ctx->opt.mle_log_tile;
    const bool contig = (ctx->opt.mle_lane_contiguous < 0 ? kMleDefaultContig : ctx->opt.mle_lane_contiguous) != 0;
    const std::vector<int> rounds = mle_pass_rounds(k, T);
    DevBuf tmp[2];                                                                          // layers after pass 0, 2, .. / 1, 3, ..
    for (size_t i = 0; i + 1 < rounds.size() && i < 2; ++i) {
        size_t left = k; for (size_t q = 0; q <= i; ++q) left -= (size_t)rounds[q];
        STARK_HIP(ctx, tmp[i].alloc(ctx, (B << left) * sizeof(fr_t)));
    }
    size_t j0 = 0; const fr_t* cur = nullptr;
    for (size_t i = 0; i < rounds.size(); ++i) {
        fr_t* nxt = i + 1 == rounds.size() ? as_fr(out) : tmp[i & 1].fr();
        STARK_TRY(mle_pass(ctx, contig, B, i ? nullptr : ptrs, cur, (uint64_t)1 << (k - j0), rounds[i], dr, k, j0, nxt));
        j0 += (size_t)rounds[i]; cur = nxt;
    }
    return STARK_OK;
}
// the argument checks of stark_mle_evaluate_batch_dev, all before anything is enqueued
static int32_t mle_check_args(stark_ctx* ctx, size_t B, const uint64_t* const* tables, size_t k, const uint64_t* r, const uint64_t* out) {
    if (!tables) return ctx->fail(STARK_ERR_INVALID_ARG, "mle_evaluate: null table array");
    if (!out) return ctx->fail(STARK_ERR_INVALID_ARG, "mle_evaluate: null out");
    if (!r && k) return ctx->fail(STARK_ERR_INVALID_ARG, "mle_evaluate: null r with k > 0");
    if (k > 40) return ctx->fail(STARK_ERR_INVALID_ARG, "mle_evaluate: k too large (at most 40)");
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + B * sizeof(fr_t), tbytes = sizeof(fr_t) << k;
    for (size_t b = 0; b < B; ++b) {
        if (!tables[b]) return ctx->fail(STARK_ERR_INVALID_ARG, "mle_evaluate: null table entry " + std::to_string(b));
        const uintptr_t t0 = (uintptr_t)tables[b];
        if (t0 < o1 && o0 < t0 + tbytes) return ctx->fail(STARK_ERR_INVALID_ARG, "mle_evaluate: out overlaps table " + std::to_string(b));
    }
    return STARK_OK;
}

}  // namespace

// ---- the streaming transcript as an object of the ABI (transcript/src/lib.rs:48-117) ------------------------------------------
struct stark_transcript { CtxRef ref_; DevTranscript T; explicit stark_transcript(stark_ctx* c) : T(c) { ref_.bind(c); } };

extern "C" {

// Transcript::new(label, default_params()) — the state lives on the device; absorbs are queued and run with the next challenge.
int32_t stark_transcript_new(stark_ctx_t* ctx, const uint8_t* label, size_t label_len, stark_transcript_t** out) {
    if (!ctx || !out || (!label && label_len)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    std::unique_ptr<stark_transcript> t(new stark_transcript(ctx));
    STARK_TRY(t->T.init(label, label_len));
    *out = t.release(); return STARK_OK;
}
int32_t stark_transcript_absorb_bytes(stark_transcript_t* t, const uint8_t* bytes, size_t n) { if (!t || (!bytes && n)) return STARK_ERR_INVALID_ARG; t->T.absorb_bytes(bytes, n); return STARK_OK; }
int32_t stark_transcript_absorb_fields(stark_transcript_t* t, const uint64_t* fields, size_t n) {
    if (!t || (!fields && n)) return STARK_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; ++i) t->T.absorb_field(load_fr(fields + 4 * i));
    return STARK_OK;
}
int32_t stark_transcript_challenge(stark_transcript_t* t, const uint8_t* label, size_t label_len, uint64_t* out4) {
    if (!t || !out4 || (!label && label_len)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(t->T.ctx));
    fr_t r; STARK_TRY(t->T.challenge(label, label_len, &r)); store_fr(out4, r); return STARK_OK;
}
// Transcript::challenges(label, n): challenge(label || le64(i)) for i < n (:103-112)
int32_t stark_transcript_challenges(stark_transcript_t* t, const uint8_t* label, size_t label_len, size_t n, uint64_t* out) {
    if (!t || (!out && n) || (!label && label_len)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(t->T.ctx));
    for (size_t i = 0; i < n; ++i) {
        std::vector<uint8_t> tag(label, label + label_len); for (int j = 0; j < 8; ++j) tag.push_back((uint8_t)((uint64_t)i >> (8 * j)));
        fr_t r; STARK_TRY(t->T.challenge(tag.data(), tag.size(), &r)); store_fr(out + 4 * i, r);
    }
    return STARK_OK;
}
int32_t stark_transcript_free(stark_transcript_t* t) { if (!t) return STARK_ERR_INVALID_ARG; delete t; return STARK_OK; }

// The reference's bench inputs (channel/benches/end_to_end.rs:249-253): `ncols` vectors of n elements drawn one after the other
// from ONE StdRng::seed_from_u64(seed) with ark-ff's Fp::rand (rand_core 0.6.4 PCG32 seed expansion, ChaCha12, rejection sampling of
// 255-bit candidates; the accepted limbs ARE the Montgomery representation).  Host-only: no context, no device.
int32_t stark_ref_bench_inputs(uint64_t seed, size_t n, size_t ncols, uint64_t* out) {
    if (!out && n * ncols) return STARK_ERR_INVALID_ARG;
    uint8_t key[32]; uint64_t state = seed;
    for (int c = 0; c < 8; ++c) {                                                          // SeedableRng::seed_from_u64
        state = state * 6364136223846793005ull + 11634580027462260723ull;
        const uint32_t xs = (uint32_t)(((state >> 18) ^ state) >> 27), rot = (uint32_t)(state >> 59);
        const uint32_t x = (xs >> rot) | (xs << ((32 - rot) & 31));
        key[4 * c] = (uint8_t)x; key[4 * c + 1] = (uint8_t)(x >> 8); key[4 * c + 2] = (uint8_t)(x >> 16); key[4 * c + 3] = (uint8_t)(x >> 24);
    }
    host::ChaCha12Rng rng(key);
    for (size_t i = 0; i < n * ncols; ++i) {
        for (;;) {                                                                         // Fp::rand: 4 limbs, top bit cleared, accept below the modulus
            uint64_t l[4]; for (int j = 0; j < 4; ++j) l[j] = rng.next_u64();
            l[3] &= 0x7FFFFFFFFFFFFFFFull;
            uint32_t t[9]; for (int j = 0; j < 4; ++j) { t[2 * j] = (uint32_t)l[j]; t[2 * j + 1] = (uint32_t)(l[j] >> 32); } t[8] = 0;
            if (fr_geq_p<PallasFr>(t)) continue;
            for (int j = 0; j < 4; ++j) out[4 * i + j] = l[j];
            break;
        }
    }
    return STARK_OK;
}

// CommitmentScheme for MerkleCommitment (commitment/src/lib.rs:80-114): arity 16, tree_label = cfg.ds_tag, parameters "POSEIDON-T17-X5-SEED".
int32_t stark_commitment_commit(stark_ctx_t* ctx, uint64_t ds_tag, const uint64_t* leaves, size_t n, stark_tree_t** out) {
    if (!ctx || !leaves || !out) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    stark_params* cp = nullptr; STARK_TRY(ctx_commit_params(ctx, &cp));
    DevBuf d; CallerUploads up(ctx); STARK_HIP(ctx, up.up(d, leaves, n * sizeof(fr_t)));
    std::unique_ptr<stark_tree> T;
    STARK_TRY(merkle_build_on(ctx, ctx->stream, cp, 16, ds_tag, d.fr(), n, 0, nullptr, 1, 0, 0, 0, DevBuf(), T));     // commit (:85-90); open = stark_merkle_open (:92-94)
    STARK_HIP(ctx, up.sync()); *out = T.release(); return STARK_OK;
}
// commit of `batch` DEVICE vectors of n leaves side by side (merkle_build_batch_on): stream-ordered, no host synchronisation
int32_t stark_commitment_commit_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* ds_tags, const uint64_t* const* leaves, size_t n, stark_tree_t** out) {
    if (!batch) return STARK_OK;
    if (!out) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad commitment batch args") : STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) out[b] = nullptr;
    if (!ctx || !ds_tags || !leaves) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad commitment batch args") : STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    stark_params* cp = nullptr; STARK_TRY(ctx_commit_params(ctx, &cp));
    return merkle_build_batch_on(ctx, cp, 16, batch, ds_tags, leaves, n, 0, nullptr, out);
}
// commit of `batch` DEVICE vectors of n[i] leaves each (merkle_build_mixed_batch_on): stream-ordered, no host synchronisation
int32_t stark_commitment_commit_mixed_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* ds_tags, const uint64_t* const* leaves, const size_t* n, stark_tree_t** out) {
    if (!batch) return STARK_OK;
    if (!out) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad commitment batch args") : STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) out[b] = nullptr;
    if (!ctx || !ds_tags || !leaves || !n) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad commitment batch args") : STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    stark_params* cp = nullptr; STARK_TRY(ctx_commit_params(ctx, &cp));
    return merkle_build_mixed_batch_on(ctx, cp, 16, batch, ds_tags, leaves, n, 0, nullptr, out);
}
// verify (:96-113): verify_many_ds with the static t = 17 parameters lifted to the dynamic form
int32_t stark_commitment_verify(stark_ctx_t* ctx, uint64_t ds_tag, const uint64_t* root4, const size_t* indices, size_t k, const uint64_t* values, const uint8_t* proof, size_t len, int32_t* accepted) {
    if (!ctx || !root4 || (!indices && k) || (!values && k) || (!proof && len) || !accepted) return STARK_ERR_INVALID_ARG;
    *accepted = 0;
    STARK_TRY(ctx_enter(ctx));
    stark_params* cp = nullptr; STARK_TRY(ctx_commit_params(ctx, &cp));
    return merkle_verify_one(ctx, cp, 16, ds_tag, root4, indices, k, values, nullptr, proof, len, accepted);      // MerkleCommitment's parameters
}

// Mle::evaluate(r) (channel/src/lib.rs:279-295): k folds layer[i] = (1 - r_j) layer[2i] + r_j layer[2i+1]; table of 2^k elements (host).
int32_t stark_mle_evaluate(stark_ctx_t* ctx, const uint64_t* table, size_t k, const uint64_t* r, uint64_t* out4) {
    if (!ctx || !table || (!r && k) || !out4 || k > 40) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const size_t n = (size_t)1 << k;
    DevBuf a, b; CallerUploads up(ctx); STARK_HIP(ctx, up.up(a, table, n * sizeof(fr_t))); STARK_HIP(ctx, b.alloc(ctx, std::max<size_t>(n / 2, 1) * sizeof(fr_t)));
    fr_t* cur = a.fr(); fr_t* nxt = b.fr(); size_t len = n;
    for (size_t j = 0; j < k; ++j) { STARK_TRY(fold(ctx, cur, len, load_fr(r + 4 * j), nxt)); std::swap(cur, nxt); len /= 2; }
    fr_t v; STARK_HIP(ctx, up.download_sync(&v, cur, sizeof(fr_t)));
    store_fr(out4, v); return STARK_OK;
}
// Mle::evaluate (:279-295) of `batch` device-resident tables, table i at the point r[i * k ..] (host): a few launches for the whole batch
// (mle_dev.hpp), stream-ordered, no synchronisation.  The host form above keeps its own path.
int32_t stark_mle_evaluate_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* tables, size_t k, const uint64_t* r, uint64_t* out) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!batch) return STARK_OK;
    STARK_TRY(mle_check_args(ctx, batch, tables, k, r, out));
    STARK_TRY(ctx_enter(ctx));
    return mle_evaluate_batch_impl(ctx, batch, tables, k, r, out);
}
int32_t stark_mle_evaluate_dev(stark_ctx_t* ctx, const uint64_t* table, size_t k, const uint64_t* r, uint64_t* out4) {
    return stark_mle_evaluate_batch_dev(ctx, 1, &table, k, r, out4);
}

int32_t stark_sumcheck_prove_plain_dev(stark_ctx_t* ctx, const uint64_t* witness, size_t k, uint64_t tree_label, stark_proof_t** out) {
    if (!ctx || !witness || !out) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return prove_sumcheck_mixed_impl(ctx, 0, 1, &witness, &k, &tree_label, 0, out);
}
int32_t stark_sumcheck_prove_mf_dev(stark_ctx_t* ctx, const uint64_t* witness, size_t k, uint64_t tree_label, size_t queries_per_round, stark_proof_t** out) {
    if (!ctx || !witness || !out) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return prove_sumcheck_mixed_impl(ctx, 1, 1, &witness, &k, &tree_label, queries_per_round, out);
}
int32_t stark_sumcheck_prove_plain(stark_ctx_t* ctx, const uint64_t* witness, size_t k, uint64_t tree_label, stark_proof_t** out) {
    if (!ctx || !witness || !out || k > 40) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    DevBuf d; CallerUploads up(ctx); STARK_HIP(ctx, up.up(d, witness, ((size_t)1 << k) * sizeof(fr_t)));
    return stark_sumcheck_prove_plain_dev(ctx, (const uint64_t*)d.p, k, tree_label, out);
}
int32_t stark_sumcheck_prove_mf(stark_ctx_t* ctx, const uint64_t* witness, size_t k, uint64_t tree_label, size_t queries_per_round, stark_proof_t** out) {
    if (!ctx || !witness || !out || k > 40) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    DevBuf d; CallerUploads up(ctx); STARK_HIP(ctx, up.up(d, witness, ((size_t)1 << k) * sizeof(fr_t)));
    return stark_sumcheck_prove_mf_dev(ctx, (const uint64_t*)d.p, k, tree_label, queries_per_round, out);
}
static int32_t prove_batch_dev(stark_ctx_t* ctx, int mf, size_t batch, const uint64_t* const* witnesses, size_t k, const uint64_t* tree_labels, size_t qpr, stark_proof_t** out) {
    if (!batch) return STARK_OK;
    if (out) for (size_t b = 0; b < batch; ++b) out[b] = nullptr;
    if (!ctx || !out || !witnesses || !tree_labels || k > 40) return STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) if (!witnesses[b]) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const std::vector<size_t> ks(batch, k);
    return prove_sumcheck_mixed_impl(ctx, mf, batch, witnesses, ks.data(), tree_labels, qpr, out);
}
static int32_t prove_mixed_batch_dev(stark_ctx_t* ctx, int mf, size_t batch, const uint64_t* const* witnesses, const size_t* k, const uint64_t* tree_labels, size_t qpr, stark_proof_t** out) {
    if (!batch) return STARK_OK;
    if (out) for (size_t b = 0; b < batch; ++b) out[b] = nullptr;
    if (!ctx || !out || !witnesses || !tree_labels || !k) return STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) if (!witnesses[b] || k[b] > 40) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return prove_sumcheck_mixed_impl(ctx, mf, batch, witnesses, k, tree_labels, qpr, out);
}
int32_t stark_sumcheck_prove_plain_mixed_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* witnesses, const size_t* k, const uint64_t* tree_labels, stark_proof_t** out) {
    return prove_mixed_batch_dev(ctx, 0, batch, witnesses, k, tree_labels, 0, out);
}
int32_t stark_sumcheck_prove_mf_mixed_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* witnesses, const size_t* k, const uint64_t* tree_labels, size_t queries_per_round,
                                                stark_proof_t** out) {
    return prove_mixed_batch_dev(ctx, 1, batch, witnesses, k, tree_labels, queries_per_round, out);
}
int32_t stark_sumcheck_prove_plain_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* witnesses, size_t k, const uint64_t* tree_labels, stark_proof_t** out) {
    return prove_batch_dev(ctx, 0, batch, witnesses, k, tree_labels, 0, out);
}
int32_t stark_sumcheck_prove_mf_batch_dev(stark_ctx_t* ctx, size_t batch, const uint64_t* const* witnesses, size_t k, const uint64_t* tree_labels, size_t queries_per_round,
                                          stark_proof_t** out) {
    return prove_batch_dev(ctx, 1, batch, witnesses, k, tree_labels, queries_per_round, out);
}
int32_t stark_sumcheck_verify_plain(stark_ctx_t* ctx, size_t k, uint64_t tree_label, const uint8_t* proof, size_t len, int32_t* accepted) {
    if (!ctx || (!proof && len) || !accepted) return STARK_ERR_INVALID_ARG;
    *accepted = 0;
    STARK_TRY(ctx_enter(ctx)); (void)k; (void)tree_label;     // verify_plain reads neither vk.k (it walks proof.rounds) nor the tree label
    return verify_sumcheck_batch_impl(ctx, 0, 1, &proof, &len, nullptr, accepted);
}
int32_t stark_sumcheck_verify_mf(stark_ctx_t* ctx, size_t k, uint64_t tree_label, size_t queries_per_round, const uint8_t* proof, size_t len, int32_t* accepted) {
    if (!ctx || (!proof && len) || !accepted) return STARK_ERR_INVALID_ARG;
    *accepted = 0;
    STARK_TRY(ctx_enter(ctx)); (void)k; (void)queries_per_round;
    return verify_sumcheck_batch_impl(ctx, 1, 1, &proof, &len, &tree_label, accepted);
}
// tree_labels: required by verify_mf; read by neither verify_plain nor its batch (may be NULL there).  k and queries_per_round are read by no verifier.
static int32_t verify_batch(stark_ctx_t* ctx, int mf, size_t batch, const uint8_t* const* proofs, const size_t* lens, const uint64_t* tree_labels, int32_t* accepted) {
    if (!batch) return STARK_OK;
    if (!accepted) return STARK_ERR_INVALID_ARG;
    memset(accepted, 0, batch * sizeof(int32_t));
    if (!ctx || !proofs || !lens || (mf && !tree_labels)) return STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) if (!proofs[b] && lens[b]) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return verify_sumcheck_batch_impl(ctx, mf, batch, proofs, lens, mf ? tree_labels : nullptr, accepted);
}
int32_t stark_sumcheck_verify_plain_batch(stark_ctx_t* ctx, size_t batch, const uint8_t* const* proofs, const size_t* lens, size_t k, const uint64_t* tree_labels, int32_t* accepted) {
    (void)k; return verify_batch(ctx, 0, batch, proofs, lens, tree_labels, accepted);
}
int32_t stark_sumcheck_verify_mf_batch(stark_ctx_t* ctx, size_t batch, const uint8_t* const* proofs, const size_t* lens, size_t k, const uint64_t* tree_labels, size_t queries_per_round,
                                       int32_t* accepted) {
    (void)k; (void)queries_per_round; return verify_batch(ctx, 1, batch, proofs, lens, tree_labels, accepted);
}

}  // extern "C"
