// stark_mlwe_amd/csrc/capi_verify.hip — the verifier entry points of the C-ABI (next row N3): the walks of fri_verify.hpp planned over
// pool slots (fri_verify_batch.hpp, merkle_batch.hpp) and every plan run by ONE runner, run_verify_batch: one upload, the prover's leaf-pair
// kernel and one gathered DS launch per (width, depth), the check kernel, one download, one synchronisation.  A single call is a batch of one.
//   stark_deep_fri_verify            deep_fri_verify                    crates/deep_ali/src/fri.rs:643-762
//   stark_merkle_verify_many_ds      MerkleProver::verify_single        crates/merkle/src/lib.rs:587-722, 800-812
//   stark_merkle_verify_pairs_ds     MerkleProver::verify_pairs         crates/merkle/src/lib.rs:723-773, 841-855
//   stark_deep_fri_verify_batch      deep_fri_verify over many proofs
//   stark_merkle_verify_many_ds_batch  verify_many_ds over many openings
#include <cstring>
#include "verify_dev.hpp"
#include "fri_verify_batch.hpp"
#include "merkle_batch.hpp"

using namespace stark;

namespace stark {
// item b is accepted iff its host flag is set and every root it computed equals the one it claims (VerifyBatchPlan::chk); one thread per item
__global__ void __launch_bounds__(256) k_verify_batch_check(const fr_t* __restrict__ pool, const uint32_t* __restrict__ chk_off, const uint32_t* __restrict__ chk,
                                                            const int32_t* __restrict__ flag, size_t batch, int32_t* __restrict__ accepted) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    int32_t acc = flag[b];
    for (uint32_t j = chk_off[b]; j < chk_off[b + 1]; ++j) {
        const fr_t x = ldg(pool + chk[2 * j]), y = ldg(pool + chk[2 * j + 1]);
        for (int i = 0; i < 8; ++i) acc &= x.v[i] == y.v[i] ? 1 : 0;
    }
    accepted[b] = acc;
}

}  // namespace stark

// The leaf step and the DS groups of a plan whose arrays are on the device, in depth order on the context's stream (groups that share a
// depth after the first on the side stream, joined before the next depth).  fixed != nullptr: every group hashes with that parameter set
// (the sum-check openings: MerkleCommitment's) instead of ctx_merkle_params(G.t).  An error while forked drains both streams (StreamFork);
// any other leaves the context's stream to the caller, who drains it for its staging vector anyway.
int32_t stark::verify_batch_groups_on(stark_ctx* ctx, const VerifyBatchPlan& V, const uint64_t* hdr, const uint32_t* off, const uint32_t* idx, fr_t* pool, stark_params* fixed) {
    hipStream_t main_st = ctx->stream; StreamFork fk(ctx);
    for (size_t g0 = 0, depth = 1; g0 < V.groups.size() || (depth == 1 && V.nl); ++depth) {
        // the launches of this depth: the leaf step (depth 1), then the DS groups of each width
        std::vector<int> items; if (depth == 1 && V.nl) items.push_back(-1);
        size_t g1 = g0; while (g1 < V.groups.size() && V.groups[g1].depth == depth) items.push_back((int)g1++);
        for (size_t i = 0; i < items.size(); ++i) {
            if (i == 1) STARK_TRY(fk.fork());                          // the rest of this depth on the side stream
            const hipStream_t st = i >= 1 ? fk.side : main_st;
            int32_t rc = STARK_OK;
            if (items[i] < 0) rc = leaf_pair_hash_on(ctx, st, pool + V.leaf_f0, pool + V.leaf_f0 + V.nl, V.nl, 1, pool + V.leaf_out0);
            else {
                const VerifyBatchPlan::Group& G = V.groups[items[i]];
                stark_params* mp = fixed; if (!mp) rc = ctx_merkle_params(ctx, G.t, &mp);
                const DsGatherStream D{hdr + 4 * G.job0, off + G.job0, idx, pool, G.n, G.max_children};
                if (!rc) rc = hash_ds_on(ctx, st, mp, D, pool + G.out0);
            }
            STARK_TRY(rc);
        }
        STARK_TRY(fk.join());                                          // before the next depth reads these digests (nothing when this depth did not fork)
        g0 = g1;
    }
    return STARK_OK;
}
// Runs one plan (a DEEP-FRI one or a Merkle one): one upload of everything the device reads (the computed digests are not sent), the leaf step and
// the DS groups in depth order (verify_batch_groups_on), the check kernel, one download of the decisions and one synchronisation.  Once the upload
// is enqueued every error drains the streams before the staging vector dies (the CallerUploads guard).
int32_t stark::run_verify_batch(stark_ctx* ctx, const VerifyBatchPlan& V, stark_params* fixed, int32_t* accepted) {
    if (!V.batch) return STARK_OK;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_hdr = 0, o_off = al(o_hdr + V.hdr.size() * 8), o_idx = al(o_off + V.off.size() * 4), o_coff = al(o_idx + V.idx.size() * 4),
                 o_chk = al(o_coff + V.chk_off.size() * 4), o_flag = al(o_chk + V.chk.size() * 4), o_pool = al(o_flag + V.batch * 4),
                 o_acc = al(o_pool + V.pool.size() * sizeof(fr_t)), total = al(o_acc + V.batch * 4);
    std::vector<uint8_t> h(o_pool + V.n_known * sizeof(fr_t));
    auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) memcpy(h.data() + o, src, bytes); };
    put(o_hdr, V.hdr.data(), V.hdr.size() * 8); put(o_off, V.off.data(), V.off.size() * 4); put(o_idx, V.idx.data(), V.idx.size() * 4);
    put(o_coff, V.chk_off.data(), V.chk_off.size() * 4); put(o_chk, V.chk.data(), V.chk.size() * 4); put(o_flag, V.flag.data(), V.batch * 4);
    put(o_pool, V.pool.data(), V.n_known * sizeof(fr_t));
    DevBuf d; STARK_HIP(ctx, d.alloc(ctx, total));
    uint8_t* base = (uint8_t*)d.p; fr_t* pool = (fr_t*)(base + o_pool); int32_t* acc_dev = (int32_t*)(base + o_acc);
    hipStream_t st = ctx->stream;
    CallerUploads up(ctx);                                                           // h is not copied again: every return below is fenced (verify_batch_groups_on drains its side stream itself)
    if (up.copy(base, h.data(), h.size()) != hipSuccess) return ctx->fail(STARK_ERR_HIP, "verify batch: upload");
    STARK_TRY(verify_batch_groups_on(ctx, V, (const uint64_t*)(base + o_hdr), (const uint32_t*)(base + o_off), (const uint32_t*)(base + o_idx), pool, fixed));
    hipLaunchKernelGGL(k_verify_batch_check, dim3((unsigned)((V.batch + 255) / 256)), dim3(256), 0, st, (const fr_t*)pool, (const uint32_t*)(base + o_coff), (const uint32_t*)(base + o_chk),
                       (const int32_t*)(base + o_flag), V.batch, acc_dev);
    if (hipGetLastError() != hipSuccess) return ctx->fail(STARK_ERR_HIP, "verify batch: check");
    STARK_HIP(ctx, up.download_sync(accepted, acc_dev, V.batch * 4));
    return STARK_OK;
}
// A plan is run once it holds this many pool slots (1 GiB of field elements), so device memory stays bounded whatever the batch.
static const size_t kVerifyBatchMaxSlots = (size_t)1 << 25;
// finishes and runs what a planner holds; `what`: the items of the entry point, for the message of one that a plan cannot index
template <class Planner>
static int32_t run_planned(stark_ctx* ctx, Planner& pl, stark_params* fixed, const char* what, int32_t* accepted) {
    if (!pl.fits_u32()) return ctx->fail(STARK_ERR_INVALID_ARG, std::string(what) + " of the batch needs more than 2^31 pool slots");
    VerifyBatchPlan V; pl.finish(V);
    return run_verify_batch(ctx, V, fixed, accepted);
}
int32_t stark::merkle_verify_one(stark_ctx* ctx, stark_params* fixed, size_t cfg_arity, uint64_t label, const uint64_t* root4, const size_t* idx, size_t k, const uint64_t* values,
                                 const uint64_t* cp_values, const uint8_t* proof, size_t len, int32_t* accepted) {
    MerkleVerifyPlanner pl; pl.add(cfg_arity, label, root4, idx, k, values, cp_values, proof, len);
    const int32_t rc = run_planned(ctx, pl, fixed, "an opening", accepted);
    if (rc) *accepted = 0;
    return rc;
}

extern "C" {

int32_t stark_deep_fri_verify(stark_ctx_t* ctx, const uint8_t* proof, size_t len, const size_t* schedule, size_t L, size_t r, uint64_t seed_z, int32_t* accepted) {
    if (!ctx || (!proof && len) || (!schedule && L) || !accepted) return STARK_ERR_INVALID_ARG;
    *accepted = 0;
    STARK_TRY(ctx_enter(ctx));
    (void)seed_z;   // DeepFriParams.seed_z is carried for signature parity: the reference's verifier never reads it (fri.rs:643-762)
    VerifyBatchPlanner pl; pl.add(proof, len, schedule, L, r);                     // not a well-formed proof: planned as a rejection
    const int32_t rc = run_planned(ctx, pl, nullptr, "a proof", accepted);
    if (rc) *accepted = 0;
    return rc;
}

int32_t stark_deep_fri_verify_batch(stark_ctx_t* ctx, size_t batch, const uint8_t* const* proofs, const size_t* lens, const size_t* schedule, size_t L, size_t r, uint64_t seed_z,
                                    int32_t* accepted) {
    if (!batch) return STARK_OK;
    if (!accepted) return STARK_ERR_INVALID_ARG;
    memset(accepted, 0, batch * sizeof(int32_t));
    if (!ctx || !proofs || !lens || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) if (!proofs[b] && lens[b]) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    (void)seed_z;   // carried for signature parity, as in stark_deep_fri_verify
    size_t b0 = 0;
    while (b0 < batch) {
        VerifyBatchPlanner pl; size_t b1 = b0;
        while (b1 < batch && (b1 == b0 || pl.slots() < kVerifyBatchMaxSlots)) { pl.add(proofs[b1], lens[b1], schedule, L, r); ++b1; }
        const int32_t rc = run_planned(ctx, pl, nullptr, "a proof", accepted + b0);
        if (rc) { memset(accepted, 0, batch * sizeof(int32_t)); return rc; }
        b0 = b1;
    }
    return STARK_OK;
}

static int32_t merkle_verify(stark_ctx_t* ctx, int pairs, size_t cfg_arity, uint64_t tree_label, const uint64_t* root4, const size_t* idx, size_t k, const uint64_t* values, const uint64_t* cp,
                             const uint8_t* proof, size_t len, int32_t* accepted) {
    if (!ctx || !root4 || (!idx && k) || (!values && k) || (pairs && !cp && k) || (!proof && len) || !accepted) return STARK_ERR_INVALID_ARG;
    *accepted = 0;
    STARK_TRY(ctx_enter(ctx));
    if (host::width_for_arity(cfg_arity) < 0 || cfg_arity == 0) return ctx->fail(STARK_ERR_UNSUPPORTED, "unsupported Merkle arity; max supported = 128");   // MerkleChannelCfg::new (poseidon/src/lib.rs:164)
    // pairs with k == 0 and no cp plans as verify_many_ds: both reject an empty index list
    return merkle_verify_one(ctx, nullptr, cfg_arity, tree_label, root4, idx, k, values, pairs ? cp : nullptr, proof, len, accepted);
}
int32_t stark_merkle_verify_many_ds(stark_ctx_t* ctx, size_t cfg_arity, uint64_t tree_label, const uint64_t* root4, const size_t* indices, size_t k, const uint64_t* values,
                                    const uint8_t* proof, size_t len, int32_t* accepted) {
    return merkle_verify(ctx, 0, cfg_arity, tree_label, root4, indices, k, values, nullptr, proof, len, accepted);
}
int32_t stark_merkle_verify_pairs_ds(stark_ctx_t* ctx, size_t cfg_arity, uint64_t tree_label, const uint64_t* root4, const size_t* indices, size_t k, const uint64_t* f_vals, const uint64_t* cp_vals,
                                     const uint8_t* proof, size_t len, int32_t* accepted) {
    return merkle_verify(ctx, 1, cfg_arity, tree_label, root4, indices, k, f_vals, cp_vals, proof, len, accepted);
}
int32_t stark_merkle_verify_many_ds_batch(stark_ctx_t* ctx, size_t cfg_arity, size_t batch, const uint64_t* tree_labels, const uint64_t* roots, const size_t* indices, const size_t* idx_off,
                                          const uint64_t* values, const uint8_t* const* proofs, const size_t* lens, int32_t* accepted) {
    if (!batch) return STARK_OK;
    if (!accepted) return STARK_ERR_INVALID_ARG;
    memset(accepted, 0, batch * sizeof(int32_t));
    if (!ctx || !tree_labels || !roots || !idx_off || !proofs || !lens) return STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) if ((!proofs[b] && lens[b]) || idx_off[b + 1] < idx_off[b]) return STARK_ERR_INVALID_ARG;
    if ((!indices || !values) && idx_off[batch] != idx_off[0]) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (host::width_for_arity(cfg_arity) < 0 || cfg_arity == 0) return ctx->fail(STARK_ERR_UNSUPPORTED, "unsupported Merkle arity; max supported = 128");   // MerkleChannelCfg::new (poseidon/src/lib.rs:164)
    auto run = [&](const VerifyBatchPlan& V, int32_t* acc) { return run_verify_batch(ctx, V, nullptr, acc); };
    int32_t rc = merkle_verify_batch(run, cfg_arity, batch, tree_labels, roots, indices, idx_off, values, proofs, lens, kVerifyBatchMaxSlots, accepted);
    if (rc == -1) rc = ctx->fail(STARK_ERR_INVALID_ARG, "an opening of the batch needs more than 2^31 pool slots");
    if (rc) memset(accepted, 0, batch * sizeof(int32_t));
    return rc;
}

}  // extern "C"
