// stark_mlwe_amd/csrc/verify_dev.hpp — what the device-backed verifiers share (capi_verify.hip, capi_sumcheck.hip): the VerifyHasher of
// fri_verify.hpp over the GPU kernels, and the leaf step and DS groups of a batch plan.
#pragma once
#include "fri_verify.hpp"
#include "poseidon_launch.hpp"

namespace stark {

// host vectors -> pooled device buffers -> kernel -> host (a few hundred hashes per call; one synchronisation each).  fixed != nullptr: the DS
// hashes use that parameter set (the sum-check openings: MerkleCommitment's, a t = 17 set that is NOT poseidon_params_for_arity(16)) instead
// of ctx_merkle_params(width_for_arity(arity)).
struct GpuVerifyHasher : VerifyHasher {
    stark_ctx* ctx; stark_params* fixed;
    explicit GpuVerifyHasher(stark_ctx* c, stark_params* fixed_ = nullptr) : ctx(c), fixed(fixed_) {}
    int32_t params(size_t arity, stark_params** mp) { *mp = fixed; return fixed ? STARK_OK : ctx_merkle_params(ctx, host::width_for_arity(arity), mp); }
    int32_t leaf_pairs(const fr_t* f, const fr_t* s, size_t n, fr_t* out) override {
        if (!n) return STARK_OK;
        DevBuf df, ds, dh; STARK_HIP(ctx, df.upload(ctx, f, n * sizeof(fr_t))); STARK_HIP(ctx, ds.upload(ctx, s, n * sizeof(fr_t))); STARK_HIP(ctx, dh.alloc(ctx, n * sizeof(fr_t)));
        STARK_TRY(leaf_pair_hash_on(ctx, ctx->stream, df.fr(), ds.fr(), n, 1, dh.fr()));
        STARK_HIP(ctx, dh.download_sync(out, n * sizeof(fr_t))); return STARK_OK;
    }
    int32_t ds_nodes(size_t arity, size_t chunk, uint32_t level, uint64_t label, const uint64_t* positions, const fr_t* children, size_t n, fr_t* out) override {
        if (!n) return STARK_OK;
        stark_params* mp = nullptr; STARK_TRY(params(arity, &mp));
        DevBuf dp, dc, dout; STARK_HIP(ctx, dp.upload(ctx, positions, n * 8)); STARK_HIP(ctx, dc.upload(ctx, children, n * chunk * sizeof(fr_t))); STARK_HIP(ctx, dout.alloc(ctx, n * sizeof(fr_t)));
        STARK_TRY(hash_ds_scattered(ctx, mp, 0, arity, chunk, level, label, (const uint64_t*)dp.p, dc.fr(), nullptr, n, dout.fr()));
        STARK_HIP(ctx, dout.download_sync(out, n * sizeof(fr_t))); return STARK_OK;
    }
    int32_t ds_pair_leaves(size_t arity, uint64_t label, const uint64_t* positions, const fr_t* f, const fr_t* cp, size_t n, fr_t* out) override {
        if (!n) return STARK_OK;
        stark_params* mp = nullptr; STARK_TRY(params(arity, &mp));
        DevBuf dp, df, dc, dout; STARK_HIP(ctx, dp.upload(ctx, positions, n * 8)); STARK_HIP(ctx, df.upload(ctx, f, n * sizeof(fr_t))); STARK_HIP(ctx, dc.upload(ctx, cp, n * sizeof(fr_t))); STARK_HIP(ctx, dout.alloc(ctx, n * sizeof(fr_t)));
        STARK_TRY(hash_ds_scattered(ctx, mp, 1, arity, arity, 0xFFFFFFFFu, label, (const uint64_t*)dp.p, df.fr(), dc.fr(), n, dout.fr()));
        STARK_HIP(ctx, dout.download_sync(out, n * sizeof(fr_t))); return STARK_OK;
    }
};

// The leaf step and the DS groups of a batch plan whose arrays are on the device (capi_verify.hip); fixed != nullptr: every group hashes with that set.
struct VerifyBatchPlan;
int32_t verify_batch_groups_on(stark_ctx* ctx, const VerifyBatchPlan& V, const uint64_t* hdr, const uint32_t* off, const uint32_t* idx, fr_t* pool, stark_params* fixed);

}  // namespace stark
