// stark_mlwe_amd/csrc/verify_dev.hpp — what the device-backed verifiers share (capi_verify.hip, capi_sumcheck.hip): how a batch plan
// (fri_verify_batch.hpp) runs on the device.  Defined in capi_verify.hip.
#pragma once
#include "fri_verify.hpp"
#include "poseidon_launch.hpp"

namespace stark {

struct VerifyBatchPlan;
// The leaf step and the DS groups of a batch plan whose arrays are on the device; fixed != nullptr: every group hashes with that parameter set (the
// sum-check openings: MerkleCommitment's, a t = 17 set that is NOT poseidon_params_for_arity(16)) instead of ctx_merkle_params(width of the group).
// On an error the side stream is drained if a depth was forked (StreamFork); the context's stream is the CALLER's to drain before it frees what the launches read.
int32_t verify_batch_groups_on(stark_ctx* ctx, const VerifyBatchPlan& V, const uint64_t* hdr, const uint32_t* off, const uint32_t* idx, fr_t* pool, stark_params* fixed);
// Runs one plan whole: one upload, verify_batch_groups_on, the check kernel, one download of accepted[0 .. V.batch) and one synchronisation.
int32_t run_verify_batch(stark_ctx* ctx, const VerifyBatchPlan& V, stark_params* fixed, int32_t* accepted);
// verify_many_ds (cp_values == nullptr) / verify_pairs_ds of ONE opening: a plan of one item through run_verify_batch.  The caller has set *accepted = 0; it stays 0 on a reject and on an error.
int32_t merkle_verify_one(stark_ctx* ctx, stark_params* fixed, size_t cfg_arity, uint64_t label, const uint64_t* root4, const size_t* idx, size_t k, const uint64_t* values,
                          const uint64_t* cp_values, const uint8_t* proof, size_t len, int32_t* accepted);

}  // namespace stark
