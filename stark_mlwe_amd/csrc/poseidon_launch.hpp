// stark_mlwe_amd/csrc/poseidon_launch.hpp — how the rest of the library launches Poseidon work: declarations only.  The kernels, the
// kernel-form selector and these launchers are defined once, in capi_poseidon.hip; every consumer (capi_fri.hip, capi_verify.hip,
// capi_sumcheck.hip) describes its sponges as a stream of poseidon_streams.hpp and calls one of these.
#pragma once
#include "ctx.hpp"
#include "poseidon_streams.hpp"

namespace stark {

void poseidon_set_attrs();                                           // per-device kernel attributes of every Poseidon kernel these can launch (stark_ctx_create)

// One launch of hash_with_ds_dynamic over the hashes of a DS stream on `st`, in the form the selector picks for a Merkle level of D.n_out nodes
// (DsStream: a Merkle level / pair-leaf level; DsGatherStream: one (width, depth) step of the batch verifiers; DsBatchStream: one level of B trees;
// DsBatchPairStream: the pair leaves of B unhashed FRI layers; DsBatchPairPtrStream: the pair leaves of B trees read through pointer tables;
// DsRaggedStream: one level, node or pair leaf, of trees of different lengths; DsRaggedPairStream: the pair leaves of unhashed FRI layers of different lengths).
int32_t hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsStream& D, fr_t* out);
int32_t hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsGatherStream& D, fr_t* out);
int32_t hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsBatchStream& D, fr_t* out);
int32_t hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsBatchPairStream& D, fr_t* out);
int32_t hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsBatchPairPtrStream& D, fr_t* out);
int32_t hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsRaggedStream& D, fr_t* out);
int32_t hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsRaggedPairStream& D, fr_t* out);
int32_t leaf_pair_hash_on(stark_ctx* ctx, hipStream_t st, const fr_t* f, const fr_t* f_next, size_t n, size_t m, fr_t* h);
// level0_block: a pooled block holding the leaves, moved into the tree as level 0; an empty one: level 0 is a copy of `leaves` (capi_poseidon.hip)
int32_t merkle_build_on(stark_ctx* ctx, hipStream_t st, stark_params* p, size_t arity, uint64_t label, const fr_t* leaves, size_t n, int pairs, const fr_t* cp, size_t cp_div,
                        uint64_t first_pos, uint32_t level0, size_t stop_at_len, DevBuf&& level0_block, std::unique_ptr<stark_tree>& out);
// MerkleTree::new / new_pairs of `batch` trees of one shape on the context's stream (merkle_batch.hpp): leaves / cp are HOST arrays of DEVICE pointers
// (cp: nullptr iff !pairs; a null entry = zeros).  Stream-ordered, no host synchronisation.  out: `batch` handles, all null on any error.
int32_t merkle_build_batch_on(stark_ctx* ctx, stark_params* p, size_t arity, size_t batch, const uint64_t* labels, const uint64_t* const* leaves, size_t n, int pairs,
                              const uint64_t* const* cp, stark_tree** out);
// The same of trees of DIFFERENT lengths n[b] >= 1 (merkle_build_mixed_batch): one launch per level over the trees that still have it.
int32_t merkle_build_mixed_batch_on(stark_ctx* ctx, stark_params* p, size_t arity, size_t batch, const uint64_t* labels, const uint64_t* const* leaves, const size_t* n, int pairs,
                                    const uint64_t* const* cp, stark_tree** out);

int32_t tr_hash_dev(stark_ctx* ctx, const char* tag, const fr_t* fields_dev, size_t k, size_t n, fr_t* out_dev);
int32_t tr_hash_columns4_dev(stark_ctx* ctx, const char* const tags[4], const fr_t* const cols[4], size_t n0, fr_t* out4_dev);
int32_t tr_hash_columns_batch_dev(stark_ctx* ctx, const char* const tags[4], const fr_t* const* ptrs_dev, size_t batch, size_t n0, fr_t* out_dev);
// n sponges of any tags and lengths in one launch (TrStream's Ragged layout); tags, fields (device pointers; null allowed iff k[i] == 0) and k on the host
int32_t tr_hash_many_dev(stark_ctx* ctx, size_t n, const char* const* tags, const fr_t* const* fields, const size_t* k, fr_t* out_dev, bool column_sponges);
int32_t tr_hash_host1(stark_ctx* ctx, const char* tag, const std::vector<fr_t>& fields, fr_t* out);   // one hash, host in/out

// One device-resident streaming transcript (17 elements at `state`, rate cursor *pos) on the context's stream: absorbs the n device fields, then
// (finish) permutes and squeezes state[0] into `out`.
int32_t tr_stream_on(stark_ctx* ctx, stark_params* tp, fr_t* state, uint32_t* pos, const fr_t* fields, size_t n, bool finish, fr_t* out);
// The active transcripts of a TrBatchStream on the context's stream, in the form the selector picks for n_for_form instances.  The batched provers
// pass 1 (they select as one instance does) and the batched verifiers T.n_active: that difference is inherited from the two launch sites this
// replaces, not designed.
int32_t tr_batch_on(stark_ctx* ctx, stark_params* tp, const TrBatchStream& T, size_t n_for_form);

}  // namespace stark
