// stark_mlwe_amd/csrc/merkle_batch.hpp — MerkleTree::new / new_pairs, open_union_of_paths and verify_many_ds (crates/merkle/src/lib.rs:147-193,
// 392-445, 246-315, 587-722) of MANY trees in one pass: the drivers written once, over an executor that runs the batched kernels
// (capi_poseidon.hip, capi_verify.hip: the device; hostcheck.cpp: the same stream bodies on the host).
//
//   build   `batch` trees of one shape (arity, n, pairs).  Level v of all trees is ONE block of batch x lens[v] elements, tree b's level the slice at
//           b * lens[v]: level 0 is one copy (or one pair-leaf launch) through the pointer tables, every level above one DsBatchStream launch.
//           Trees of different lengths: merkle_build_mixed_batch, level v one block of the slices of the trees that still have it (DsRaggedStream).
//   open    any trees of one context: every tree is planned on the host (merkle_open_from over a recording source), all siblings of all trees and
//           levels come back with ONE gather, and each proof is encoded with enc_mproof.  stark_merkle_open is this with one tree.
//   verify  every opening is parsed (dec_mproof) and walked over pool slots (DsJobPlanner) into the plan shape of fri_verify_batch.hpp; what runs the
//           plan makes one launch per (width, depth) and compares each item's computed root with the claimed one.  The single verify calls are a batch of one.
// Element i of every result equals what the single call returns for item i alone, byte for byte.  Host-only C++ (no HIP).
#pragma once
#include <cstdint>
#include <map>
#include <vector>
#include "fr.hpp"
#include "poseidon_streams.hpp"
#include "fri_plan.hpp"
#include "fri_verify_batch.hpp"

namespace stark {

#define MB_TRY(e) do { int32_t rc__ = (e); if (rc__) return rc__; } while (0)

// The level lengths of a tree of n leaves (merkle/src/lib.rs:166-190); n = 1 is the one level whose only element is the root.
inline std::vector<size_t> merkle_level_lens(size_t n, size_t arity) {
    std::vector<size_t> lens(1, n);
    while (lens.back() > 1) lens.push_back((lens.back() + arity - 1) / arity);
    return lens;
}

// ---- build ------------------------------------------------------------------------------------------------------------------------------------
// An executor X provides (pointers are its own memory: device pointers on the GPU, host pointers in the host check):
//   int32_t level_block(size_t n_fr, fr_t** out)      the block of one level of all trees; it lives as long as the trees do
//   int32_t tables(const uint64_t* labels, const fr_t* const* leaves, const fr_t* const* cp, size_t B,
//                  const uint64_t** labels_x, const fr_t* const** leaves_x, const fr_t* const** cp_x)
//                                                      the labels and pointer tables in X's memory (cp == nullptr: *cp_x = nullptr); the caller's arrays may die on return
//   int32_t copy_rows(const fr_t* const* src_x, size_t n, size_t B, fr_t* dst)          dst[b n + i] = src[b][i]
//   int32_t pair_level(const DsBatchPairPtrStream& D, fr_t* out)
//   int32_t ds_level(const DsBatchStream& D, fr_t* out)
// lens[v] / base[v]: the length of level v and the block that holds it for all trees.  The argument checks are the caller's (merkle_build_on's).
template <class X>
inline int32_t merkle_build_batch(X& x, size_t arity, size_t B, const uint64_t* labels, const fr_t* const* leaves, size_t n, int pairs, const fr_t* const* cp,
                                  std::vector<size_t>& lens, std::vector<fr_t*>& base) {
    lens = merkle_level_lens(n, arity); base.assign(lens.size(), nullptr);
    const uint64_t* labels_x = nullptr; const fr_t* const* leaves_x = nullptr; const fr_t* const* cp_x = nullptr;
    MB_TRY(x.tables(labels, leaves, pairs ? cp : nullptr, B, &labels_x, &leaves_x, &cp_x));
    MB_TRY(x.level_block(B * n, &base[0]));
    if (pairs) MB_TRY(x.pair_level(DsBatchPairPtrStream::make(arity, labels_x, leaves_x, cp_x, n, B), base[0]));     // new_pairs (:380-388, 392-414)
    else MB_TRY(x.copy_rows(leaves_x, n, B, base[0]));                                                                // new: the leaves are level 0
    for (size_t v = 1; v < lens.size(); ++v) {                                                                        // :163-179
        MB_TRY(x.level_block(B * lens[v], &base[v]));
        MB_TRY(x.ds_level(DsBatchStream::make(arity, (uint32_t)(v - 1), 0, labels_x, nullptr, base[v - 1], lens[v - 1], B), base[v]));
    }
    return 0;
}

// ---- build, trees of different lengths ------------------------------------------------------------------------------------------------------------
// `B` trees of one arity and parameter set, tree b of n[b] >= 1 leaves.  Level v of the call is ONE block: the slices of the trees that have more
// than v levels, back to back in tree order (a tree of one leaf has its one level and no hash; trees drop out as they reach their root).  Level 0 is
// one ragged copy (or one ragged pair-leaf launch), every level above one DsRaggedStream launch over the trees that still have it.  All blocks are
// taken first, so every segment table of the call is built on the host and goes up as ONE table.
// An executor X provides (level_block as above):
//   int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** x)   the table in X's memory; `h` may die on return
//   int32_t copy_ragged(const DsRaggedStream& D, fr_t* dst)                                      dst[first_s + j] = in0_s[j] (D of mode 1)
//   int32_t ragged_level(const DsRaggedStream& D, fr_t* out)
// lens[b]: the level lengths of tree b; at[b][v]: where its level v starts in base[v].  The argument checks are the caller's.
template <class X>
inline int32_t merkle_build_mixed_batch(X& x, size_t arity, size_t B, const uint64_t* labels, const fr_t* const* leaves, const size_t* n, int pairs, const fr_t* const* cp,
                                        std::vector<std::vector<size_t>>& lens, std::vector<std::vector<size_t>>& at, std::vector<fr_t*>& base) {
    lens.assign(B, {}); at.assign(B, {}); size_t depth = 0;
    for (size_t b = 0; b < B; ++b) { lens[b] = merkle_level_lens(n[b], arity); at[b].assign(lens[b].size(), 0); depth = std::max(depth, lens[b].size()); }
    std::vector<size_t> block(depth, 0);
    for (size_t v = 0; v < depth; ++v) for (size_t b = 0; b < B; ++b) if (lens[b].size() > v) { at[b][v] = block[v]; block[v] += lens[b][v]; }
    base.assign(depth, nullptr);
    for (size_t v = 0; v < depth; ++v) MB_TRY(x.level_block(block[v], &base[v]));
    // table 0: the leaves (pair-leaf mode; the plain copy reads the same table), table v >= 1: the node level that turns level v - 1 into level v
    std::vector<DsRaggedTable> T(depth);
    for (size_t b = 0; b < B; ++b) T[0].add(1, arity, leaves[b], pairs ? cp[b] : nullptr, n[b], labels[b]);
    for (size_t v = 1; v < depth; ++v) for (size_t b = 0; b < B; ++b) if (lens[b].size() > v) T[v].add(0, arity, base[v - 1] + at[b][v - 1], nullptr, lens[b][v - 1], labels[b]);
    std::vector<DsRaggedStream::Seg> all; std::vector<size_t> t0(depth);
    for (size_t v = 0; v < depth; ++v) { t0[v] = all.size(); all.insert(all.end(), T[v].segs.begin(), T[v].segs.end()); }
    const DsRaggedStream::Seg* sx = nullptr; MB_TRY(x.segments(all, &sx));
    const DsRaggedStream L0 = DsRaggedStream::make(1, arity, 0xFFFFFFFFu, 0, sx, B, T[0].n_out);
    if (pairs) MB_TRY(x.ragged_level(L0, base[0]));                                                                   // new_pairs (:380-388, 392-414)
    else MB_TRY(x.copy_ragged(L0, base[0]));                                                                          // new: the leaves are level 0
    for (size_t v = 1; v < depth; ++v)                                                                                // :163-179
        MB_TRY(x.ragged_level(DsRaggedStream::make(0, arity, (uint32_t)(v - 1), 0, sx + t0[v], T[v].segs.size(), T[v].n_out), base[v]));
    return 0;
}

// ---- open -------------------------------------------------------------------------------------------------------------------------------------
// A tree as the open driver sees it: its arity, level lengths and level arrays (in the executor's memory).
struct MerkleTreeView { size_t arity; const std::vector<size_t>* lens; const fr_t* const* levels; };
// The reads of ONE row gather — the openings of a batch of trees, the opened values of a query phase: request i is element index[i] of the array
// base[src[i]] (each source array once in `base`, however often it is read) and lands in row i of the result, or in row[i] when the list carries
// explicit rows (add(); all requests of a list or none: a sharded query phase fills only its own rank's rows of a zeroed table).
struct MerkleGatherList {
    std::vector<const fr_t*> base; std::vector<uint32_t> src; std::vector<uint64_t> index, row;
    std::map<const fr_t*, uint32_t> slot;
    uint32_t slot_of(const fr_t* from) {
        auto it = slot.emplace(from, (uint32_t)base.size()).first;
        if (it->second == base.size()) base.push_back(from);
        return it->second;
    }
    void level(const fr_t* from, const std::vector<size_t>& idx) { const uint32_t s = slot_of(from); for (size_t i : idx) { src.push_back(s); index.push_back((uint64_t)i); } }
    void add(const fr_t* from, uint64_t i, uint64_t to_row) { src.push_back(slot_of(from)); index.push_back(i); row.push_back(to_row); }
    size_t size() const { return src.size(); }
    uint64_t row_of(size_t i) const { return row.empty() ? (uint64_t)i : row[i]; }
};
// -1: a non-monotone idx_off, an empty index list (open_many, :247) or a leaf index out of range — found before anything is read.
// An executor X provides   int32_t gather(const MerkleGatherList& G, fr_t* out_host)   (one launch, one download, one synchronisation).
template <class X>
inline int32_t merkle_open_batch(X& x, const MerkleTreeView* trees, size_t B, const size_t* idx, const size_t* idx_off, std::vector<std::vector<uint8_t>>& proofs) {
    struct Recorder : FriSource {
        const MerkleTreeView* t; MerkleGatherList& G;
        Recorder(const MerkleTreeView* t_, MerkleGatherList& g) : t(t_), G(g) {}
        int32_t layer(size_t, const std::vector<size_t>&, std::vector<fr_t>&) override { return -1; }
        int32_t digests(size_t tree, size_t level, const std::vector<size_t>& ix, std::vector<fr_t>& out) override {
            G.level(t[tree].levels[level], ix); out.assign(ix.size(), fr_zero<PallasFr>()); return 0;
        }
    };
    for (size_t b = 0; b < B; ++b) {
        if (idx_off[b + 1] <= idx_off[b]) return -1;
        for (size_t j = idx_off[b]; j < idx_off[b + 1]; ++j) if (idx[j] >= (*trees[b].lens)[0]) return -1;
    }
    MerkleGatherList G; Recorder rec(trees, G);
    std::vector<MerkleProofHost> pr(B);
    for (size_t b = 0; b < B; ++b)
        MB_TRY(merkle_open_from(rec, b, *trees[b].lens, trees[b].arity, std::vector<size_t>(idx + idx_off[b], idx + idx_off[b + 1]), pr[b]));
    std::vector<fr_t> got(G.size());
    if (G.size()) MB_TRY(x.gather(G, got.data()));
    proofs.assign(B, {}); const fr_t* g = got.data();
    for (size_t b = 0; b < B; ++b) {                                   // the siblings in request order: tree by tree, level by level
        for (auto& l : pr[b].siblings) for (auto& s : l) s = *g++;
        enc_mproof(proofs[b], pr[b]);
    }
    return 0;
}

// ---- verify -----------------------------------------------------------------------------------------------------------------------------------
// Plans verify_many_ds (cp_values == nullptr) or verify_pairs_ds of one opening at a time.  Every input slot holds a field element the caller handed
// over (values in the stored form; siblings decoded from the proof bytes; the claimed root).  After finish(): an accepted item has flag 1 and one
// check (the root its walk computed, the root it claims); a rejected item keeps no job, an empty check range and flag 0.
class MerkleVerifyPlanner : public DsJobPlanner {
public:
    // root4 / values / cp_values: the caller's host words, four per element, at whatever alignment a uint64_t has (an fr_t is 16-byte aligned: never cast)
    void add(size_t cfg_arity, uint64_t label, const uint64_t* root4, const size_t* idx, size_t k, const uint64_t* values, const uint64_t* cp_values, const uint8_t* proof, size_t len) {
        const JobMark m = job_mark(); bool ok = false;
        ByteReader R(proof, len); MerkleProofHost pr;
        if (dec_mproof(R, pr) && !R.left()) {                          // bytes that do not decode: a rejection
            const std::vector<size_t> ix(idx, idx + k); std::vector<uint32_t> v, c;
            for (size_t i = 0; i < k; ++i) { v.push_back(input(words(values + 4 * i))); if (cp_values) c.push_back(input(words(cp_values + 4 * i))); }
            auto sib = [&](size_t level, size_t j) { return input(pr.siblings[level][j]); };
            auto root = [&]() { return input(words(root4)); };
            ok = cp_values ? pairs_rooted(cfg_arity, ix, v, c, pr, label, sib, root) : many_rooted(cfg_arity, ix, v, pr, label, sib, root);
        }
        if (!ok) { job_rollback(m); pool_.resize(m.in); }
        end_item(ok);
    }
    size_t items() const { return flag_.size(); }
    size_t slots() const { return pool_.size() + n_comp_; }
    bool fits_u32() const { return slots() < kComputed && ch_.size() < kComputed; }
    void finish(VerifyBatchPlan& o) const {
        o = VerifyBatchPlan(); finish_items(o); o.n_known = pool_.size();
        std::vector<uint32_t> pos(n_comp_);
        const size_t total = finish_jobs(o, pos, pool_.size());
        o.pool.assign(total, fr_zero<PallasFr>()); std::copy(pool_.begin(), pool_.end(), o.pool.begin());
    }
private:
    std::vector<fr_t> pool_;
    uint32_t input(const fr_t& x) { pool_.push_back(x); return new_input(); }
    static fr_t words(const uint64_t* p) { fr_t x; for (int i = 0; i < 4; ++i) { x.v[2 * i] = (uint32_t)p[i]; x.v[2 * i + 1] = (uint32_t)(p[i] >> 32); } return x; }
};
// verify_many_ds of `batch` openings: item i opens indices[idx_off[i] .. idx_off[i + 1]) with values[4 x the same range] against roots[4 i ..] under
// labels[i] (roots and values as uint64_t words, read at their own alignment).  A plan is run once it holds max_slots pool slots, so the memory of
// whatever runs it stays bounded whatever the batch.  run(V, accepted) runs one plan: the DS groups of V in depth order, then its checks.
// -1: an item that needs more than 2^31 pool slots.
template <class Run>
inline int32_t merkle_verify_batch(Run run, size_t cfg_arity, size_t batch, const uint64_t* labels, const uint64_t* roots, const size_t* indices, const size_t* idx_off,
                                   const uint64_t* values, const uint8_t* const* proofs, const size_t* lens, size_t max_slots, int32_t* accepted) {
    size_t b0 = 0;
    while (b0 < batch) {
        MerkleVerifyPlanner pl; size_t b1 = b0;
        while (b1 < batch && (b1 == b0 || pl.slots() < max_slots)) {
            pl.add(cfg_arity, labels[b1], roots + 4 * b1, indices + idx_off[b1], idx_off[b1 + 1] - idx_off[b1], values + 4 * idx_off[b1], nullptr, proofs[b1], lens[b1]); ++b1;
        }
        if (!pl.fits_u32()) return -1;
        VerifyBatchPlan V; pl.finish(V);
        MB_TRY(run(V, accepted + b0));
        b0 = b1;
    }
    return 0;
}
#undef MB_TRY

}  // namespace stark
