// stark_mlwe_amd/csrc/merkle_batch.hpp — MerkleTree::new / new_pairs, open_union_of_paths and verify_many_ds (crates/merkle/src/lib.rs:147-193,
// 392-445, 246-315, 587-722) of MANY trees in one pass: the drivers written once, over an executor that runs the batched kernels
// (capi_poseidon.hip, capi_verify.hip: the device; hostcheck.cpp: the same stream bodies on the host).
//
//   build   `batch` trees of one shape (arity, n, pairs).  Level v of all trees is ONE block of batch x lens[v] elements, tree b's level the slice at
//           b * lens[v]: level 0 is one copy (or one pair-leaf launch) through the pointer tables, every level above one DsBatchStream launch.
//           Trees of different lengths: merkle_build_mixed_batch, level v one block of the slices of the trees that still have it (DsRaggedStream).
//           The loop over the levels is merkle_climb / merkle_climb_ragged, which the batched FRI and sum-check commits run too.
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

// ---- the climb: level v of all trees hashed into level v + 1 until every tree has its root (merkle/src/lib.rs:163-179) ---------------------------------
// Written here once for every batched builder (merkle_build_batch / merkle_build_mixed_batch below, FriBatchCommit::commit_layer in fri_batch.hpp,
// ScBatch::commit_layers / commit_witnesses in sumcheck_batch.hpp).  The rules: level v - 1 is the DS level number of the launch that writes level v,
// positions start at 0, the last node of a level may be ragged, a tree of one leaf has its one level and no hash (the pair leaves, DS level 2^32 - 1,
// are a level 0 and so the caller's).  An executor X provides (pointers are its own memory: device pointers on the GPU, host pointers in the host check):
//   int32_t level_block(size_t n_fr, fr_t** out)                     the block of one level of all trees; it lives as long as the trees do
//   template <class DS> int32_t hash_level(const DS& D, fr_t* out)   one launch of hash_with_ds_dynamic over the hashes of D
//
// `B` trees of one shape: tree b's level 0 is in_ptrs[b][0 .. n) (a pointer table in X's memory) or in[b n .. (b + 1) n); labels_x: the per-tree
// labels in X's memory.  Level v >= 1 of all trees is ONE block of B x lens[v] elements written by ONE DsBatchStream launch, tree b's level the slice
// at base[v] + b lens[v]; base[0] = in (null behind a pointer table).  top: where the top level (the B roots) goes instead of a block of its own, or null.
template <class X>
inline int32_t merkle_climb(X& x, size_t arity, size_t B, const uint64_t* labels_x, const fr_t* const* in_ptrs, const fr_t* in, size_t n, fr_t* top,
                            std::vector<size_t>& lens, std::vector<fr_t*>& base) {
    lens = merkle_level_lens(n, arity); base.assign(lens.size(), nullptr); base[0] = const_cast<fr_t*>(in);
    for (size_t v = 1; v < lens.size(); ++v) {
        if (top && v + 1 == lens.size()) base[v] = top; else MB_TRY(x.level_block(B * lens[v], &base[v]));
        MB_TRY(x.hash_level(DsBatchStream::make(arity, (uint32_t)(v - 1), 0, labels_x, v == 1 ? in_ptrs : nullptr, v == 1 ? in : base[v - 1], lens[v - 1], B), base[v]));
    }
    return 0;
}

// Trees of different lengths, tree b of n[b] >= 1 leaves: level v of the call is ONE block, the slices of the trees that have more than v levels back
// to back in tree order (trees drop out as they reach their root), written by ONE DsRaggedStream launch over a segment table of those trees.
// The plan is everything about such a call that the lengths decide, as host data with no executor in it: lens[b] the level lengths of tree b,
// at[b][v] where its level v starts in the block of level v, block[v] that block's length, and every segment table of the call as ONE table: table v
// (n_seg[v] segments from segs[t0[v]], n_out[v] hashes) is the launch that writes level v, segment s of it tree tree[t0[v] + s] with its label, the
// length of its level v - 1 and `first`.  Table 0, only with leaf_table, is the launch that makes level 0 of every tree out of n[b] inputs
// each (the caller's: pair leaves or a copy).  in0 / in1 are left null: the climb points in0 of the tables v >= 1 at the blocks, table 0 is the caller's.
struct MerkleRaggedPlan {
    size_t arity = 0, depth = 0;
    std::vector<std::vector<size_t>> lens, at; std::vector<size_t> block;
    std::vector<DsRaggedStream::Seg> segs; std::vector<uint32_t> tree; std::vector<size_t> t0, n_seg, n_out;
};
inline MerkleRaggedPlan merkle_ragged_plan(size_t arity, size_t B, const size_t* n, const uint64_t* labels, bool leaf_table) {
    MerkleRaggedPlan P; P.arity = arity; P.lens.assign(B, {}); P.at.assign(B, {});
    for (size_t b = 0; b < B; ++b) { P.lens[b] = merkle_level_lens(n[b], arity); P.at[b].assign(P.lens[b].size(), 0); P.depth = std::max(P.depth, P.lens[b].size()); }
    P.block.assign(P.depth, 0); P.t0.assign(P.depth, 0); P.n_seg.assign(P.depth, 0); P.n_out.assign(P.depth, 0);
    for (size_t v = 0; v < P.depth; ++v) {
        P.t0[v] = P.segs.size();
        for (size_t b = 0; b < B; ++b) if (P.lens[b].size() > v) {
            P.at[b][v] = P.block[v]; P.block[v] += P.lens[b][v];
            if (!v && !leaf_table) continue;
            P.segs.push_back(DsRaggedStream::Seg{nullptr, nullptr, (uint64_t)(v ? P.lens[b][v - 1] : n[b]), labels[b], (uint64_t)P.n_out[v]}); P.tree.push_back((uint32_t)b);
            P.n_out[v] += P.lens[b][v];
        }
        P.n_seg[v] = P.segs.size() - P.t0[v];
    }
    return P;
}
// The climb over a plan.  level0[b]: where tree b's level 0 is (a host array of pointers in X's memory); top: where the top level goes instead of a
// block of its own, or null.  The blocks of the levels 1 .. depth - 1 are taken first, then the whole table goes up ONCE (x.segments), then
// level0_launch(table 0 in X's memory) runs what makes level 0 — it must return 0 without a launch where level 0 exists already — and then the levels,
// one launch each.  base[v]: the block of level v (base[0] stays null: level 0 is wherever the caller has it).  Besides level_block and hash_level, X provides
//   int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** x)   the table in X's memory; `h` may die on return
template <class X, class L0>
inline int32_t merkle_climb_ragged(X& x, MerkleRaggedPlan& P, const fr_t* const* level0, fr_t* top, std::vector<fr_t*>& base, L0 level0_launch) {
    base.assign(P.depth, nullptr);
    for (size_t v = 1; v < P.depth; ++v) { if (top && v + 1 == P.depth) base[v] = top; else MB_TRY(x.level_block(P.block[v], &base[v])); }
    for (size_t v = 1; v < P.depth; ++v) for (size_t s = P.t0[v]; s < P.t0[v] + P.n_seg[v]; ++s) {
        const size_t b = P.tree[s]; P.segs[s].in0 = v == 1 ? level0[b] : base[v - 1] + P.at[b][v - 1];
    }
    if (P.segs.empty()) return 0;
    const DsRaggedStream::Seg* sx = nullptr; MB_TRY(x.segments(P.segs, &sx));
    MB_TRY(level0_launch(sx));
    for (size_t v = 1; v < P.depth; ++v) MB_TRY(x.hash_level(DsRaggedStream::make(0, P.arity, (uint32_t)(v - 1), 0, sx + P.t0[v], P.n_seg[v], P.n_out[v]), base[v]));
    return 0;
}

// ---- build ------------------------------------------------------------------------------------------------------------------------------------
// `batch` trees of one shape.  Besides the climb's level_block and hash_level, an executor X provides:
//   int32_t tables(const uint64_t* labels, const fr_t* const* leaves, const fr_t* const* cp, size_t B,
//                  const uint64_t** labels_x, const fr_t* const** leaves_x, const fr_t* const** cp_x)
//                                                      the labels and pointer tables in X's memory (cp == nullptr: *cp_x = nullptr); the caller's arrays may die on return
//   int32_t copy_rows(const fr_t* const* src_x, size_t n, size_t B, fr_t* dst)          dst[b n + i] = src[b][i]
// lens[v] / base[v]: the length of level v and the block that holds it for all trees.  The argument checks are the caller's (merkle_build_on's).
template <class X>
inline int32_t merkle_build_batch(X& x, size_t arity, size_t B, const uint64_t* labels, const fr_t* const* leaves, size_t n, int pairs, const fr_t* const* cp,
                                  std::vector<size_t>& lens, std::vector<fr_t*>& base) {
    const uint64_t* labels_x = nullptr; const fr_t* const* leaves_x = nullptr; const fr_t* const* cp_x = nullptr;
    MB_TRY(x.tables(labels, leaves, pairs ? cp : nullptr, B, &labels_x, &leaves_x, &cp_x));
    fr_t* l0 = nullptr; MB_TRY(x.level_block(B * n, &l0));
    if (pairs) MB_TRY(x.hash_level(DsBatchPairPtrStream::make(arity, labels_x, leaves_x, cp_x, n, B), l0));          // new_pairs (:380-388, 392-414)
    else MB_TRY(x.copy_rows(leaves_x, n, B, l0));                                                                     // new: the leaves are level 0
    return merkle_climb(x, arity, B, labels_x, nullptr, l0, n, nullptr, lens, base);
}

// ---- build, trees of different lengths ------------------------------------------------------------------------------------------------------------
// `B` trees of one arity and parameter set, tree b of n[b] >= 1 leaves.  Level 0 is one ragged copy (or one ragged pair-leaf launch) over table 0 of
// the plan, which goes up with the climb's tables.  Besides the climb's three, an executor X provides:
//   int32_t copy_ragged(const DsRaggedStream& D, fr_t* dst)                                      dst[first_s + j] = in0_s[j] (D of mode 1)
// lens[b]: the level lengths of tree b; at[b][v]: where its level v starts in base[v].  The argument checks are the caller's.
template <class X>
inline int32_t merkle_build_mixed_batch(X& x, size_t arity, size_t B, const uint64_t* labels, const fr_t* const* leaves, const size_t* n, int pairs, const fr_t* const* cp,
                                        std::vector<std::vector<size_t>>& lens, std::vector<std::vector<size_t>>& at, std::vector<fr_t*>& base) {
    MerkleRaggedPlan P = merkle_ragged_plan(arity, B, n, labels, true);
    fr_t* l0 = nullptr; MB_TRY(x.level_block(P.block[0], &l0));
    std::vector<const fr_t*> level0(B);
    for (size_t b = 0; b < B; ++b) { P.segs[b].in0 = leaves[b]; P.segs[b].in1 = pairs ? cp[b] : nullptr; level0[b] = l0 + P.at[b][0]; }
    MB_TRY(merkle_climb_ragged(x, P, level0.data(), nullptr, base, [&](const DsRaggedStream::Seg* t0) {
        const DsRaggedStream L0 = DsRaggedStream::make(1, arity, 0xFFFFFFFFu, 0, t0, B, P.n_out[0]);
        return pairs ? x.hash_level(L0, l0)                                                                           // new_pairs (:380-388, 392-414)
                     : x.copy_ragged(L0, l0);                                                                         // new: the leaves are level 0
    }));
    base[0] = l0; lens = std::move(P.lens); at = std::move(P.at);
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
