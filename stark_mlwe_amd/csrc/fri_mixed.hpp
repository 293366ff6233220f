// stark_mlwe_amd/csrc/fri_mixed.hpp — the commit phase of deep_fri_prove (fri_build_transcript, crates/deep_ali/src/fri.rs:231-312) for a pass of
// Bp traces that share a SCHEDULE and nothing else: trace b has its own n0[b].  The ragged twin of fri_batch.hpp, over an executor that runs the
// kernels (capi_fri.hip: the device; hostcheck.cpp: the same bodies on the host).
//
// The layout.  Layer l of all traces is ONE buffer, the traces' slices back to back in trace order: trace b's slice starts at at[l][b], the prefix
// sum of n[.][l].  The traces share every fold arity m_l and every m_l divides every n[b][l], so
//       at[l + 1][b] * m_l == at[l][b]                                                                      (checked by shape())
// and the global partner rule of fri_batch.hpp — output j folds the inputs j m_l .. (j + 1) m_l, leaf i pairs with element i / m_l of the next
// buffer — holds on the concatenation whatever the lengths.  What differs from trace to trace:
//   * the fold challenge: z_l depends on (seed_z, l, n_l) (fri.rs:250).  One challenge and one z^t table per DISTINCT (l, n_l) of the pass (zkeys);
//     all tables come from one zpows_many.  A layer whose traces share n_l folds through the executor's plain fold; any other through fold_ragged,
//     whose segment table holds (first output, table offset) per run of traces with one n_l;
//   * the tree shapes: the leaf digests of a hashed arity are one leaf_pairs over the concatenation (the invariant again), the pair leaves of an
//     unhashed one a DsRaggedPairStream launch, and the levels merkle_climb_ragged over a MerkleRaggedPlan.  Trees finish at different levels, so a
//     tree's root is the top of its own level list and all (L + 1) Bp roots are fetched into `roots` (trace-major) by one gather;
//   * the Merkle arity, on the LAST layer only.  Below it the arity of a layer is a function of m_l alone when n0 is a power of two
//     (pick_arity_for_layer: n_l is a multiple of min(m_l, 128)); the last layer has arity 2 where n_L > 1 and arity 1 where n_L == 1.  Layer l's
//     trees are partitioned by arity (parts[l]); shape() refuses a layer below the last with more than one part.
// Layers 1..L are committed between fork() and side(false), underneath layer 0.  Nothing here synchronises the host.  Host-only C++ (no HIP).
#pragma once
#include <string>
#include <utility>
#include <vector>
#include "fr.hpp"
#include "host_util.hpp"
#include "poseidon_streams.hpp"
#include "fri_plan.hpp"
#include "merkle_batch.hpp"

namespace stark {

// The tables the ragged kernels read (fri_dev.hpp) and their host restatements.
// A run of fold outputs under one challenge: outputs [first_out, the next run's first_out) fold under zp[zp_off ..].  first_out ascends from 0.
struct FoldSeg { uint64_t first_out, zp_off; };
FR_HD size_t fold_seg_of(const FoldSeg* segs, size_t n_seg, uint64_t j) {            // the last run whose first output is <= j
    size_t lo = 0, hi = n_seg;
    while (hi - lo > 1) { const size_t mid = (lo + hi) >> 1; if (segs[mid].first_out <= j) lo = mid; else hi = mid; }
    return lo;
}
// One z^t table: zp[off + t] = z^t, t < m.
struct ZpowJob { fr_t z; uint64_t off, m; };
// out[j] = sum_t f[j m + t] zp[zp_off_seg(j) + t], j < n / m: what k_fri_fold_ragged computes, output by output.
inline void fri_fold_ragged_host(const fr_t* f, size_t n, const FoldSeg* segs, size_t n_seg, const fr_t* zp, size_t m, fr_t* out) {
    for (size_t j = 0; j < n / m; ++j) {
        const fr_t* t = zp + segs[fold_seg_of(segs, n_seg, j)].zp_off;
        fr_t acc = fr_zero<PallasFr>();
        for (size_t u = 0; u < m; ++u) acc = fr_add<PallasFr>(acc, fr_mul<PallasFr>(f[j * m + u], t[u]));
        out[j] = acc;
    }
}

#define FM_TRY(e) do { int32_t rc__ = (e); if (rc__) return rc__; } while (0)

// An executor X is an arena (alloc / upload / put) plus:
//   int32_t zpows_many(const ZpowJob* jobs, size_t n_jobs, size_t max_m, fr_t* zp)                         every table of the pass (jobs in X's memory)
//   int32_t fold(const fr_t* f, size_t n, const fr_t* zp, size_t m, fr_t* out)                              fri_fold_layer over n elements, one table
//   int32_t fold_ragged(const fr_t* f, size_t n, const FoldSeg* segs, size_t n_seg, const fr_t* zp, size_t m, fr_t* out)     the table per run
//   int32_t leaf_pairs(const fr_t* f, const fr_t* f_next, size_t n, size_t m, fr_t* h)                      hash_leaf_pair(f[i], f_next[i / m])
//   template <class DS> int32_t hash_level(size_t arity, const DS& D, fr_t* out)                            one launch over the hashes of D
//   int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** x)              a segment table in X's memory
//   int32_t gather(const MerkleGatherList& G, fr_t* out)                                                    out[row] = base[src][index], one launch
//   int32_t fork() / void side(bool on) / int32_t join()                                                    as in fri_batch.hpp
template <class X> struct FriMixedCommit {
    X& x; size_t Bp = 0, L = 0;
    std::vector<size_t> sched;
    std::vector<std::vector<size_t>> n, arity;                                  // n[b][l], arity[b][l]
    std::vector<std::vector<size_t>> at;                                        // at[l][b], b <= Bp: at[l][Bp] is the length of layer l's buffer
    struct ZKey { size_t l, n, zp_off; };
    std::vector<ZKey> zkeys; std::vector<std::vector<uint32_t>> zkey_of;        // the distinct (l, n_l), in order of first appearance; zkey_of[l][b]
    std::vector<fr_t> z; size_t zp_total = 0;                                   // z[k]: the challenge of zkeys[k]
    std::vector<fr_t*> f;                                                       // f[l]: the layer-l slices back to back
    // The trees of layer l that share an arity: traces[i] is the trace of tree i; level v of tree i is plan.lens[i][v] digests at
    // (v ? base[v] : leaves) + plan.at[i][v].
    struct Part { size_t arity = 0; std::vector<uint32_t> traces; MerkleRaggedPlan plan; fr_t* leaves = nullptr; std::vector<fr_t*> base; };
    std::vector<std::vector<Part>> parts;                                       // parts[l]
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> part_of;            // part_of[l][b] = (part, tree in it)
    fr_t* roots = nullptr;                                                      // Bp x (L + 1), trace-major
    explicit FriMixedCommit(X& x_) : x(x_) {}

    struct AtArity {
        FriMixedCommit& c; size_t arity;
        int32_t level_block(size_t k, fr_t** out) { return c.alloc_fr(k, out); }
        template <class DS> int32_t hash_level(const DS& D, fr_t* out) { return c.x.hash_level(arity, D, out); }
        int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** o) { return c.x.segments(h, o); }
    };
    int32_t alloc_fr(size_t k, fr_t** out) { void* p = nullptr; FM_TRY(x.alloc((k ? k : 1) * sizeof(fr_t), &p)); *out = (fr_t*)p; return 0; }
    // The shapes of a pass.  -1: an empty layer or a schedule that does not divide; -2: a layer with arity 1 and more than one leaf, or arities that
    // differ below the last layer; -3: the layout invariant does not hold (it always does once every m_l divides every n_l).
    int32_t shape(size_t Bp_, const size_t* n0, const size_t* schedule, size_t L_, std::string& err) {
        Bp = Bp_; L = L_; sched.assign(schedule, schedule + L);
        if (!Bp) { err = layer_shape_text(LayerShape::empty_layer); return -1; }
        n.assign(Bp, {}); arity.assign(Bp, {});
        for (size_t b = 0; b < Bp; ++b) {
            const LayerShape sh = fri_layers(n0[b], schedule, L, n[b], arity[b]);
            if (sh == LayerShape::arity_one) { err = "arity 1 with more than one leaf never terminates in the reference"; return -2; }
            if (sh != LayerShape::ok) { err = layer_shape_text(sh); return -1; }
        }
        at.assign(L + 1, std::vector<size_t>(Bp + 1, 0));
        for (size_t l = 0; l <= L; ++l) for (size_t b = 0; b < Bp; ++b) at[l][b + 1] = at[l][b] + n[b][l];
        for (size_t l = 0; l < L; ++l) for (size_t b = 0; b <= Bp; ++b) if (at[l + 1][b] * sched[l] != at[l][b]) { err = "ragged layout: at[l + 1][b] * m_l != at[l][b]"; return -3; }
        parts.assign(L + 1, {}); part_of.assign(L + 1, std::vector<std::pair<uint32_t, uint32_t>>(Bp));
        for (size_t l = 0; l <= L; ++l) {
            for (size_t b = 0; b < Bp; ++b) {
                size_t p = 0; while (p < parts[l].size() && parts[l][p].arity != arity[b][l]) ++p;
                if (p == parts[l].size()) { parts[l].emplace_back(); parts[l][p].arity = arity[b][l]; }
                part_of[l][b] = std::make_pair((uint32_t)p, (uint32_t)parts[l][p].traces.size()); parts[l][p].traces.push_back((uint32_t)b);
            }
            if (l < L && parts[l].size() > 1) { err = "the Merkle arities of a layer below the last differ between the traces"; return -2; }
        }
        zkeys.clear(); zkey_of.assign(L, std::vector<uint32_t>(Bp, 0)); zp_total = 0;
        for (size_t l = 0; l < L; ++l) for (size_t b = 0; b < Bp; ++b) {
            size_t k = 0; while (k < zkeys.size() && !(zkeys[k].l == l && zkeys[k].n == n[b][l])) ++k;
            if (k == zkeys.size()) { zkeys.push_back(ZKey{l, n[b][l], zp_total}); zp_total += sched[l]; }
            zkey_of[l][b] = (uint32_t)k;
        }
        return 0;
    }
    // After shape(): the layer buffers and the roots; z_[k] = fri_sample_z_ell(seed_z, zkeys[k].l, zkeys[k].n).  The caller then fills f[0] (trace b at
    // at[0][b]) and calls run().
    int32_t init(const fr_t* z_) {
        z.assign(z_, z_ + zkeys.size());
        f.assign(L + 1, nullptr);
        for (size_t l = 0; l <= L; ++l) FM_TRY(alloc_fr(at[l][Bp], &f[l]));
        return alloc_fr((L + 1) * Bp, &roots);
    }
    // The commitment of layer l of every trace, part by part: leaf digests, then the levels of every tree up to its own root.
    int32_t commit_layer(size_t l) {
        const size_t m = l < L ? sched[l] : 1;
        const fr_t* f_next = l < L ? f[l + 1] : nullptr;                                                        // zero partners on the last layer (fri.rs:266)
        for (Part& P : parts[l]) {
            const size_t k = P.traces.size(); const bool hashed = hashed_arity(P.arity);
            AtArity xa{*this, P.arity};
            std::vector<size_t> np(k); for (size_t i = 0; i < k; ++i) np[i] = n[P.traces[i]][l];
            const std::vector<uint64_t> labels(k, (uint64_t)l);
            P.plan = merkle_ragged_plan(P.arity, k, np.data(), labels.data(), !hashed);
            FM_TRY(xa.level_block(P.plan.block[0], &P.leaves));
            std::vector<const fr_t*> level0(k);
            for (size_t i = 0; i < k; ++i) { level0[i] = P.leaves + P.plan.at[i][0]; if (!hashed) P.plan.segs[i].in0 = f[l] + at[l][P.traces[i]]; }
            // a hashed part is the whole layer (shape()): its leaf digests are one launch over the concatenation, and so is in1 of the pair stream
            if (hashed) FM_TRY(x.leaf_pairs(f[l], f_next, at[l][Bp], m, P.leaves));
            FM_TRY(merkle_climb_ragged(xa, P.plan, level0.data(), nullptr, P.base, [&](const DsRaggedStream::Seg* t0) {
                return hashed ? 0 : xa.hash_level(DsRaggedPairStream::make(P.arity, t0, k, P.plan.n_out[0], f_next, m), P.leaves);
            }));
        }
        return 0;
    }
    int32_t run() {
        if (L) {
            fr_t* zp = nullptr; FM_TRY(alloc_fr(zp_total, &zp));
            std::vector<ZpowJob> jobs; size_t max_m = 0;
            for (size_t k = 0; k < zkeys.size(); ++k) { jobs.push_back(ZpowJob{z[k], (uint64_t)zkeys[k].zp_off, (uint64_t)sched[zkeys[k].l]}); max_m = std::max(max_m, sched[zkeys[k].l]); }
            std::vector<FoldSeg> segs; std::vector<size_t> s0(L + 1, 0);                                          // the runs of every ragged layer, one table
            for (size_t l = 0; l < L; ++l) {
                s0[l] = segs.size();
                for (size_t b = 0; b < Bp; ++b) if (!b || zkey_of[l][b] != zkey_of[l][b - 1]) segs.push_back(FoldSeg{(uint64_t)at[l + 1][b], (uint64_t)zkeys[zkey_of[l][b]].zp_off});
                if (segs.size() - s0[l] == 1) segs.resize(s0[l]);                                                 // one n_l: the plain fold, no lookup
            }
            s0[L] = segs.size();
            ZpowJob* jobs_x = nullptr; FoldSeg* segs_x = nullptr;
            FM_TRY(x.put(jobs, &jobs_x)); if (!segs.empty()) FM_TRY(x.put(segs, &segs_x));
            FM_TRY(x.zpows_many(jobs_x, jobs.size(), max_m, zp));
            for (size_t l = 0; l < L; ++l) {                                                                      // the folds back to back: no challenge depends on a commitment
                if (s0[l + 1] == s0[l]) FM_TRY(x.fold(f[l], at[l][Bp], zp + zkeys[zkey_of[l][0]].zp_off, sched[l], f[l + 1]));
                else FM_TRY(x.fold_ragged(f[l], at[l][Bp], segs_x + s0[l], s0[l + 1] - s0[l], zp, sched[l], f[l + 1]));
            }
        }
        FM_TRY(x.fork());
        x.side(true);
        int32_t rc = 0;
        for (size_t l = L; l >= 1 && !rc; --l) rc = commit_layer(l);
        x.side(false);
        if (!rc) rc = commit_layer(0);
        const int32_t jrc = x.join();
        if (rc || jrc) return rc ? rc : jrc;
        MerkleGatherList G;                                                                                       // every tree's root: the top of its own level list
        for (size_t b = 0; b < Bp; ++b) for (size_t l = 0; l <= L; ++l) { size_t len; G.add(level_at(b, l, levels(b, l) - 1, &len), 0, b * (L + 1) + l); }
        return x.gather(G, roots);
    }
    const fr_t* layer_at(size_t b, size_t l) const { return f[l] + at[l][b]; }
    size_t levels(size_t b, size_t l) const { const auto& q = part_of[l][b]; return parts[l][q.first].plan.lens[q.second].size(); }
    const fr_t* level_at(size_t b, size_t l, size_t v, size_t* len) const {
        const auto& q = part_of[l][b]; const Part& P = parts[l][q.first];
        *len = P.plan.lens[q.second][v];
        return (v ? P.base[v] : P.leaves) + P.plan.at[q.second][v];
    }
};
#undef FM_TRY

}  // namespace stark
