// stark_mlwe_amd/csrc/fri_verify_batch.hpp — deep_fri_verify over one proof or many, planned on the host (product code).  This is the
// only verifier there is: the single entry point plans a batch of one.
//
// The hashes a verification makes depend only on the indices and group sizes inside the proof, never on hash values, so the walks
// of fri_verify.hpp run once per proof over pool SLOTS instead of field elements and record every hash as a job.  The device then runs
// every opening of every proof that sits at the same dependency depth in one launch per Poseidon width (capi_verify.hip), and one
// thread per proof compares its computed roots with the claimed ones.  Everything that compares values inside the proof only
// (s_i == f_parent[b], final_index, the n0 / schedule checks) stays in the walk on the host and ends in the per-proof flag.
//
// The plan, after finish():
//   pool     [ inputs: siblings, pair-leaf children, claimed roots | leaf f (nl) | leaf s (nl) | computed digests ]
//   leaf     pool[leaf_out0 + j] = hash_leaf_pair(pool[leaf_f0 + j], pool[leaf_f0 + nl + j])                              depth 1
//   groups   DS jobs of one (width, depth), in depth order: job k of group G writes pool[G.out0 + k - G.job0]; its header is
//            hdr[4k .. 4k+3] = (arity, level, position, label) and its children pool[idx[off[k]] .. idx[off[k+1] - 1]]   (DsGatherStream)
//   checks   proof b is accepted iff flag[b] and pool[chk[2j]] == pool[chk[2j+1]] for every j in [chk_off[b], chk_off[b+1])
// Inputs are depth 0; a computed digest is one deeper than its deepest child.  A proof that fails a check in the walk keeps no job.
// Host-only C++.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "fri_verify.hpp"

namespace stark {

struct VerifyBatchPlan {
    struct Group { int t; uint32_t depth; size_t job0, n, max_children, out0; };
    size_t batch = 0, n_known = 0;                 // n_known: the pool prefix the host fills (inputs and leaf f / s); the rest is computed
    std::vector<fr_t> pool;
    size_t nl = 0, leaf_f0 = 0, leaf_out0 = 0;
    std::vector<uint64_t> hdr; std::vector<uint32_t> off, idx;
    std::vector<Group> groups;
    std::vector<uint32_t> chk_off, chk; std::vector<int32_t> flag;
};

// The job, depth and group machinery of a batch plan, shared by the planners that walk openings over pool slots (the DEEP-FRI one below,
// the sum-check one of sumcheck_verify_batch.hpp).  Slots while planning: an input is its pool index, a computed digest is kComputed | its
// number.  A planner hands out input slots with new_input() (what the pool holds there is its own business), records DS hashes with
// ds_job() and root comparisons with many() / pairs_rooted(), closes each item with end_item() and lays the jobs out with finish_jobs().
class DsJobPlanner {
public:
    static constexpr uint32_t kComputed = 0x80000000u;
protected:
    struct Job { int t; uint32_t depth; uint64_t hdr[4]; size_t ch0, nch; uint32_t out; };
    struct JobMark { size_t in, jobs, ch, comp, chk; };
    size_t n_in_ = 0;                                                                    // input slots handed out so far
    std::vector<Job> jobs_; std::vector<uint32_t> ch_; std::vector<uint32_t> depth_;     // depth_[c]: depth of computed digest c
    size_t n_comp_ = 0;
    std::vector<uint32_t> chk_, chk_off_{0}; std::vector<int32_t> flag_;                 // item b: its host flag, its checks chk_[2 chk_off_[b] .. 2 chk_off_[b + 1])

    JobMark job_mark() const { return JobMark{n_in_, jobs_.size(), ch_.size(), n_comp_, chk_.size()}; }
    void job_rollback(const JobMark& m) { n_in_ = m.in; jobs_.resize(m.jobs); ch_.resize(m.ch); n_comp_ = m.comp; depth_.resize(m.comp); chk_.resize(m.chk); }
    void end_item(bool ok) { flag_.push_back(ok ? 1 : 0); chk_off_.push_back((uint32_t)(chk_.size() / 2)); }      // after the rollback of a rejected item: an empty range
    uint32_t new_input() { return (uint32_t)(n_in_++); }
    uint32_t depth_of(uint32_t s) const { return s & kComputed ? depth_[s & ~kComputed] : 0; }
    uint32_t computed(uint32_t depth) { depth_.push_back(depth); return kComputed | (uint32_t)(n_comp_++); }
    uint32_t ds_job(size_t arity, uint32_t level, uint64_t position, uint64_t label, const std::vector<uint32_t>& kids) {
        Job j; j.t = host::width_for_arity(arity); j.hdr[0] = arity; j.hdr[1] = level; j.hdr[2] = position; j.hdr[3] = label;
        j.ch0 = ch_.size(); j.nch = kids.size(); uint32_t d = 0;
        for (uint32_t k : kids) { ch_.push_back(k); d = std::max(d, depth_of(k)); }
        j.depth = d + 1; j.out = computed(j.depth); jobs_.push_back(j); return j.out;
    }
    // verify_many_ds over slots: the level walk records each group as a job; a good walk leaves one root comparison against `root`.
    //   sib(level, j) -> slot of the j-th sibling of `level`
    template <class Proof, class Sib>
    bool many(size_t cfg_arity, uint32_t root, const std::vector<size_t>& ix, const std::vector<uint32_t>& vals, const Proof& pr, uint64_t label, Sib sib) {
        auto hash_level = [&](uint32_t level, size_t arity, const std::vector<size_t>& parents, const std::vector<std::vector<uint32_t>>& kids, std::vector<uint32_t>& nv) -> int32_t {
            for (size_t g = 0; g < parents.size(); ++g) nv[g] = ds_job(arity, level, (uint64_t)parents[g], label, kids[g]);
            return 0;
        };
        bool shaped = false; uint32_t top = 0;
        ds_walk(cfg_arity, ix, vals, pr, sib, hash_level, shaped, top);
        if (!shaped) return false;
        chk_.push_back(top); chk_.push_back(root); return true;
    }
    // many() against a claimed root that is an input of the plan: root_slot() hands out its slot after the walk's siblings, and only for a walk that is shaped
    template <class Proof, class Sib, class Root>
    bool many_rooted(size_t cfg_arity, const std::vector<size_t>& ix, const std::vector<uint32_t>& vals, const Proof& pr, uint64_t label, Sib sib, Root root_slot) {
        const size_t before = chk_.size();
        if (!many(cfg_arity, 0u, ix, vals, pr, label, sib)) return false;
        chk_[before + 1] = root_slot(); return true;
    }
    // verify_pairs_ds over slots (merkle/src/lib.rs:723-773): one two-child job at level 2^32 - 1 per distinct index over (f, cp), then many_rooted over those leaves
    template <class Sib, class Root>
    bool pairs_rooted(size_t cfg_arity, const std::vector<size_t>& ix, const std::vector<uint32_t>& f, const std::vector<uint32_t>& cp, const MerkleProofHost& pr, uint64_t label, Sib sib,
                      Root root_slot) {
        std::vector<size_t> req; std::vector<uint32_t> cf, cc, v;
        if (!pairs_leaf_set(cfg_arity, ix, f, cp, pr, req, cf, cc)) return false;
        for (size_t k = 0; k < req.size(); ++k) v.push_back(ds_job(pr.arity, 0xFFFFFFFFu, (uint64_t)req[k], label, {cf[k], cc[k]}));
        return many_rooted(cfg_arity, req, v, pr, label, sib, root_slot);
    }
    // the items of a plan whose checks are all root comparisons (the DEEP-FRI and Merkle planners; the sum-check plan keeps its own flags and turns
    // its comparisons into records)
    void finish_items(VerifyBatchPlan& o) const { o.batch = flag_.size(); o.flag = flag_; o.chk_off = chk_off_; }
    // Lays the jobs out in launch order — by depth, then width; each group's digests contiguous from pool slot `next` on — and fills the
    // plan's groups, hdr, off, idx and chk.  pos: computed digest -> pool slot, preset by the caller for what it computes itself (leaf
    // digests).  Returns the pool size.
    size_t finish_jobs(VerifyBatchPlan& o, std::vector<uint32_t>& pos, size_t next) const {
        std::vector<size_t> order(jobs_.size()); for (size_t k = 0; k < order.size(); ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return jobs_[a].depth != jobs_[b].depth ? jobs_[a].depth < jobs_[b].depth : jobs_[a].t < jobs_[b].t; });
        for (size_t k = 0; k < order.size(); ++k) {
            const Job& J = jobs_[order[k]];
            if (o.groups.empty() || o.groups.back().depth != J.depth || o.groups.back().t != J.t) o.groups.push_back(VerifyBatchPlan::Group{J.t, J.depth, k, 0, 0, next});
            VerifyBatchPlan::Group& G = o.groups.back(); ++G.n; G.max_children = std::max(G.max_children, J.nch);
            pos[J.out & ~kComputed] = (uint32_t)next++;
        }
        auto slot = [&](uint32_t s) { return s & kComputed ? pos[s & ~kComputed] : s; };
        o.hdr.reserve(4 * order.size()); o.off.reserve(order.size() + 1); o.idx.reserve(ch_.size());
        o.off.push_back(0);
        for (size_t k : order) {
            const Job& J = jobs_[k];
            o.hdr.insert(o.hdr.end(), J.hdr, J.hdr + 4);
            for (size_t c = 0; c < J.nch; ++c) o.idx.push_back(slot(ch_[J.ch0 + c]));
            o.off.push_back((uint32_t)o.idx.size());
        }
        o.chk.resize(chk_.size()); for (size_t j = 0; j < chk_.size(); ++j) o.chk[j] = slot(chk_[j]);
        return next;
    }
};

// Builds the VerifyBatchPlan of deep_fri_verify one proof at a time.  Every input slot holds a field element of the proof (pool_).
class VerifyBatchPlanner : public DsJobPlanner {
public:
    // plans deep_fri_verify of one proof; a proof that does not decode or fails a check in the walk is planned as a rejection
    void add(const uint8_t* bytes, size_t len, const size_t* schedule, size_t L, size_t r) {
        const Mark m = mark();
        DeepFriProofHost P; bool ok = false;
        if (decode_proof(bytes, len, P)) deep_fri_walk(P, schedule, L, r, [&](size_t layer, size_t ar, bool hashed, const std::vector<size_t>& ix, const std::vector<fr_t>& ff,
                                                                              const std::vector<fr_t>& ss, const MerkleProofHost& pr, bool& good) -> int32_t {
            good = open(P, layer, ar, hashed, ix, ff, ss, pr); return 0;
        }, ok);
        if (!ok) rollback(m);
        end_item(ok);
    }
    size_t proofs() const { return flag_.size(); }
    size_t slots() const { return pool_.size() + 2 * leaf_f_.size() + n_comp_; }      // the pool the plan needs so far
    bool fits_u32() const { return slots() < kComputed && ch_.size() < kComputed; }
    void finish(VerifyBatchPlan& out);
private:
    struct Mark { JobMark j; size_t leaf; };
    std::vector<fr_t> pool_, leaf_f_, leaf_s_; std::vector<uint32_t> leaf_out_;

    Mark mark() const { return Mark{job_mark(), leaf_f_.size()}; }
    void rollback(const Mark& m) { job_rollback(m.j); pool_.resize(m.j.in); leaf_f_.resize(m.leaf); leaf_s_.resize(m.leaf); leaf_out_.resize(m.leaf); }
    uint32_t input(const fr_t& x) { pool_.push_back(x); return new_input(); }
    uint32_t leaf(const fr_t& f, const fr_t& s) { leaf_f_.push_back(f); leaf_s_.push_back(s); leaf_out_.push_back(computed(1)); return leaf_out_.back(); }
    bool open(const DeepFriProofHost& P, size_t layer, size_t ar, bool hashed, const std::vector<size_t>& ix, const std::vector<fr_t>& ff, const std::vector<fr_t>& ss,
              const MerkleProofHost& pr) {
        auto sib = [&](size_t level, size_t j) { return input(pr.siblings[level][j]); };
        auto root = [&]() { return input(P.roots[layer]); };
        if (hashed) {                                                    // verify_single over hash_leaf_pair(f, s)
            std::vector<uint32_t> v; for (size_t k = 0; k < ix.size(); ++k) v.push_back(leaf(ff[k], ss[k]));
            return many_rooted(ar, ix, v, pr, (uint64_t)layer, sib, root);
        }
        std::vector<uint32_t> f, s;                                      // verify_pairs over (f, s)
        for (size_t k = 0; k < ix.size(); ++k) { f.push_back(input(ff[k])); s.push_back(input(ss[k])); }
        return pairs_rooted(ar, ix, f, s, pr, (uint64_t)layer, sib, root);
    }
};

inline void VerifyBatchPlanner::finish(VerifyBatchPlan& out) {
    VerifyBatchPlan& o = out; o = VerifyBatchPlan();
    finish_items(o);
    const size_t ni = pool_.size(), nl = leaf_f_.size();
    o.nl = nl; o.leaf_f0 = ni; o.leaf_out0 = ni + 2 * nl; o.n_known = ni + 2 * nl;
    std::vector<uint32_t> pos(n_comp_);                                 // computed digest -> pool slot: the leaf digests, then each group's
    for (size_t j = 0; j < nl; ++j) pos[leaf_out_[j] & ~kComputed] = (uint32_t)(o.leaf_out0 + j);
    const size_t total = finish_jobs(o, pos, o.leaf_out0 + nl);
    o.pool.assign(total, fr_zero<PallasFr>());
    std::copy(pool_.begin(), pool_.end(), o.pool.begin());
    std::copy(leaf_f_.begin(), leaf_f_.end(), o.pool.begin() + ni); std::copy(leaf_s_.begin(), leaf_s_.end(), o.pool.begin() + ni + nl);
}

}  // namespace stark
