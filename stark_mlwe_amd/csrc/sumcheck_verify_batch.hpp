// stark_mlwe_amd/csrc/sumcheck_verify_batch.hpp — verify_plain / verify_mf (crates/channel/src/lib.rs:1080-1128, :1176-1240) over a batch of
// proofs, planned on the host and decided on the device (capi_sumcheck.hip: the device; hostcheck.cpp: the same bodies on the host).
//
// Everything a sum-check verifier hashes or absorbs is data inside the proof: verify_mf draws r_i from prev_root, which it reads and never
// computes, and checks each opening against a root the proof claims; verify_plain's transcript absorbs only the proof's coefficients.  So
// the planner parses the bincode layout of ProofPlain / ProofMF (length guards that a forged prefix cannot pass, the == 32 FBytes prefix, the
// Option tag byte of ProofPlain, no trailing bytes) but converts NO field element: it records where each one sits in the uploaded bytes and
// which pool slot it lands in, and the device decodes them (sc_decode_fr: range check and Montgomery conversion, one lane each).
//
// The plan, after finish():
//   blob     the bytes of the proofs that parsed, each from a 16-byte boundary, as little-endian dwords (two dwords of padding at the end)
//   decode   entry j fills pool[j]: the element at byte dec_off[j] of the blob, owned by proof dec_proof[j] (a value >= r clears that
//            proof's flag); with kClaim set in dec_proof[j] the entry is the claim 2 c0 + c1 of the two elements at dec_off[j], + 40
//   pool     [ decoded (n_dec) | challenges (n_seg) | computed digests ]; the transcripts' constants are a pool of their own (consts)
//   tr       transcript streams (TrBatchStream): stream g runs instances [inst0, inst0 + n) of nseg segments each from Transcript::new;
//            segment s (counted over all streams) absorbs tr_idx[tr_off[s] .. tr_off[s + 1]) and leaves its challenge in pool[n_dec + s]
//            plain: one instance per proof, one segment per round, streams by round count; mf: one one-segment instance per round
//   ds       the DS groups of every opening (VerifyBatchPlan: groups, hdr, off, idx), MerkleCommitment's parameters, in depth order
//   rec      8 words per check; a failed check clears flag[proof]
//            plain, one per (proof, round i):  { proof, c0_i, c1_i, c0_{i-1}, c1_{i-1}, r_{i-1}, final, r_i }   (kNone where absent)
//                   i >= 1: 2 c0_i + c1_i == c0_{i-1} + c1_{i-1} r_{i-1};   last round: final == c0_i + c1_i r_i
//            mf, one per relation:             { kind, proof, a, b, c, d, e, 0 }
//                   kChain 2 a + b == c + d e | kFinal a == c + d e | kFold a + e (b - a) == c | kEq a == b (a computed root, the claimed one)
// accepted[b] = flag[b] after the checks.  A proof that does not parse or fails a host check keeps nothing in the plan and has flag 0.
// Host-only C++ but for the FR_HD bodies, which the kernels of capi_sumcheck.hip run.  Included by sumcheck_impl.hpp after sumcheck_batch.hpp.
#pragma once
#include <map>
#include "fri_verify_batch.hpp"

namespace stark {

constexpr uint32_t kScNone = 0xFFFFFFFFu, kScClaim = 0x80000000u;
enum ScCheckKind : uint32_t { kScChain = 0, kScFinal = 1, kScFold = 2, kScEq = 3 };

// ---- the bodies the kernels run (and hostcheck.cpp, on the host) ------------------------------------------------------------------
// The 32 canonical little-endian bytes at byte offset `off` of `words` (a buffer of little-endian dwords with one readable dword past the
// element): the nine covering aligned dwords, funnel-shifted into eight limbs.  false: the value is >= r (not a field element).
FR_HD bool sc_load_canonical(const uint32_t* __restrict__ words, uint64_t off, fr_t& t) {
    const uint32_t* w = words + (off >> 2); const uint32_t sh = 8u * (uint32_t)(off & 3);
    uint32_t d[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = w[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
        t.v[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], sh);                   // ({d[i+1], d[i]} >> sh) & 0xffffffff; sh = 0 gives d[i]
#else
        t.v[i] = sh ? (d[i] >> sh) | (d[i + 1] << (32 - sh)) : d[i];
#endif
    }
    return !fr_geq_p<PF>(t.v);
}
// decode entry j of a plan: pool[j] in the stored Montgomery form (one product by R^2); false clears the owning proof's flag
FR_HD bool sc_decode_fr(const uint32_t* __restrict__ words, uint32_t off, uint32_t owner, fr_t& out) {
    fr_t a; bool ok = sc_load_canonical(words, off, a);
    a = fr_from_canonical<PF>(a);
    if (owner & kScClaim) {                                                       // 2 c0 + c1 of round 0 (send_claim): c1's bytes follow c0's and its length prefix
        fr_t b; ok = sc_load_canonical(words, (uint64_t)off + 40, b) && ok;
        a = fr_add<PF>(fr_add<PF>(a, a), fr_from_canonical<PF>(b));
    }
    out = a; return ok;
}
FR_HD bool sc_rel_lin(const fr_t& lhs, const fr_t& c, const fr_t& d, const fr_t& e) { return fr_eq(lhs, fr_add<PF>(c, fr_mul<PF>(d, e))); }
// one (proof, round) record of verify_plain
FR_HD bool sc_check_plain(const fr_t* __restrict__ pool, const uint32_t* __restrict__ rec) {
    const fr_t c0 = ldg(pool + rec[1]), c1 = ldg(pool + rec[2]); bool ok = true;
    if (rec[3] != kScNone) ok = sc_rel_lin(fr_add<PF>(fr_add<PF>(c0, c0), c1), ldg(pool + rec[3]), ldg(pool + rec[4]), ldg(pool + rec[5]));
    if (rec[6] != kScNone) ok = sc_rel_lin(ldg(pool + rec[6]), c0, c1, ldg(pool + rec[7])) && ok;
    return ok;
}
// one relation record of verify_mf
FR_HD bool sc_check_mf(const fr_t* __restrict__ pool, const uint32_t* __restrict__ rec) {
    const fr_t a = ldg(pool + rec[2]);
    switch (rec[0]) {
    case kScChain: { const fr_t b = ldg(pool + rec[3]); return sc_rel_lin(fr_add<PF>(fr_add<PF>(a, a), b), ldg(pool + rec[4]), ldg(pool + rec[5]), ldg(pool + rec[6])); }
    case kScFinal: return sc_rel_lin(a, ldg(pool + rec[4]), ldg(pool + rec[5]), ldg(pool + rec[6]));
    case kScFold:  { const fr_t b = ldg(pool + rec[3]); return fr_eq(fr_add<PF>(a, fr_mul<PF>(ldg(pool + rec[6]), fr_sub<PF>(b, a))), ldg(pool + rec[4])); }
    default:       return fr_eq(a, ldg(pool + rec[3]));
    }
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
struct ScVerifyPlan {
    struct Stream { size_t inst0, n, nseg, seg0; };          // seg0: its first segment, counted over all streams
    int mf = 0; size_t batch = 0;
    std::vector<int32_t> flag;
    std::vector<uint32_t> blob, dec_off, dec_proof;
    size_t n_dec = 0, n_seg = 0, n_inst = 0, pool_slots = 0;
    std::vector<fr_t> consts;
    std::vector<Stream> tr; std::vector<uint32_t> tr_off, tr_idx;
    VerifyBatchPlan ds;
    std::vector<uint32_t> rec;
    size_t n_rec() const { return rec.size() / 8; }
    // the device steps of the plan as (kind, count) rows: 0 decode (elements), 1 a transcript stream (instances), 2 a DS group (hashes), 3 the checks
    std::vector<std::pair<int, size_t>> steps() const {
        std::vector<std::pair<int, size_t>> s;
        if (n_dec) s.push_back({0, n_dec});
        for (const Stream& t : tr) s.push_back({1, t.n});
        for (const VerifyBatchPlan::Group& g : ds.groups) s.push_back({2, g.n});
        if (n_rec()) s.push_back({3, n_rec()});
        return s;
    }
};

class ScVerifyPlanner : public DsJobPlanner {
public:
    explicit ScVerifyPlanner(int mf) : mf_(mf), C_(0u, TrBatchStream::kPool1) {}
    // plans verify_plain (the label is not read) / verify_mf of one proof
    void add(const uint8_t* bytes, size_t len, uint64_t label) {
        const Mark m = mark();
        proof_ = (uint32_t)flag_.size(); base_ = blob_.size() * 4;
        const bool ok = mf_ ? add_mf(bytes, len, label) : add_plain(bytes, len);
        if (ok) { blob_.resize((base_ + len + 15) / 16 * 4, 0u); if (len) memcpy((uint8_t*)blob_.data() + base_, bytes, len); }
        else rollback(m);
        end_item(ok);
    }
    size_t proofs() const { return flag_.size(); }
    size_t slots() const { return n_in_ + seg_end_.size() + n_comp_; }               // the pool the plan needs so far
    bool fits_u32() const { return slots() < kRSlot && ch_.size() < kComputed && tidx_.size() < kComputed && (blob_.size() + 16) * 4 < ((uint64_t)1 << 32); }
    void finish(ScVerifyPlan& out);
private:
    static constexpr uint32_t kRSlot = 0x40000000u;           // while planning: kRSlot | segment number (in planning order)
    struct SibLevel { uint32_t slot0; size_t n; size_t size() const { return n; } };
    struct SlotProof { std::vector<size_t> indices; std::vector<SibLevel> siblings; std::vector<std::vector<uint8_t>> group_sizes; size_t arity = 0; };
    struct RoundMF { uint32_t c0, c1, next_root; std::vector<size_t> cur_indices, next_indices; std::vector<uint32_t> cur_values, next_values; SlotProof cur_proof, next_proof; };
    struct Inst { size_t seg0, nseg; };                       // a transcript instance: its segments [seg0, seg0 + nseg) in planning order
    struct Mark { JobMark j; size_t dec, inst, seg, tidx, rec; };
    int mf_; uint32_t proof_ = 0; size_t base_ = 0;
    ScConsts C_;
    std::vector<uint32_t> blob_, dec_off_, dec_proof_;
    std::vector<Inst> inst_; std::vector<uint32_t> seg_end_, tidx_;      // seg_end_[s]: end of segment s in tidx_
    std::vector<uint32_t> rec_;

    Mark mark() const { return Mark{job_mark(), dec_off_.size(), inst_.size(), seg_end_.size(), tidx_.size(), rec_.size()}; }
    void rollback(const Mark& m) { job_rollback(m.j); dec_off_.resize(m.dec); dec_proof_.resize(m.dec); inst_.resize(m.inst); seg_end_.resize(m.seg); tidx_.resize(m.tidx); rec_.resize(m.rec); }
    uint32_t decode_at(size_t pos, uint32_t tag) { dec_off_.push_back((uint32_t)(base_ + pos)); dec_proof_.push_back(proof_ | tag); return new_input(); }
    void record(std::initializer_list<uint32_t> w) { rec_.insert(rec_.end(), w.begin(), w.end()); }
    uint32_t end_segment() { seg_end_.push_back((uint32_t)tidx_.size()); return kRSlot | (uint32_t)(seg_end_.size() - 1); }

    // the bincode reader over slots: an FBytes is its length prefix (== 32) and 32 bytes that stay where they are
    struct Rd {
        ScVerifyPlanner& P; ByteReader R; Rd(ScVerifyPlanner& p, const uint8_t* b, size_t n) : P(p), R(b, n) {}
        uint32_t fb() { if (R.u64() != 32) R.ok = false; if (!R.ok || R.left() < 32) { R.ok = false; return 0; } const uint32_t s = P.decode_at(R.pos, 0u); R.pos += 32; return s; }
        bool idxs(std::vector<size_t>& v) { size_t k = R.len(8); v.resize(k); for (size_t i = 0; i < k; ++i) v[i] = (size_t)R.u64(); return R.ok; }
        bool fvec(std::vector<uint32_t>& v) { size_t k = R.len(40); v.resize(k); for (size_t i = 0; i < k && R.ok; ++i) v[i] = fb(); return R.ok; }
        bool mproof(SlotProof& p) {
            p.arity = (size_t)R.u64();
            size_t g = R.len(8); p.group_sizes.assign(g, {}); for (size_t i = 0; i < g && R.ok; ++i) { size_t k = R.len(1); p.group_sizes[i].resize(k); for (size_t j = 0; j < k; ++j) p.group_sizes[i][j] = R.u8(); }
            if (!idxs(p.indices)) return false;
            size_t a = R.len(8); p.siblings.assign(a, SibLevel{0, 0});
            for (size_t i = 0; i < a && R.ok; ++i) { std::vector<uint32_t> l; fvec(l); p.siblings[i] = SibLevel{l.empty() ? 0u : l[0], l.size()}; }   // consecutive decode entries: consecutive slots
            return R.ok;
        }
    };

    bool add_plain(const uint8_t* bytes, size_t len) {                                          // verify_plain (:1080-1128): a failed check answers `false` (in the reference a failed assert_eq!, a panic)
        Rd D(*this, bytes, len); const uint32_t root = D.fb(); const size_t nr = D.R.len(80);
        std::vector<std::pair<uint32_t, uint32_t>> rounds(nr); size_t c0_pos = 0;
        for (size_t i = 0; i < nr && D.R.ok; ++i) { if (i == 0) c0_pos = D.R.pos + 8; rounds[i].first = D.fb(); rounds[i].second = D.fb(); }
        if (D.R.u8() != 0) D.R.ok = false;
        const uint32_t fin = D.fb();
        if (!D.R.ok || D.R.left()) return false;
        if (rounds.empty()) return false;                                                        // :1100-1102
        const uint32_t claim = decode_at(c0_pos, kScClaim);                                      // running_0 = 2 c0_0 + c1_0
        ScSeg S{C_, tidx_}; inst_.push_back(Inst{seg_end_.size(), nr});
        S.str(sc_lab::plain); S.digest(sc_lab::root, root); S.str(sc_lab::claim); S.slot(claim);
        uint32_t r_prev = kScNone;
        for (size_t i = 0; i < nr; ++i) {
            S.str(sc_lab::round); S.u64(i); S.str(sc_lab::c0); S.slot(rounds[i].first); S.str(sc_lab::c1); S.slot(rounds[i].second);
            S.challenge(lab_idx(sc_lab::r, i));
            const uint32_t r = end_segment(); const bool last = i + 1 == nr;
            record({proof_, rounds[i].first, rounds[i].second, i ? rounds[i - 1].first : kScNone, i ? rounds[i - 1].second : kScNone, i ? r_prev : kScNone, last ? fin : kScNone, r});
            r_prev = r;
        }
        return true;
    }
    bool add_mf(const uint8_t* bytes, size_t len, uint64_t label) {                              // verify_mf (:1176-1240)
        Rd D(*this, bytes, len); const uint32_t initial_root = D.fb(); const size_t nr = D.R.len(120);
        std::vector<RoundMF> rounds(nr);
        for (size_t i = 0; i < nr && D.R.ok; ++i) { RoundMF& R = rounds[i]; R.c0 = D.fb(); R.c1 = D.fb(); R.next_root = D.fb(); D.idxs(R.cur_indices); D.fvec(R.cur_values); D.mproof(R.cur_proof); D.idxs(R.next_indices); D.fvec(R.next_values); D.mproof(R.next_proof); }
        const uint32_t fin = D.fb();
        if (!D.R.ok || D.R.left()) return false;
        uint32_t prev_root = initial_root, r_prev = kScNone;
        const std::vector<uint8_t> r_i(sc_lab::r_i, sc_lab::r_i + strlen(sc_lab::r_i));
        for (size_t i = 0; i < nr; ++i) {
            const RoundMF& R = rounds[i];
            if (i) record({kScChain, proof_, R.c0, R.c1, rounds[i - 1].c0, rounds[i - 1].c1, r_prev, 0u});                           // start_round (:803-804)
            ScSeg S{C_, tidx_}; inst_.push_back(Inst{seg_end_.size(), 1});                                                        // mf_round_challenge_from_root (:592-598)
            S.str(sc_lab::mf_round_chal); S.str(sc_lab::mf_r); S.u64(i); S.slot(prev_root); S.challenge(r_i);
            const uint32_t r = end_segment();
            auto sib_of = [](const SlotProof& p) { return [&p](size_t level, size_t j) { return p.siblings[level].slot0 + (uint32_t)j; }; };
            if (!many(16, prev_root, R.cur_indices, R.cur_values, R.cur_proof, label, sib_of(R.cur_proof))) return false;           // verify_fold_openings (:821-869)
            if (!many(16, R.next_root, R.next_indices, R.next_values, R.next_proof, label, sib_of(R.next_proof))) return false;
            if (R.cur_indices.size() != R.cur_values.size() || R.next_indices.size() != R.next_values.size()) return false;
            std::map<size_t, std::pair<std::pair<bool, uint32_t>, std::pair<bool, uint32_t>>> pairs;
            for (size_t t = 0; t < R.cur_indices.size(); ++t) { const size_t ix = R.cur_indices[t]; auto& e = pairs[ix / 2]; if (ix % 2 == 0) e.first = {true, R.cur_values[t]}; else e.second = {true, R.cur_values[t]}; }
            for (size_t t = 0; t < R.next_indices.size(); ++t) {
                auto it = pairs.find(R.next_indices[t]);
                if (it == pairs.end() || !it->second.first.first || !it->second.second.first) return false;
                record({kScFold, proof_, it->second.first.second, it->second.second.second, R.next_values[t], 0u, r, 0u});
            }
            r_prev = r; prev_root = R.next_root;
        }
        if (nr) record({kScFinal, proof_, fin, 0u, rounds[nr - 1].c0, rounds[nr - 1].c1, r_prev, 0u});                              // :1237-1238 (no rounds: accepted)
        return true;
    }
};

inline void ScVerifyPlanner::finish(ScVerifyPlan& out) {
    ScVerifyPlan& o = out; o = ScVerifyPlan();
    o.mf = mf_; o.batch = flag_.size(); o.flag = flag_;
    o.blob = blob_; o.blob.resize(blob_.size() + 2, 0u);
    o.dec_off = dec_off_; o.dec_proof = dec_proof_; o.n_dec = dec_off_.size();
    o.consts = C_.v; o.n_inst = inst_.size(); o.n_seg = seg_end_.size();
    // streams: the instances by segment count (verify_mf: one stream of one-segment instances), their segments renumbered in that order
    std::vector<size_t> order(inst_.size()); for (size_t a = 0; a < order.size(); ++a) order[a] = a;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return inst_[a].nseg < inst_[b].nseg; });
    std::vector<uint32_t> seg_new(seg_end_.size());
    o.tr_off.reserve(seg_end_.size() + 1); o.tr_idx.reserve(tidx_.size()); o.tr_off.push_back(0);
    for (size_t a = 0; a < order.size(); ++a) {
        const Inst& I = inst_[order[a]];
        if (o.tr.empty() || o.tr.back().nseg != I.nseg) o.tr.push_back(ScVerifyPlan::Stream{a, 0, I.nseg, o.tr_off.size() - 1});
        ++o.tr.back().n;
        for (size_t s = I.seg0; s < I.seg0 + I.nseg; ++s) {
            seg_new[s] = (uint32_t)(o.tr_off.size() - 1);
            o.tr_idx.insert(o.tr_idx.end(), tidx_.begin() + (s ? seg_end_[s - 1] : 0), tidx_.begin() + seg_end_[s]);
            o.tr_off.push_back((uint32_t)o.tr_idx.size());
        }
    }
    std::vector<uint32_t> pos(n_comp_);
    o.pool_slots = finish_jobs(o.ds, pos, o.n_dec + o.n_seg);
    auto slot = [&](uint32_t s) { return s == kScNone ? s : (s & kRSlot ? (uint32_t)(o.n_dec + seg_new[s & ~kRSlot]) : s); };
    o.rec = rec_;
    for (size_t j = 0; j < o.rec.size(); j += 8) for (size_t w = mf_ ? 2 : 1; w < 8; ++w) o.rec[j + w] = slot(o.rec[j + w]);
    if (mf_) for (size_t b = 0; b < o.batch; ++b) for (uint32_t j = chk_off_[b]; j < chk_off_[b + 1]; ++j)
        o.rec.insert(o.rec.end(), {(uint32_t)kScEq, (uint32_t)b, o.ds.chk[2 * j], o.ds.chk[2 * j + 1], 0u, 0u, 0u, 0u});
}

// Plans the proofs [b0, b1) of a batch into `out` until the plan holds `max_slots` pool slots (at least one proof); returns b1.
inline size_t sc_verify_plan_some(int mf, size_t b0, size_t batch, const uint8_t* const* proofs, const size_t* lens, const uint64_t* labels, size_t max_slots, ScVerifyPlan& out, bool& fits) {
    ScVerifyPlanner pl(mf); size_t b1 = b0;
    while (b1 < batch && (b1 == b0 || pl.slots() < max_slots)) { pl.add(proofs[b1], lens[b1], mf ? labels[b1] : 0); ++b1; }
    fits = pl.fits_u32();
    if (fits) pl.finish(out);
    return b1;
}

}  // namespace stark
