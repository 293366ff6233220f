// stark_mlwe_amd/csrc/sumcheck_batch.hpp — prove_plain / prove_mf (crates/channel/src/lib.rs:1045-1076, :1130-1172) of B independent
// witnesses of 2^k elements in one pass: the round loops written once, over an executor that runs the batched kernels
// (capi_sumcheck.hip: the device; hostcheck.cpp: the same bodies on the host).
//
// Every per-round step is ONE operation for the whole batch, whatever B:
//   * the Merkle commits (MerkleCommitment: arity 16, label per witness, commitment/src/lib.rs:85-90) run one DS level of all B trees per
//     launch (DsBatchStream); the top level writes the B roots straight into their slots of the value pool;
//   * the round coefficients write c0, c1 (and at round 0 the claim 2 c0 + c1) into the pool, the fold reads r_i from it;
//   * the Fiat-Shamir transcripts are B device-resident transcripts advanced by one launch (TrBatchStream): the host lays out once what
//     every instance absorbs as pool indices (labels, round indices, tags: constants; roots, c0, c1, claims, openings: value slots the
//     kernels fill), so prove_plain has no host round trip inside its round loop — one download of the value pool at the end.
//   * prove_mf syncs once per round (the query challenges decide the openings, as in the single path); the openings of every instance are
//     planned on the host (merkle_open_from over a recording source, fri_plan.hpp), gathered by ONE launch straight into the next round's
//     pool and absorbed from there; the opened values come back to the host once, at the end.
// Host-only C++ (no HIP).  The transcript labels (sc_lab) are the reference's strings, defined in sumcheck_impl.hpp, which includes this file.
#pragma once
#include <algorithm>
#include <cstring>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>
#include "fr.hpp"
#include "host_util.hpp"
#include "poseidon_streams.hpp"
#include "fri_plan.hpp"

namespace stark {

// ---- bincode layout of ProofPlain / ProofMF (channel/src/lib.rs:925-979) ---------------------------------------------------
struct BinW {
    std::vector<uint8_t>& b; explicit BinW(std::vector<uint8_t>& v) : b(v) {}
    void u64(uint64_t x) { enc_u64(b, x); }
    void fb(const fr_t& x) { u64(32); enc_fr(b, x); }                                      // FBytes: serde_bytes Vec<u8> of the 32-byte compressed element
    void idxs(const std::vector<size_t>& v) { u64(v.size()); for (size_t x : v) u64(x); }
    void fvec(const std::vector<fr_t>& v) { u64(v.size()); for (auto& x : v) fb(x); }
    void mproof(const MerkleProofHost& p) {                                                // MerkleProofBytes { arity, group_sizes, indices, siblings }
        u64(p.arity);
        u64(p.group_sizes.size()); for (auto& l : p.group_sizes) { u64(l.size()); for (uint8_t x : l) b.push_back(x); }
        idxs(p.indices);
        u64(p.siblings.size()); for (auto& l : p.siblings) fvec(l);
    }
};
struct RoundMFHost { fr_t c0, c1, next_root; std::vector<size_t> cur_indices, next_indices; std::vector<fr_t> cur_values, next_values; MerkleProofHost cur_proof, next_proof; };
static inline std::vector<uint8_t> lab_idx(const char* base, uint64_t i) { std::vector<uint8_t> l((const uint8_t*)base, (const uint8_t*)base + strlen(base)); for (int j = 0; j < 8; ++j) l.push_back((uint8_t)(i >> (8 * j))); return l; }
static inline std::vector<uint8_t> mf_query_label(uint64_t i, uint64_t j) { std::vector<uint8_t> l = lab_idx(sc_lab::mf_q, i); for (int b = 0; b < 8; ++b) l.push_back((uint8_t)(j >> (8 * b))); return l; }
static inline size_t mf_query_index(const fr_t& r, size_t half) {                            // :667-676
    const fr_t c = fr_to_canonical<PallasFr>(r); uint64_t acc = 0;
    for (int i = 0; i < 4; ++i) acc ^= (uint64_t)c.v[2 * i] | ((uint64_t)c.v[2 * i + 1] << 32);
    return (size_t)(acc % (uint64_t)half);
}

// ---- transcript layout: what each instance absorbs, as pool indices ---------------------------------------------------------
// Constants are interned into one host vector that lands in a pool at `base`; a value slot is an index the caller knows.
struct ScConsts {
    std::vector<fr_t> v; uint32_t base, tag;
    std::unordered_map<uint64_t, uint32_t> words;                        // small integers (u64 absorbs, group sizes): by value
    std::unordered_map<std::string, std::vector<uint32_t>> strs;         // absorb_bytes of a string: the marker and its words
    std::unordered_map<std::string, uint32_t> other;
    ScConsts(uint32_t base_, uint32_t tag_) : base(base_), tag(tag_) {}
    uint32_t put(const fr_t& x) { v.push_back(x); return tag | (base + (uint32_t)(v.size() - 1)); }
    uint32_t field(const fr_t& x) {
        std::string key((const char*)x.v, sizeof(x.v)); auto it = other.find(key);
        if (it != other.end()) return it->second;
        const uint32_t i = put(x); other.emplace(key, i); return i;
    }
    uint32_t word(uint64_t x) { auto it = words.find(x); if (it != words.end()) return it->second; const uint32_t i = put(host::h_u64(x)); words.emplace(x, i); return i; }
    const std::vector<uint32_t>& bytes(const uint8_t* b, size_t n) {                    // :67-73: marker, then 31-byte words
        std::string key((const char*)b, n); auto it = strs.find(key);
        if (it != strs.end()) return it->second;
        std::vector<uint32_t> e; e.push_back(field(host::h_tag("FSv1-ABSORB-BYTES")));
        for (size_t o = 0; o < n; o += 31) e.push_back(field(host::h_from_le_bytes_mod_order(b + o, std::min<size_t>(31, n - o))));
        return strs.emplace(key, std::move(e)).first->second;
    }
};
struct ScSeg {                                                          // the absorbs of DevTranscript, recorded instead of queued
    ScConsts& C; std::vector<uint32_t>& idx;
    void slot(uint32_t i) { idx.push_back(i); }
    void field(const fr_t& x) { idx.push_back(C.field(x)); }
    void bytes(const uint8_t* b, size_t n) { const auto& e = C.bytes(b, n); idx.insert(idx.end(), e.begin(), e.end()); }
    void str(const char* s) { bytes((const uint8_t*)s, strlen(s)); }
    void u64(uint64_t x) { idx.push_back(C.field(host::h_tag("FSv1-ABSORB-BYTES"))); idx.push_back(C.word(x)); }   // absorb_u64: 8 LE bytes = one word
    void byte(uint8_t x) { idx.push_back(C.field(host::h_tag("FSv1-ABSORB-BYTES"))); idx.push_back(C.word(x)); }
    void challenge(const std::vector<uint8_t>& label) { idx.push_back(C.field(host::h_tag("FSv1-CHALLENGE"))); bytes(label.data(), label.size()); }
    void digest(const char* label, uint32_t s) { str(sc_lab::digest); str(label); slot(s); }     // send_digest (:22-26)
};

#define SC_TRY(e) do { int32_t rc__ = (e); if (rc__) return rc__; } while (0)

// An executor X is an arena (alloc / upload / put / download: DevArena in ctx.hpp on the GPU, HostArena in hostcheck.cpp; pointers are its own
// memory) plus:
//   int32_t ds_level(const DsBatchStream& D, fr_t* out)        one Merkle level of all trees (MerkleCommitment's parameters)
//   int32_t coeffs(const fr_t* const* ptrs, const fr_t* layers, size_t len, size_t B, fr_t* c01, fr_t* claim)
//           c01[2b], c01[2b+1] = (c0, c1) of layer b (ptrs[b] or layers + b len); claim != nullptr: claim[b] = 2 c0 + c1
//   int32_t fold(const fr_t* const* ptrs, const fr_t* layers, size_t len, size_t B, const fr_t* r, fr_t* next)   next + b len/2 with r[b]
//   int32_t transcript(const TrBatchStream& T)                 (the transcript parameters)
//   int32_t gather(const fr_t* const* addr, size_t n, fr_t* out)   out[j] = *addr[j]
template <class X> struct ScBatch {
    X& x; size_t B, k, n; const fr_t* const* wit; const uint64_t* labels;
    const fr_t* const* wit_x = nullptr; const uint64_t* labels_x = nullptr;
    fr_t init_cap;
    ScBatch(X& x_, size_t B_, const fr_t* const* w, size_t k_, const uint64_t* l) : x(x_), B(B_), k(k_), n((size_t)1 << k_), wit(w), labels(l) {
        init_cap = host::h_tag("FSv1-TRANSCRIPT-INIT");
    }
    template <class T> int32_t put(const std::vector<T>& h, T** out) { return x.put(h, out); }
    int32_t alloc_fr(size_t n_fr, fr_t** out) { void* p = nullptr; SC_TRY(x.alloc(std::max<size_t>(n_fr, 1) * sizeof(fr_t), &p)); *out = (fr_t*)p; return 0; }
    int32_t setup() {
        std::vector<const fr_t*> w(wit, wit + B); std::vector<uint64_t> l(labels, labels + B);
        const fr_t** wp = nullptr; uint64_t* lp = nullptr;
        SC_TRY(put(w, &wp)); SC_TRY(put(l, &lp)); wit_x = wp; labels_x = lp; return 0;
    }
    int32_t gather(const std::vector<const fr_t*>& addr, fr_t* out) {
        if (addr.empty()) return 0;
        const fr_t** a = nullptr; SC_TRY(put(addr, &a)); return x.gather(a, addr.size(), out);
    }
    // The trees of B same-shape layers: level v of tree b at base[v] + b lens[v] (level 0 of the witnesses: wit[b]).
    struct Trees {
        std::vector<size_t> lens; std::vector<const fr_t*> base; const fr_t* const* ptrs = nullptr;
        const fr_t* addr(size_t b, size_t level, size_t i) const { return level == 0 && ptrs ? ptrs[b] + i : base[level] + b * lens[level] + i; }
    };
    // MerkleProver::commit_vector of each layer (merkle_build_on: level 0, positions from 0); roots[b] = root of tree b
    int32_t commit(const fr_t* const* ptrs_x, const fr_t* const* ptrs_host, const fr_t* layers, size_t len, fr_t* roots, Trees& T) {
        T.lens.assign(1, len); T.base.assign(1, layers); T.ptrs = ptrs_host;
        if (len == 1) { std::vector<const fr_t*> a(B); for (size_t b = 0; b < B; ++b) a[b] = T.addr(b, 0, 0); return gather(a, roots); }
        const fr_t* const* in_ptrs = ptrs_x; const fr_t* in = layers; uint32_t level = 0;
        while (len > 1) {
            const size_t nn = (len + 15) / 16;
            fr_t* dst = roots; if (nn > 1) SC_TRY(alloc_fr(B * nn, &dst));
            SC_TRY(x.ds_level(DsBatchStream::make(16, level, 0, labels_x, in_ptrs, in, len, B), dst));
            T.lens.push_back(nn); T.base.push_back(dst);                                   // the top level is the root slots (never opened)
            in_ptrs = nullptr; in = dst; len = nn; ++level;
        }
        return 0;
    }
    TrBatchStream stream(fr_t* state, uint32_t* pos, size_t inst0, const uint32_t* inst, size_t n_active, size_t nseg, const uint32_t* el_off, const uint32_t* idx,
                         const fr_t* pool0, const fr_t* pool1, fr_t* out, bool reset) const {
        TrBatchStream T; T.state = state; T.pos = pos; T.inst = inst; T.inst0 = inst0; T.n_active = n_active; T.nseg = nseg; T.el_off = el_off; T.idx = idx;
        T.pool0 = pool0; T.pool1 = pool1; T.out = out; T.init_cap = init_cap; T.reset = reset ? 1 : 0; T.finish_last = 1; return T;
    }

    // ---- prove_plain (:1045-1076) ----------------------------------------------------------------------------------------------
    int32_t prove_plain(std::vector<std::vector<uint8_t>>& proofs) {
        SC_TRY(setup());
        // pool: value slots [root | claim | final | (c0, c1) per round | r per round], then the constants
        const size_t v_root = 0, v_claim = B, v_fin = 2 * B, v_c = 3 * B, v_r = 3 * B + 2 * B * k, V = 3 * B + 3 * B * k;
        ScConsts C((uint32_t)V, 0u);
        std::vector<uint32_t> idx, off(1, 0);
        for (size_t i = 0; i < k; ++i) {
            const std::vector<uint8_t> lb = lab_idx(sc_lab::r, i);
            for (size_t b = 0; b < B; ++b) {
                ScSeg S{C, idx};
                if (i == 0) { S.str(sc_lab::plain); S.digest(sc_lab::root, (uint32_t)(v_root + b)); S.str(sc_lab::claim); S.slot((uint32_t)(v_claim + b)); }   // send_claim (:434-446)
                S.str(sc_lab::round); S.u64(i);                                                                         // round (:448-472)
                S.str(sc_lab::c0); S.slot((uint32_t)(v_c + 2 * B * i + 2 * b)); S.str(sc_lab::c1); S.slot((uint32_t)(v_c + 2 * B * i + 2 * b + 1));
                S.challenge(lb);
                off.push_back((uint32_t)idx.size());
            }
        }
        fr_t* pool = nullptr; SC_TRY(alloc_fr(V + C.v.size(), &pool));
        if (!C.v.empty()) SC_TRY(x.upload(pool + V, C.v.data(), C.v.size() * sizeof(fr_t)));
        Trees T; SC_TRY(commit(wit_x, wit, nullptr, n, pool + v_root, T));                                           // MerkleProver::commit_vector (:172-179)
        if (k == 0) {                                                                                                  // claim = final = the single element
            std::vector<const fr_t*> a(2 * B); for (size_t b = 0; b < B; ++b) a[b] = a[B + b] = wit[b];
            SC_TRY(gather(a, pool + v_claim));
        } else {
            uint32_t *d_off = nullptr, *d_idx = nullptr; SC_TRY(put(off, &d_off)); SC_TRY(put(idx, &d_idx));
            fr_t *state = nullptr, *bufA = nullptr, *bufB = nullptr; void* pos = nullptr;
            SC_TRY(alloc_fr(17 * B, &state)); SC_TRY(x.alloc(4 * B, &pos));
            SC_TRY(alloc_fr(B * std::max<size_t>(n / 2, 1), &bufA)); SC_TRY(alloc_fr(B * std::max<size_t>(n / 4, 1), &bufB));
            const fr_t* const* src_p = wit_x; const fr_t* src = nullptr; size_t len = n;
            for (size_t i = 0; i < k; ++i) {
                SC_TRY(x.coeffs(src_p, src, len, B, pool + v_c + 2 * B * i, i == 0 ? pool + v_claim : nullptr));
                SC_TRY(x.transcript(stream(state, (uint32_t*)pos, 0, nullptr, B, 1, d_off + i * B, d_idx, pool, nullptr, pool + v_r + B * i, i == 0)));
                fr_t* nx = i + 1 == k ? pool + v_fin : ((i & 1) ? bufB : bufA);
                SC_TRY(x.fold(src_p, src, len, B, pool + v_r + B * i, nx));
                src_p = nullptr; src = nx; len /= 2;
            }
        }
        std::vector<fr_t> v(V); SC_TRY(x.download(v.data(), pool, V * sizeof(fr_t)));                              // roots, claims, coefficients, finals
        proofs.assign(B, {});
        for (size_t b = 0; b < B; ++b) {
            BinW W(proofs[b]);
            W.fb(v[v_root + b]); W.u64(k); for (size_t i = 0; i < k; ++i) { W.fb(v[v_c + 2 * B * i + 2 * b]); W.fb(v[v_c + 2 * B * i + 2 * b + 1]); }
            proofs[b].push_back(0);                                                                                   // extra_openings: None
            W.fb(v[v_fin + b]);
        }
        return 0;
    }

    // ---- prove_mf (:1130-1172) -------------------------------------------------------------------------------------------------
    // A recording source over the trees of one instance: each digest request becomes an address to gather.
    struct AddrSource : FriSource {
        const Trees* t[2]; size_t b; std::vector<const fr_t*>& addr;
        AddrSource(const Trees* cur, const Trees* nxt, size_t b_, std::vector<const fr_t*>& a) : b(b_), addr(a) { t[0] = cur; t[1] = nxt; }
        int32_t layer(size_t, const std::vector<size_t>&, std::vector<fr_t>&) override { return -1; }
        int32_t digests(size_t tree, size_t level, const std::vector<size_t>& idx, std::vector<fr_t>& out) override {
            for (size_t i : idx) addr.push_back(t[tree]->addr(b, level, i));
            out.assign(idx.size(), host::h_zero()); return 0;
        }
    };
    int32_t prove_mf(size_t qpr, std::vector<std::vector<uint8_t>>& proofs) {
        SC_TRY(setup());
        // pool0: value slots [root r = 0..k | claim | (c0, c1) per round | r per round], then the constants of the round transcripts
        const size_t v_root = 0, v_claim = (k + 1) * B, v_c = (k + 2) * B, v_r = (k + 2) * B + 2 * B * k, V = (k + 2) * B + 3 * B * k;
        ScConsts C0((uint32_t)V, 0u);
        std::vector<uint32_t> ridx, roff(1, 0);                                     // mf_round_challenge_from_root (:592-598): a fresh transcript per round
        for (size_t i = 0; i < k; ++i) for (size_t b = 0; b < B; ++b) {
            ScSeg S{C0, ridx};
            S.str(sc_lab::mf_round_chal); S.str(sc_lab::mf_r); S.u64(i); S.slot((uint32_t)(v_root + i * B + b));
            S.challenge(std::vector<uint8_t>(sc_lab::r_i, sc_lab::r_i + strlen(sc_lab::r_i)));
            roff.push_back((uint32_t)ridx.size());
        }
        fr_t* pool = nullptr; SC_TRY(alloc_fr(V + C0.v.size(), &pool));
        if (!C0.v.empty()) SC_TRY(x.upload(pool + V, C0.v.data(), C0.v.size() * sizeof(fr_t)));
        Trees cur; SC_TRY(commit(wit_x, wit, nullptr, n, pool + v_root, cur));                                     // SumCheckMFProver::new (:601-622)
        std::vector<std::vector<RoundMFHost>> R(B, std::vector<RoundMFHost>(k));
        struct Opened { const fr_t* region; size_t n; std::vector<size_t> at; };   // gathered opening values of one round: region[0 .. n), instance b from at[b]
        std::vector<Opened> opened;
        if (k > 0) {
            uint32_t *d_roff = nullptr, *d_ridx = nullptr; SC_TRY(put(roff, &d_roff)); SC_TRY(put(ridx, &d_ridx));
            fr_t *state = nullptr, *bufA = nullptr, *bufB = nullptr, *qout = nullptr; void* pos = nullptr;
            SC_TRY(alloc_fr(17 * 2 * B, &state)); SC_TRY(x.alloc(4 * 2 * B, &pos));                                  // instances [0, B): main, [B, 2B): round transcripts
            SC_TRY(alloc_fr(B * std::max<size_t>(n / 2, 1), &bufA)); SC_TRY(alloc_fr(B * std::max<size_t>(n / 4, 1), &bufB));
            SC_TRY(alloc_fr(B * std::min(std::max(qpr, (size_t)1), n / 2), &qout));
            const fr_t* const* src_p = wit_x; const fr_t* src = nullptr; size_t len = n;
            // main segments of round i: [openings of round i-1 | prefix at round 0] + the round's absorbs + the first query challenge; then one challenge each
            std::vector<uint32_t> midx, moff(1, 0);
            ScConsts C1(0u, TrBatchStream::kPool1);
            auto round_segments = [&](size_t i, size_t b, size_t q_target, ScSeg& S) {
                if (i == 0) { S.str(sc_lab::mf); S.digest(sc_lab::mf_root0, (uint32_t)(v_root + b)); S.str(sc_lab::mf_claim); S.slot((uint32_t)(v_claim + b)); }   // send_claim (:624-629)
                S.str(sc_lab::mf_round); S.u64(i);
                S.str(sc_lab::c0); S.slot((uint32_t)(v_c + 2 * B * i + 2 * b)); S.str(sc_lab::c1); S.slot((uint32_t)(v_c + 2 * B * i + 2 * b + 1));
                S.digest(sc_lab::mf_root_next, (uint32_t)(v_root + (i + 1) * B + b));
                for (size_t j = 0; j < q_target; ++j) { if (j) moff.push_back((uint32_t)midx.size()); S.challenge(mf_query_label(i, j)); }
                moff.push_back((uint32_t)midx.size());
            };
            { const size_t qt0 = std::min(std::max(qpr, (size_t)1), n / 2); for (size_t b = 0; b < B; ++b) { ScSeg S{C1, midx}; round_segments(0, b, qt0, S); } }
            const fr_t* region = nullptr; size_t region_g = 0;                      // the pool1 of the current round's main segments
            { fr_t* r0 = nullptr; SC_TRY(put(C1.v, &r0)); region = r0; }
            for (size_t i = 0; i < k; ++i) {                                         // round (:631-737)
                const size_t half = len / 2, q_target = std::min(std::max(qpr, (size_t)1), half);   // :656
                SC_TRY(x.coeffs(src_p, src, len, B, pool + v_c + 2 * B * i, i == 0 ? pool + v_claim : nullptr));
                SC_TRY(x.transcript(stream(state, (uint32_t*)pos, B, nullptr, B, 1, d_roff + i * B, d_ridx, pool, nullptr, pool + v_r + B * i, true)));
                fr_t* nx = (i & 1) ? bufB : bufA;
                SC_TRY(x.fold(src_p, src, len, B, pool + v_r + B * i, nx));
                Trees nxt; SC_TRY(commit(nullptr, nullptr, nx, half, pool + v_root + (i + 1) * B, nxt));
                { uint32_t *d_off = nullptr, *d_idx = nullptr; SC_TRY(put(moff, &d_off)); SC_TRY(put(midx, &d_idx));
                  SC_TRY(x.transcript(stream(state, (uint32_t*)pos, 0, nullptr, B, q_target, d_off, d_idx, pool, region, qout, i == 0))); }
                std::vector<fr_t> ch(B * q_target); SC_TRY(x.download(ch.data(), qout, ch.size() * sizeof(fr_t)));   // the round's one host sync
                // query indices (:656-690): draws until q_target distinct or max_attempts; the few instances with duplicates draw again together
                const size_t max_attempts = std::max(q_target * 16, (size_t)16);
                std::vector<std::set<size_t>> qs(B); std::vector<size_t> drawn(B, q_target);
                for (size_t b = 0; b < B; ++b) for (size_t j = 0; j < q_target; ++j) qs[b].insert(mf_query_index(ch[b * q_target + j], half));
                for (;;) {
                    std::vector<uint32_t> inst; std::vector<size_t> want;
                    for (size_t b = 0; b < B; ++b) if (qs[b].size() < q_target && drawn[b] < max_attempts) { inst.push_back((uint32_t)b); want.push_back(std::min(q_target - qs[b].size(), max_attempts - drawn[b])); }
                    if (inst.empty()) break;
                    const size_t d = *std::min_element(want.begin(), want.end());   // one uniform launch; instances that need more come round again
                    ScConsts Cr(0u, TrBatchStream::kPool1); std::vector<uint32_t> ridx2, roff2(1, 0);
                    for (size_t a = 0; a < inst.size(); ++a) for (size_t j = 0; j < d; ++j) { ScSeg S{Cr, ridx2}; S.challenge(mf_query_label(i, drawn[inst[a]] + j)); roff2.push_back((uint32_t)ridx2.size()); }
                    uint32_t *d_inst = nullptr, *d_off = nullptr, *d_idx = nullptr; fr_t* d_c = nullptr; fr_t* d_out = nullptr;
                    SC_TRY(put(inst, &d_inst)); SC_TRY(put(roff2, &d_off)); SC_TRY(put(ridx2, &d_idx)); SC_TRY(put(Cr.v, &d_c)); SC_TRY(alloc_fr(inst.size() * d, &d_out));
                    SC_TRY(x.transcript(stream(state, (uint32_t*)pos, 0, d_inst, inst.size(), d, d_off, d_idx, pool, d_c, d_out, false)));
                    std::vector<fr_t> c2(inst.size() * d); SC_TRY(x.download(c2.data(), d_out, c2.size() * sizeof(fr_t)));
                    for (size_t a = 0; a < inst.size(); ++a) { for (size_t j = 0; j < d; ++j) qs[inst[a]].insert(mf_query_index(c2[a * d + j], half)); drawn[inst[a]] += d; }
                }
                // openings: every instance's requests, one gather into the next round's pool
                std::vector<const fr_t*> addr; Opened O; O.at.resize(B);
                for (size_t b = 0; b < B; ++b) {
                    for (size_t idx0 = 0; idx0 < half && qs[b].size() < q_target; ++idx0) qs[b].insert(idx0);     // :683-690
                    RoundMFHost& M = R[b][i]; O.at[b] = addr.size();
                    for (size_t jj : qs[b]) { M.cur_indices.push_back(2 * jj); M.cur_indices.push_back(2 * jj + 1); }
                    M.next_indices.assign(qs[b].begin(), qs[b].end());
                    AddrSource src_b(&cur, &nxt, b, addr);
                    for (size_t ix : M.cur_indices) addr.push_back(cur.addr(b, 0, ix));
                    if (merkle_open_from(src_b, 0, cur.lens, 16, M.cur_indices, M.cur_proof)) return -1;
                    for (size_t ix : M.next_indices) addr.push_back(nxt.addr(b, 0, ix));
                    if (merkle_open_from(src_b, 1, nxt.lens, 16, M.next_indices, M.next_proof)) return -1;
                }
                O.n = addr.size();
                midx.clear(); moff.assign(1, 0); ScConsts C2((uint32_t)O.n, TrBatchStream::kPool1);
                if (i + 1 < k) {
                    const size_t qn = std::min(std::max(qpr, (size_t)1), half / 2);
                    for (size_t b = 0; b < B; ++b) {                               // send_opening (:32-62) of both openings, then round i+1
                        ScSeg S{C2, midx}; const RoundMFHost& M = R[b][i]; uint32_t g = (uint32_t)O.at[b] | TrBatchStream::kPool1;
                        auto opening = [&](const std::vector<size_t>& ix, const MerkleProofHost& pr) {
                            S.str(sc_lab::open);
                            for (size_t v : ix) S.u64(v);
                            for (size_t j = 0; j < ix.size(); ++j) S.slot(g++);
                            S.str(sc_lab::arity); S.u64(pr.arity);
                            S.str(sc_lab::group_sizes);
                            for (auto& l : pr.group_sizes) { S.u64(l.size()); for (uint8_t sz : l) S.byte(sz); }
                            S.str(sc_lab::siblings);
                            for (auto& l : pr.siblings) { S.u64(l.size()); for (size_t j = 0; j < l.size(); ++j) S.slot(g++); }
                        };
                        opening(M.cur_indices, M.cur_proof); opening(M.next_indices, M.next_proof);
                        round_segments(i + 1, b, qn, S);
                    }
                }
                fr_t* reg = nullptr; SC_TRY(alloc_fr(O.n + C2.v.size(), &reg));
                if (!C2.v.empty()) SC_TRY(x.upload(reg + O.n, C2.v.data(), C2.v.size() * sizeof(fr_t)));
                SC_TRY(gather(addr, reg));
                O.region = reg; opened.push_back(std::move(O)); region = reg; region_g = O.n;
                cur = nxt; src_p = nullptr; src = nx; len = half;
            }
            (void)region_g;
        }
        std::vector<fr_t> v(V); SC_TRY(x.download(v.data(), pool, V * sizeof(fr_t)));
        std::vector<std::vector<fr_t>> got(opened.size());
        for (size_t i = 0; i < opened.size(); ++i) { got[i].resize(opened[i].n); if (opened[i].n) SC_TRY(x.download(got[i].data(), opened[i].region, opened[i].n * sizeof(fr_t))); }
        proofs.assign(B, {});
        for (size_t b = 0; b < B; ++b) {
            BinW W(proofs[b]);
            W.fb(v[v_root + b]); W.u64(k);
            for (size_t i = 0; i < k; ++i) {
                RoundMFHost& M = R[b][i]; const fr_t* g = got[i].data() + opened[i].at[b];
                M.c0 = v[v_c + 2 * B * i + 2 * b]; M.c1 = v[v_c + 2 * B * i + 2 * b + 1]; M.next_root = v[v_root + (i + 1) * B + b];
                M.cur_values.assign(g, g + M.cur_indices.size()); g += M.cur_indices.size();
                for (auto& l : M.cur_proof.siblings) for (auto& s : l) s = *g++;
                M.next_values.assign(g, g + M.next_indices.size()); g += M.next_indices.size();
                for (auto& l : M.next_proof.siblings) for (auto& s : l) s = *g++;
                W.fb(M.c0); W.fb(M.c1); W.fb(M.next_root); W.idxs(M.cur_indices); W.fvec(M.cur_values); W.mproof(M.cur_proof); W.idxs(M.next_indices); W.fvec(M.next_values); W.mproof(M.next_proof);
            }
            W.fb(v[v_root + k * B + b]);                                          // the final evaluation: the one-leaf tree's root is the leaf
        }
        return 0;
    }
};
#undef SC_TRY

}  // namespace stark
