// stark_mlwe_amd/csrc/sumcheck_batch.hpp — prove_plain / prove_mf (crates/channel/src/lib.rs:1045-1076, :1130-1172) of B independent
// witnesses of 2^k[b] elements (any mix of sizes; see ScBatch) in one pass: the round loops written once, over an executor that runs the batched kernels
// (capi_sumcheck.hip: the device; hostcheck.cpp: the same bodies on the host).
//
// Every per-round step is ONE operation for the whole batch, whatever B:
//   * the Merkle commits (MerkleCommitment: arity 16, label per witness, commitment/src/lib.rs:85-90) run one DS level of all B trees per
//     launch (merkle_climb / merkle_climb_ragged, merkle_batch.hpp); the top level writes the B roots straight into their slots of the value pool;
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
#include "merkle_batch.hpp"

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
//   template <class DS> int32_t hash_level(const DS& D, fr_t* out)   one Merkle level of all trees (MerkleCommitment's parameters): DsBatchStream,
//           or DsRaggedStream for trees of different lengths (the witnesses' commit)
//   int32_t coeffs(const fr_t* const* ptrs, const fr_t* layers, size_t len, size_t B, fr_t* c01, fr_t* claim, size_t claim_from)
//           c01[2b], c01[2b+1] = (c0, c1) of layer b (ptrs[b] or layers + b len); claim != nullptr: claim[b] = 2 c0 + c1 for b >= claim_from
//   int32_t fold(const fr_t* const* ptrs, const fr_t* layers, size_t len, size_t B, const fr_t* r, fr_t* next)   next + b len/2 with r[b]
//   int32_t transcript(const TrBatchStream& T)                 (the transcript parameters)
//   int32_t gather(const fr_t* const* addr, size_t n, fr_t* out)   out[j] = *addr[j]
//
// Instances of different sizes: witness b has 2^k[b] elements.  The rounds are aligned at the END: with K = max k, instance b joins at step
// K - k[b] with its witness as its layer, so at step j every active instance holds a layer of 2^(K - j) elements and runs its round j - (K - k[b]).
// The instances are ordered by k descending (stable; the proofs go back in the caller's order), so the active set of a step is a prefix [0, A_j)
// and the joiners of a step are its tail [A_{j-1}, A_j): every per-step array (partial sums, c0 / c1, r, next layers, next roots, transcript
// segments) is indexed by b with A_j in place of B, the round kernels and the commits of the folded layers stay uniform, and only the commit of
// the witnesses is ragged.  A step with joiners reads its layers through a pointer table (earlier instances: their slice of the layer buffer,
// joiners: their witness); every such table is built on the host up front and goes up with the witness table.  k[b] = 0: claim = final = the
// witness's only element, no round; it never enters a step.  Equal k is the case A_j = B for every j.
template <class X> struct ScBatch {
    X& x; size_t B, K; const fr_t* const* wit; const uint64_t* labels; const size_t* kin;
    std::vector<size_t> perm, ks, A;                                       // sorted position -> caller's index; k in sorted order; active count per step
    std::vector<const fr_t*> wit_s; std::vector<uint64_t> labels_s;      // in sorted order (host copies)
    const fr_t* const* wit_x = nullptr; const uint64_t* labels_x = nullptr;
    std::vector<const fr_t* const*> step_ptrs;                             // the layer pointer table of step j in X's memory, or nullptr: contiguous
    fr_t* buf[2] = {nullptr, nullptr};                                     // the folded layers of even / odd steps: A_j x 2^(K - j - 1)
    fr_t init_cap;
    ScBatch(X& x_, size_t B_, const fr_t* const* w, const size_t* k_, const uint64_t* l) : x(x_), B(B_), K(0), wit(w), labels(l), kin(k_) {
        init_cap = host::h_tag("FSv1-TRANSCRIPT-INIT");
    }
    template <class T> int32_t put(const std::vector<T>& h, T** out) { return x.put(h, out); }
    int32_t alloc_fr(size_t n_fr, fr_t** out) { void* p = nullptr; SC_TRY(x.alloc(std::max<size_t>(n_fr, 1) * sizeof(fr_t), &p)); *out = (fr_t*)p; return 0; }
    size_t len_at(size_t j) const { return (size_t)1 << (K - j); }         // the layer length of step j
    size_t prev_active(size_t j) const { return j ? A[j - 1] : 0; }        // the instances of step j that ran step j - 1 (the others join)
    size_t round_of(size_t b, size_t j) const { return j - (K - ks[b]); }  // the round instance b runs at step j
    size_t step_of(size_t b, size_t i) const { return i + (K - ks[b]); }
    int32_t setup() {
        perm.resize(B); for (size_t b = 0; b < B; ++b) perm[b] = b;
        std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return kin[a] > kin[b]; });
        ks.resize(B); wit_s.resize(B); labels_s.resize(B);
        for (size_t b = 0; b < B; ++b) { ks[b] = kin[perm[b]]; wit_s[b] = wit[perm[b]]; labels_s[b] = labels[perm[b]]; }
        K = B ? ks[0] : 0; A.assign(K, 0);
        for (size_t j = 0; j < K; ++j) { size_t a = prev_active(j); while (a < B && ks[a] >= K - j) ++a; A[j] = a; }
        size_t need[2] = {0, 0};
        for (size_t j = 0; j < K; ++j) need[j & 1] = std::max(need[j & 1], A[j] * (len_at(j) / 2));
        if (K) { SC_TRY(alloc_fr(need[0], &buf[0])); SC_TRY(alloc_fr(need[1], &buf[1])); }
        // ONE table: the witnesses (the table of step 0, where everyone active joins), then the table of every later step that has joiners
        std::vector<const fr_t*> tab(wit_s); std::vector<size_t> at(K, 0);
        for (size_t j = 1; j < K; ++j) if (A[j] > A[j - 1]) {
            at[j] = tab.size();
            for (size_t b = 0; b < A[j]; ++b) tab.push_back(b < A[j - 1] ? buf[(j - 1) & 1] + b * len_at(j) : wit_s[b]);
        }
        const fr_t** wp = nullptr; uint64_t* lp = nullptr;
        SC_TRY(put(tab, &wp)); SC_TRY(put(labels_s, &lp)); wit_x = wp; labels_x = lp;
        step_ptrs.assign(K, nullptr);
        for (size_t j = 0; j < K; ++j) if (j == 0 || A[j] > A[j - 1]) step_ptrs[j] = wp + at[j];
        return 0;
    }
    const fr_t* step_layers(size_t j) const { return step_ptrs[j] ? nullptr : buf[(j - 1) & 1]; }
    int32_t gather(const std::vector<const fr_t*>& addr, fr_t* out) {
        if (addr.empty()) return 0;
        const fr_t** a = nullptr; SC_TRY(put(addr, &a)); return x.gather(a, addr.size(), out);
    }
    // One committed layer of one instance: its level lengths and where each level starts (level 0: the layer itself).
    struct Tree {
        std::vector<size_t> lens; std::vector<const fr_t*> lv;
        const fr_t* addr(size_t level, size_t i) const { return lv[level] + i; }
    };
    static constexpr size_t kArity = 16;                                   // MerkleCommitment's (commitment/src/lib.rs:85-90)
    // The executor the climbs see (merkle_batch.hpp): X's memory and hashes, the segment tables through put().
    struct Levels {
        ScBatch& s;
        int32_t level_block(size_t n_fr, fr_t** out) { return s.alloc_fr(n_fr, out); }
        template <class DS> int32_t hash_level(const DS& D, fr_t* out) { return s.x.hash_level(D, out); }
        int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** o) { DsRaggedStream::Seg* d = nullptr; SC_TRY(s.put(h, &d)); *o = d; return 0; }
    };
    // MerkleProver::commit_vector of the layers of the first `A` instances, all of `len` elements, at layers + b len or behind a pointer table
    // (ptrs_x in X's memory, ptrs_host its host copy), read in place as level 0; roots[b] = root of tree b: the top level is the root slots (never
    // opened), and the root of a one-leaf tree, its leaf, comes by a gather.
    int32_t commit_layers(const fr_t* const* ptrs_x, const fr_t* const* ptrs_host, const fr_t* layers, size_t len, size_t A_, fr_t* roots, std::vector<Tree>& T) {
        T.assign(A_, Tree());
        if (len == 1) {
            std::vector<const fr_t*> a(A_);
            for (size_t b = 0; b < A_; ++b) { T[b].lens.assign(1, 1); T[b].lv.assign(1, ptrs_host ? ptrs_host[b] : layers + b); a[b] = T[b].lv[0]; }
            return gather(a, roots);
        }
        Levels xl{*this}; std::vector<size_t> lens; std::vector<fr_t*> base;
        SC_TRY(merkle_climb(xl, kArity, A_, labels_x, ptrs_x, layers, len, roots, lens, base));
        for (size_t b = 0; b < A_; ++b) {
            T[b].lens = lens; T[b].lv.assign(1, ptrs_host ? ptrs_host[b] : layers + b * len);
            for (size_t v = 1; v < lens.size(); ++v) T[b].lv.push_back(base[v] + b * lens[v]);
        }
        return 0;
    }
    // The same of all B witnesses, tree b of 2^ks[b] leaves, read in place: merkle_climb_ragged, level v one launch over the trees that have it — a
    // prefix, the trees being ordered by size.  The top level (the largest trees' roots) is written straight into the root slots; the roots of the
    // trees that end below it, and of the one-leaf trees, follow with one gather.  Witnesses of ONE size take the same-shape stream (a division finds
    // the tree of a hash where the ragged stream searches its table: measured).
    int32_t commit_witnesses(fr_t* roots, std::vector<Tree>& W) {
        if (B && ks.front() == ks.back()) return commit_layers(wit_x, wit_s.data(), nullptr, (size_t)1 << ks[0], B, roots, W);
        std::vector<size_t> n(B); for (size_t b = 0; b < B; ++b) n[b] = (size_t)1 << ks[b];
        MerkleRaggedPlan P = merkle_ragged_plan(kArity, B, n.data(), labels_s.data(), false);
        Levels xl{*this}; std::vector<fr_t*> base;
        SC_TRY(merkle_climb_ragged(xl, P, wit_s.data(), roots, base, [](const DsRaggedStream::Seg*) { return 0; }));
        W.assign(B, Tree()); std::vector<const fr_t*> a; size_t first = 0;
        for (size_t b = 0; b < B; ++b) {
            W[b].lens = P.lens[b]; W[b].lv.assign(1, wit_s[b]);
            for (size_t v = 1; v < P.lens[b].size(); ++v) W[b].lv.push_back(base[v] + P.at[b][v]);
            if (P.depth > 1 && P.lens[b].size() == P.depth) first = b + 1; else a.push_back(W[b].lv.back());
        }
        return gather(a, roots + first);
    }
    TrBatchStream stream(fr_t* state, uint32_t* pos, size_t inst0, const uint32_t* inst, size_t n_active, size_t nseg, const uint32_t* el_off, const uint32_t* idx,
                         const fr_t* pool0, const fr_t* pool1, fr_t* out, size_t reset_from) const {
        TrBatchStream T; T.state = state; T.pos = pos; T.inst = inst; T.inst0 = inst0; T.n_active = n_active; T.nseg = nseg; T.el_off = el_off; T.idx = idx;
        T.pool0 = pool0; T.pool1 = pool1; T.out = out; T.init_cap = init_cap; T.reset_from = reset_from; T.finish_last = 1; return T;
    }
    // claim = final = the only element of the witnesses that have no round: the tail [Z, B) of the ordered instances
    int32_t no_round_values(size_t Z, fr_t* claim, fr_t* fin) {
        std::vector<const fr_t*> a; for (size_t b = Z; b < B; ++b) a.push_back(wit_s[b]);
        if (Z == 0 && fin == claim + B) { std::vector<const fr_t*> a2(a); a2.insert(a2.end(), a.begin(), a.end()); return gather(a2, claim); }
        SC_TRY(gather(a, claim + Z)); return gather(a, fin + Z);
    }

    // ---- prove_plain (:1045-1076) ----------------------------------------------------------------------------------------------
    int32_t prove_plain(std::vector<std::vector<uint8_t>>& proofs) {
        SC_TRY(setup());
        // pool: value slots [root | claim | final] per instance, then per step [(c0, c1) of the active instances], then per step [r], then the constants
        const size_t v_root = 0, v_claim = B, v_fin = 2 * B; size_t V = 3 * B;
        std::vector<size_t> v_c(K), v_r(K), s0(K);
        for (size_t j = 0; j < K; ++j) { v_c[j] = V; V += 2 * A[j]; }
        for (size_t j = 0; j < K; ++j) { v_r[j] = V; V += A[j]; }
        ScConsts C((uint32_t)V, 0u);
        std::vector<uint32_t> idx, off(1, 0);
        for (size_t j = 0; j < K; ++j) {
            s0[j] = off.size() - 1;
            for (size_t b = 0; b < A[j]; ++b) {
                const size_t i = round_of(b, j); ScSeg S{C, idx};
                if (i == 0) { S.str(sc_lab::plain); S.digest(sc_lab::root, (uint32_t)(v_root + b)); S.str(sc_lab::claim); S.slot((uint32_t)(v_claim + b)); }   // send_claim (:434-446)
                S.str(sc_lab::round); S.u64(i);                                                                         // round (:448-472)
                S.str(sc_lab::c0); S.slot((uint32_t)(v_c[j] + 2 * b)); S.str(sc_lab::c1); S.slot((uint32_t)(v_c[j] + 2 * b + 1));
                S.challenge(lab_idx(sc_lab::r, i));
                off.push_back((uint32_t)idx.size());
            }
        }
        fr_t* pool = nullptr; SC_TRY(alloc_fr(V + C.v.size(), &pool));
        if (!C.v.empty()) SC_TRY(x.upload(pool + V, C.v.data(), C.v.size() * sizeof(fr_t)));
        std::vector<Tree> W; SC_TRY(commit_witnesses(pool + v_root, W));                                             // MerkleProver::commit_vector (:172-179)
        const size_t Z = K ? A[K - 1] : 0;                                                                             // the instances with at least one round
        if (Z < B) SC_TRY(no_round_values(Z, pool + v_claim, pool + v_fin));
        if (K) {
            uint32_t *d_off = nullptr, *d_idx = nullptr; SC_TRY(put(off, &d_off)); SC_TRY(put(idx, &d_idx));
            fr_t* state = nullptr; void* pos = nullptr;
            SC_TRY(alloc_fr(17 * B, &state)); SC_TRY(x.alloc(4 * B, &pos));
            for (size_t j = 0; j < K; ++j) {
                const size_t len = len_at(j), Aj = A[j], P = prev_active(j);
                SC_TRY(x.coeffs(step_ptrs[j], step_layers(j), len, Aj, pool + v_c[j], P < Aj ? pool + v_claim : nullptr, P));
                SC_TRY(x.transcript(stream(state, (uint32_t*)pos, 0, nullptr, Aj, 1, d_off + s0[j], d_idx, pool, nullptr, pool + v_r[j], P)));
                fr_t* nx = j + 1 == K ? pool + v_fin : buf[j & 1];
                SC_TRY(x.fold(step_ptrs[j], step_layers(j), len, Aj, pool + v_r[j], nx));
            }
        }
        std::vector<fr_t> v(V); SC_TRY(x.download(v.data(), pool, V * sizeof(fr_t)));                              // roots, claims, coefficients, finals
        proofs.assign(B, {});
        for (size_t b = 0; b < B; ++b) {
            std::vector<uint8_t>& out = proofs[perm[b]]; BinW W_(out);
            W_.fb(v[v_root + b]); W_.u64(ks[b]);
            for (size_t i = 0; i < ks[b]; ++i) { const size_t j = step_of(b, i); W_.fb(v[v_c[j] + 2 * b]); W_.fb(v[v_c[j] + 2 * b + 1]); }
            out.push_back(0);                                                                                         // extra_openings: None
            W_.fb(v[v_fin + b]);
        }
        return 0;
    }

    // ---- prove_mf (:1130-1172) -------------------------------------------------------------------------------------------------
    // A recording source over the two trees of one instance: each digest request becomes an address to gather.
    struct AddrSource : FriSource {
        const Tree* t[2]; std::vector<const fr_t*>& addr;
        AddrSource(const Tree* cur, const Tree* nxt, std::vector<const fr_t*>& a) : addr(a) { t[0] = cur; t[1] = nxt; }
        int32_t layer(size_t, const std::vector<size_t>&, std::vector<fr_t>&) override { return -1; }
        int32_t digests(size_t tree, size_t level, const std::vector<size_t>& idx, std::vector<fr_t>& out) override {
            for (size_t i : idx) addr.push_back(t[tree]->addr(level, i));
            out.assign(idx.size(), host::h_zero()); return 0;
        }
    };
    int32_t prove_mf(size_t qpr, std::vector<std::vector<uint8_t>>& proofs) {
        SC_TRY(setup());
        // pool0: value slots [witness root | claim] per instance, then per step [next root], [(c0, c1)], [r] of the active instances, then the
        // constants of the round transcripts
        const size_t v_root0 = 0, v_claim = B; size_t V = 2 * B;
        std::vector<size_t> v_next(K), v_c(K), v_r(K), s0(K);
        for (size_t j = 0; j < K; ++j) { v_next[j] = V; V += A[j]; }
        for (size_t j = 0; j < K; ++j) { v_c[j] = V; V += 2 * A[j]; }
        for (size_t j = 0; j < K; ++j) { v_r[j] = V; V += A[j]; }
        auto root_slot = [&](size_t b, size_t i) { return (uint32_t)(i == 0 ? v_root0 + b : v_next[step_of(b, i) - 1] + b); };   // the root of round i's layer
        ScConsts C0((uint32_t)V, 0u);
        std::vector<uint32_t> ridx, roff(1, 0);                                     // mf_round_challenge_from_root (:592-598): a fresh transcript per round
        for (size_t j = 0; j < K; ++j) {
            s0[j] = roff.size() - 1;
            for (size_t b = 0; b < A[j]; ++b) {
                const size_t i = round_of(b, j); ScSeg S{C0, ridx};
                S.str(sc_lab::mf_round_chal); S.str(sc_lab::mf_r); S.u64(i); S.slot(root_slot(b, i));
                S.challenge(std::vector<uint8_t>(sc_lab::r_i, sc_lab::r_i + strlen(sc_lab::r_i)));
                roff.push_back((uint32_t)ridx.size());
            }
        }
        fr_t* pool = nullptr; SC_TRY(alloc_fr(V + C0.v.size(), &pool));
        if (!C0.v.empty()) SC_TRY(x.upload(pool + V, C0.v.data(), C0.v.size() * sizeof(fr_t)));
        std::vector<Tree> W; SC_TRY(commit_witnesses(pool + v_root0, W));                                          // SumCheckMFProver::new (:601-622)
        std::vector<std::vector<RoundMFHost>> R(B); for (size_t b = 0; b < B; ++b) R[b].resize(ks[b]);
        struct Opened { const fr_t* region; size_t n; std::vector<size_t> at; };   // gathered opening values of one step: region[0 .. n), instance b from at[b]
        std::vector<Opened> opened;
        if (K > 0) {
            uint32_t *d_roff = nullptr, *d_ridx = nullptr; SC_TRY(put(roff, &d_roff)); SC_TRY(put(ridx, &d_ridx));
            fr_t *state = nullptr, *qout = nullptr; void* pos = nullptr;
            SC_TRY(alloc_fr(17 * 2 * B, &state)); SC_TRY(x.alloc(4 * 2 * B, &pos));                                  // instances [0, B): main, [B, 2B): round transcripts
            auto q_of = [&](size_t j) { return std::min(std::max(qpr, (size_t)1), len_at(j) / 2); };                 // :656
            { size_t nq = 0; for (size_t j = 0; j < K; ++j) nq = std::max(nq, A[j] * q_of(j)); SC_TRY(alloc_fr(nq, &qout)); }
            // main segments of step j, instance b: [openings of its previous round | prefix at its round 0] + the round's absorbs + the first query
            // challenge; then one challenge each
            std::vector<uint32_t> midx, moff(1, 0);
            auto round_segments = [&](size_t j, size_t b, ScSeg& S) {
                const size_t i = round_of(b, j), q_target = q_of(j);
                if (i == 0) { S.str(sc_lab::mf); S.digest(sc_lab::mf_root0, (uint32_t)(v_root0 + b)); S.str(sc_lab::mf_claim); S.slot((uint32_t)(v_claim + b)); }   // send_claim (:624-629)
                S.str(sc_lab::mf_round); S.u64(i);
                S.str(sc_lab::c0); S.slot((uint32_t)(v_c[j] + 2 * b)); S.str(sc_lab::c1); S.slot((uint32_t)(v_c[j] + 2 * b + 1));
                S.digest(sc_lab::mf_root_next, (uint32_t)(v_next[j] + b));
                for (size_t q = 0; q < q_target; ++q) { if (q) moff.push_back((uint32_t)midx.size()); S.challenge(mf_query_label(i, q)); }
                moff.push_back((uint32_t)midx.size());
            };
            ScConsts C1(0u, TrBatchStream::kPool1);
            for (size_t b = 0; b < A[0]; ++b) { ScSeg S{C1, midx}; round_segments(0, b, S); }
            const fr_t* region = nullptr;                                           // the pool1 of the current step's main segments
            { fr_t* r0 = nullptr; SC_TRY(put(C1.v, &r0)); region = r0; }
            std::vector<Tree> cur(W.begin(), W.begin() + A[0]);
            for (size_t j = 0; j < K; ++j) {                                         // round (:631-737)
                const size_t len = len_at(j), half = len / 2, q_target = q_of(j), Aj = A[j], P = prev_active(j);
                SC_TRY(x.coeffs(step_ptrs[j], step_layers(j), len, Aj, pool + v_c[j], P < Aj ? pool + v_claim : nullptr, P));
                SC_TRY(x.transcript(stream(state, (uint32_t*)pos, B, nullptr, Aj, 1, d_roff + s0[j], d_ridx, pool, nullptr, pool + v_r[j], 0)));
                fr_t* nx = buf[j & 1];
                SC_TRY(x.fold(step_ptrs[j], step_layers(j), len, Aj, pool + v_r[j], nx));
                std::vector<Tree> nxt; SC_TRY(commit_layers(nullptr, nullptr, nx, half, Aj, pool + v_next[j], nxt));
                { uint32_t *d_off = nullptr, *d_idx = nullptr; SC_TRY(put(moff, &d_off)); SC_TRY(put(midx, &d_idx));
                  SC_TRY(x.transcript(stream(state, (uint32_t*)pos, 0, nullptr, Aj, q_target, d_off, d_idx, pool, region, qout, P))); }
                std::vector<fr_t> ch(Aj * q_target); SC_TRY(x.download(ch.data(), qout, ch.size() * sizeof(fr_t)));   // the step's one host sync
                // query indices (:656-690): draws until q_target distinct or max_attempts; the few instances with duplicates draw again together
                const size_t max_attempts = std::max(q_target * 16, (size_t)16);
                std::vector<std::set<size_t>> qs(Aj); std::vector<size_t> drawn(Aj, q_target);
                for (size_t b = 0; b < Aj; ++b) for (size_t q = 0; q < q_target; ++q) qs[b].insert(mf_query_index(ch[b * q_target + q], half));
                for (;;) {
                    std::vector<uint32_t> inst; std::vector<size_t> want;
                    for (size_t b = 0; b < Aj; ++b) if (qs[b].size() < q_target && drawn[b] < max_attempts) { inst.push_back((uint32_t)b); want.push_back(std::min(q_target - qs[b].size(), max_attempts - drawn[b])); }
                    if (inst.empty()) break;
                    const size_t d = *std::min_element(want.begin(), want.end());   // one uniform launch; instances that need more come round again
                    ScConsts Cr(0u, TrBatchStream::kPool1); std::vector<uint32_t> ridx2, roff2(1, 0);
                    for (size_t a = 0; a < inst.size(); ++a) for (size_t q = 0; q < d; ++q) { ScSeg S{Cr, ridx2}; S.challenge(mf_query_label(round_of(inst[a], j), drawn[inst[a]] + q)); roff2.push_back((uint32_t)ridx2.size()); }
                    uint32_t *d_inst = nullptr, *d_off = nullptr, *d_idx = nullptr; fr_t* d_c = nullptr; fr_t* d_out = nullptr;
                    SC_TRY(put(inst, &d_inst)); SC_TRY(put(roff2, &d_off)); SC_TRY(put(ridx2, &d_idx)); SC_TRY(put(Cr.v, &d_c)); SC_TRY(alloc_fr(inst.size() * d, &d_out));
                    SC_TRY(x.transcript(stream(state, (uint32_t*)pos, 0, d_inst, inst.size(), d, d_off, d_idx, pool, d_c, d_out, inst.size())));
                    std::vector<fr_t> c2(inst.size() * d); SC_TRY(x.download(c2.data(), d_out, c2.size() * sizeof(fr_t)));
                    for (size_t a = 0; a < inst.size(); ++a) { for (size_t q = 0; q < d; ++q) qs[inst[a]].insert(mf_query_index(c2[a * d + q], half)); drawn[inst[a]] += d; }
                }
                // openings: every active instance's requests, one gather into the next step's pool
                std::vector<const fr_t*> addr; Opened O; O.at.resize(Aj);
                for (size_t b = 0; b < Aj; ++b) {
                    for (size_t idx0 = 0; idx0 < half && qs[b].size() < q_target; ++idx0) qs[b].insert(idx0);     // :683-690
                    RoundMFHost& M = R[b][round_of(b, j)]; O.at[b] = addr.size();
                    for (size_t jj : qs[b]) { M.cur_indices.push_back(2 * jj); M.cur_indices.push_back(2 * jj + 1); }
                    M.next_indices.assign(qs[b].begin(), qs[b].end());
                    AddrSource src_b(&cur[b], &nxt[b], addr);
                    for (size_t ix : M.cur_indices) addr.push_back(cur[b].addr(0, ix));
                    if (merkle_open_from(src_b, 0, cur[b].lens, kArity, M.cur_indices, M.cur_proof)) return -1;
                    for (size_t ix : M.next_indices) addr.push_back(nxt[b].addr(0, ix));
                    if (merkle_open_from(src_b, 1, nxt[b].lens, kArity, M.next_indices, M.next_proof)) return -1;
                }
                O.n = addr.size();
                midx.clear(); moff.assign(1, 0); ScConsts C2((uint32_t)O.n, TrBatchStream::kPool1);
                if (j + 1 < K) {
                    for (size_t b = 0; b < A[j + 1]; ++b) {                        // send_opening (:32-62) of both openings, then the next round; a joiner: its prefix
                        ScSeg S{C2, midx};
                        if (b < Aj) {
                            const RoundMFHost& M = R[b][round_of(b, j)]; uint32_t g = (uint32_t)O.at[b] | TrBatchStream::kPool1;
                            auto opening = [&](const std::vector<size_t>& ix, const MerkleProofHost& pr) {
                                S.str(sc_lab::open);
                                for (size_t v : ix) S.u64(v);
                                for (size_t q = 0; q < ix.size(); ++q) S.slot(g++);
                                S.str(sc_lab::arity); S.u64(pr.arity);
                                S.str(sc_lab::group_sizes);
                                for (auto& l : pr.group_sizes) { S.u64(l.size()); for (uint8_t sz : l) S.byte(sz); }
                                S.str(sc_lab::siblings);
                                for (auto& l : pr.siblings) { S.u64(l.size()); for (size_t q = 0; q < l.size(); ++q) S.slot(g++); }
                            };
                            opening(M.cur_indices, M.cur_proof); opening(M.next_indices, M.next_proof);
                        }
                        round_segments(j + 1, b, S);
                    }
                }
                fr_t* reg = nullptr; SC_TRY(alloc_fr(O.n + C2.v.size(), &reg));
                if (!C2.v.empty()) SC_TRY(x.upload(reg + O.n, C2.v.data(), C2.v.size() * sizeof(fr_t)));
                SC_TRY(gather(addr, reg));
                O.region = reg; opened.push_back(std::move(O)); region = reg;
                cur = std::move(nxt);
                if (j + 1 < K) cur.insert(cur.end(), W.begin() + Aj, W.begin() + A[j + 1]);                         // the joiners of the next step: their witness trees
            }
        }
        std::vector<fr_t> v(V); SC_TRY(x.download(v.data(), pool, V * sizeof(fr_t)));
        std::vector<std::vector<fr_t>> got(opened.size());
        for (size_t j = 0; j < opened.size(); ++j) { got[j].resize(opened[j].n); if (opened[j].n) SC_TRY(x.download(got[j].data(), opened[j].region, opened[j].n * sizeof(fr_t))); }
        proofs.assign(B, {});
        for (size_t b = 0; b < B; ++b) {
            std::vector<uint8_t>& out = proofs[perm[b]]; BinW W_(out);
            W_.fb(v[v_root0 + b]); W_.u64(ks[b]);
            for (size_t i = 0; i < ks[b]; ++i) {
                const size_t j = step_of(b, i); RoundMFHost& M = R[b][i]; const fr_t* g = got[j].data() + opened[j].at[b];
                M.c0 = v[v_c[j] + 2 * b]; M.c1 = v[v_c[j] + 2 * b + 1]; M.next_root = v[v_next[j] + b];
                M.cur_values.assign(g, g + M.cur_indices.size()); g += M.cur_indices.size();
                for (auto& l : M.cur_proof.siblings) for (auto& s : l) s = *g++;
                M.next_values.assign(g, g + M.next_indices.size()); g += M.next_indices.size();
                for (auto& l : M.next_proof.siblings) for (auto& s : l) s = *g++;
                W_.fb(M.c0); W_.fb(M.c1); W_.fb(M.next_root); W_.idxs(M.cur_indices); W_.fvec(M.cur_values); W_.mproof(M.cur_proof); W_.idxs(M.next_indices); W_.fvec(M.next_values); W_.mproof(M.next_proof);
            }
            W_.fb(v[ks[b] ? v_next[K - 1] + b : v_root0 + b]);                   // the final evaluation: the one-leaf tree's root is the leaf
        }
        return 0;
    }
};
#undef SC_TRY

}  // namespace stark
