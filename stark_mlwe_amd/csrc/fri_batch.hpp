// stark_mlwe_amd/csrc/fri_batch.hpp — the commit phase of deep_fri_prove (fri_build_transcript, crates/deep_ali/src/fri.rs:231-312) for a
// pass of Bp traces of equal (n0, schedule, seed_z) side by side: the layer loops written once, over an executor that runs the batched
// kernels (capi_fri.hip: the device; hostcheck.cpp: the same stream bodies on the host).
//
// Every step is ONE operation for the whole pass, whatever Bp:
//   * layer l of all traces is one trace-major buffer of Bp * n_l elements (layer 0 is filled by the caller: the batched merge writes it, or
//     one copy kernel over a pointer table);
//   * a fold, and the leaf-pair hashes of a hashed arity, run over that concatenation as if it were one layer of Bp * n_l elements.  This is
//     exact: the fold challenge z_l depends only on (seed_z, l, n_l) (fri.rs:250), so all traces share it, and every m_l divides n_l, so
//     neither a fold group (b m_l .. (b + 1) m_l) nor a leaf's partner index i / m_l crosses from one trace's slice into the next;
//   * the pair leaves of an unhashed arity (4 and 2; every prove has one: the last layer is arity 2 with zero partners, fri.rs:266, 289) are
//     one DsBatchPairStream launch, and the Merkle levels of the Bp same-shape trees are merkle_climb (merkle_batch.hpp): one DsBatchStream launch
//     per level under a per-tree label array holding l; the top level writes the Bp roots of layer l into roots[l * Bp ..];
//   * layers 1..L are committed between fork() and side(false) — the device runs them on its side stream underneath layer 0, as fri_build does.
// A pass of ONE trace does not come here: its commit is fri_build_impl (capi_fri.hip: PassCommit::run chooses), whose levels are DsStreams and
// reach k_node16_pair and the "fri_side_pair" form; everything before and after the commit phase is shared by both forms.
// Nothing here synchronises the host.  Memory of a pass: the layers (Bp n0 (1 + 1/m_0 + ...)), the leaf digests of every layer (the same
// again) and the upper tree levels (at most 1/(arity - 1) of that): about Bp * n0 * 32 B * (2 + small), all released with the executor.
// Host-only C++ (no HIP).
#pragma once
#include <string>
#include <vector>
#include "fr.hpp"
#include "host_util.hpp"
#include "poseidon_streams.hpp"
#include "fri_plan.hpp"
#include "merkle_batch.hpp"

namespace stark {

// The RNG part of fri_sample_z_ell (fri.rs:59-82) from fused = H("FRI/z/l", [seed_z, level, domain_size]): the first candidate outside the domain.
inline fr_t fri_z_from_fused(const fr_t& fused, uint64_t seed_z, size_t level, size_t domain_size) {
    uint8_t seed[32]; host::h_to_bytes_le(fused, seed);
    host::ChaCha12Rng rng(seed);
    const fr_t one = host::h_one();
    for (size_t tries = 0;;) {
        const fr_t cand = host::h_u64(rng.next_u64());
        if (!fr_is_zero(cand) && !fr_eq(fr_pow_u64<PallasFr>(cand, domain_size), one)) return cand;
        if (++tries >= 1000) {
            const fr_t fb = host::h_u64(seed_z + (uint64_t)level + 7);
            return !fr_eq(fr_pow_u64<PallasFr>(fb, domain_size), one) ? fb : host::h_u64(11);
        }
    }
}

#define FB_TRY(e) do { int32_t rc__ = (e); if (rc__) return rc__; } while (0)

// An executor X is an arena (alloc / upload / put: DevArena in ctx.hpp on the GPU, HostArena in hostcheck.cpp; pointers are its own memory) plus:
//   int32_t zpows(const fr_t& z, size_t m, fr_t* zp)            zp[t] = z^t, t < m
//   int32_t fold(const fr_t* f, size_t n, const fr_t* zp, size_t m, fr_t* out)              fri_fold_layer over n elements
//   int32_t leaf_pairs(const fr_t* f, const fr_t* f_next, size_t n, size_t m, fr_t* h)      hash_leaf_pair(f[i], f_next[i / m]) (f_next == nullptr: zero)
//   template <class DS> int32_t hash_level(size_t arity, const DS& D, fr_t* out)            one launch over the hashes of D (the Merkle parameters of `arity`)
//   int32_t fork() / void side(bool on) / int32_t join()        work issued while side(true) may run concurrently with what follows side(false) until join()
template <class X> struct FriBatchCommit {
    X& x; size_t Bp = 0, L = 0;
    std::vector<size_t> sched, n, arity; std::vector<fr_t> z;
    std::vector<fr_t*> f;                                                       // f[l]: Bp x n[l], trace-major
    struct Tree { std::vector<fr_t*> levels; std::vector<size_t> lens; };       // levels[v]: Bp x lens[v]; the top level is roots + l * Bp
    std::vector<Tree> trees;
    fr_t* roots = nullptr;                                                      // (L + 1) x Bp, layer-major
    uint64_t* labels = nullptr; std::vector<uint64_t> labels_host;              // (L + 1) x Bp: labels[l * Bp + b] = l
    explicit FriBatchCommit(X& x_) : x(x_) {}

    // The executor the climb of one layer sees: X's memory, and X's hashes under the Merkle parameters of that layer's arity.
    struct AtArity {
        FriBatchCommit& c; size_t arity;
        int32_t level_block(size_t k, fr_t** out) { return c.alloc_fr(k, out); }
        template <class DS> int32_t hash_level(const DS& D, fr_t* out) { return c.x.hash_level(arity, D, out); }
    };
    int32_t alloc_fr(size_t k, fr_t** out) { void* p = nullptr; FB_TRY(x.alloc((k ? k : 1) * sizeof(fr_t), &p)); *out = (fr_t*)p; return 0; }
    // The shapes of a pass (fri_layers).  -1: an empty layer or a schedule that does not divide; -2: a layer with arity 1.
    int32_t shape(size_t Bp_, size_t n0, const size_t* schedule, size_t L_, std::string& err) {
        Bp = Bp_; L = L_; sched.assign(schedule, schedule + L);
        const LayerShape sh = Bp ? fri_layers(n0, schedule, L, n, arity) : LayerShape::empty_layer;
        if (sh == LayerShape::arity_one) { err = "arity 1 with more than one leaf never terminates in the reference"; return -2; }
        if (sh != LayerShape::ok) { err = layer_shape_text(sh); return -1; }
        return 0;
    }
    // After shape(): the layers, the root and label buffers; z_[l] = fri_sample_z_ell(seed_z, l, n[l]).  The caller then fills f[0] and calls run().
    int32_t init(const fr_t* z_) {
        z.assign(z_, z_ + L);
        f.assign(L + 1, nullptr); trees.assign(L + 1, Tree());
        for (size_t l = 0; l <= L; ++l) FB_TRY(alloc_fr(Bp * n[l], &f[l]));
        FB_TRY(alloc_fr((L + 1) * Bp, &roots));
        labels_host.resize((L + 1) * Bp); for (size_t l = 0; l <= L; ++l) for (size_t b = 0; b < Bp; ++b) labels_host[l * Bp + b] = l;
        void* lp = nullptr; FB_TRY(x.alloc(labels_host.size() * sizeof(uint64_t), &lp)); labels = (uint64_t*)lp;
        return x.upload(labels, labels_host.data(), labels_host.size() * sizeof(uint64_t));
    }
    // The commitment of layer l of every trace: leaf digests (hash_leaf_pair for a hashed arity, fri.rs:283; pair leaves otherwise, fri.rs:289),
    // then MerkleTree::new's levels up to the Bp roots (a layer of one element: the leaf digests are the roots).
    int32_t commit_layer(size_t l) {
        const size_t a = arity[l], nl = n[l], m = l < L ? sched[l] : 1;
        const fr_t* f_next = l < L ? f[l + 1] : nullptr;                                                        // zero partners on the last layer (fri.rs:266)
        AtArity xa{*this, a};
        fr_t* leaves = roots + l * Bp; if (nl > 1) FB_TRY(xa.level_block(Bp * nl, &leaves));
        if (hashed_arity(a)) FB_TRY(x.leaf_pairs(f[l], f_next, Bp * nl, m, leaves));
        else FB_TRY(xa.hash_level(DsBatchPairStream::make(a, labels + l * Bp, f[l], f_next, nl, m, Bp), leaves));
        return merkle_climb(xa, a, Bp, labels + l * Bp, nullptr, leaves, nl, roots + l * Bp, trees[l].lens, trees[l].levels);
    }
    int32_t run() {
        size_t zp_total = 0; for (size_t l = 0; l < L; ++l) zp_total += sched[l];
        fr_t* zp = nullptr; if (L) FB_TRY(alloc_fr(zp_total, &zp));
        for (size_t l = 0, off = 0; l < L; off += sched[l], ++l) {                                                // the folds back to back: no challenge depends on a commitment
            FB_TRY(x.zpows(z[l], sched[l], zp + off));
            FB_TRY(x.fold(f[l], Bp * n[l], zp + off, sched[l], f[l + 1]));
        }
        FB_TRY(x.fork());
        x.side(true);
        int32_t rc = 0;
        for (size_t l = L; l >= 1 && !rc; --l) rc = commit_layer(l);
        x.side(false);
        if (!rc) rc = commit_layer(0);
        const int32_t jrc = x.join();
        return rc ? rc : jrc;
    }
    const fr_t* layer_at(size_t b, size_t l) const { return f[l] + b * n[l]; }
    const fr_t* level_at(size_t b, size_t l, size_t v) const { return trees[l].levels[v] + b * trees[l].lens[v]; }
};

}  // namespace stark
