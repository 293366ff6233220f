// stark_mlwe_amd/csrc/poseidon_streams.hpp — what the Poseidon sponges absorb, written once for every kernel form (host and device).
//
// A stream describes a batch of sponges: sponge k absorbs total(k) elements, element q read by elem(k, q), into a state whose capacity
// element starts as the stream's `cap` (TrStream resolves sponge k first: sponge(k).total(), sponge(k).elem(q)).  The lane bodies (poseidon_dev.hpp, also instantiated on the host by the host-check library), the
// one-wave (poseidon_coop.hpp), wave-pair (poseidon_pair.hpp), five-wave (poseidon_chain.hpp) and wide (poseidon_wave.hpp) kernels all read
// their inputs through these types; only the absorb schedule (eager or lazy permute) and the arithmetic differ between them.
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>
#include "fr.hpp"
#include "dev_common.hpp"

namespace stark {

typedef PallasFr PF;   // the prover field

// hash_with_ds_dynamic([arity, level, pos0 + k, label] || children_k || 1)  (merkle/src/lib.rs:167-176), eager sponge, zero padded, cap 0.
//   mode 0 (node level): children_k = in0[k*arity .. min((k+1)*arity, n_in))  (the last node of a level may be ragged)
//   mode 1 (pair leaf) : children_k = {in0[k], in1[k / cp_div]}  (merkle/src/lib.rs:380-388); in1 == nullptr: the second child is zero
//                        (fri.rs:266).  cp_div = m serves commit_pairs(f_l, s_l) with s_l the view f_{l+1}[i/m].
// (The verifiers' union-of-paths levels, whose parents are scattered, are DsGatherStream's.)
struct DsStream {
    fr_t arity_f, level_f, label_f; uint64_t pos0; size_t arity, n_in, n_out; int mode; size_t cp_div;
    const fr_t* in0; const fr_t* in1;
    static inline DsStream make(int mode, size_t arity, uint32_t level, uint64_t pos0, uint64_t label, const fr_t* in0, const fr_t* in1, size_t n_in,
                                size_t cp_div = 1) {
        DsStream D;
        D.arity_f = fr_from_u64<PF>(arity); D.level_f = fr_from_u64<PF>(level); D.label_f = fr_from_u64<PF>(label); D.pos0 = pos0;
        D.arity = arity; D.n_in = n_in; D.mode = mode; D.cp_div = cp_div ? cp_div : 1; D.in0 = in0; D.in1 = in1;
        D.n_out = mode == 1 ? n_in : (n_in + D.arity - 1) / D.arity;
        return D;
    }
    FR_HD uint64_t position(size_t k) const { return pos0 + k; }
    FR_HD size_t total(size_t k) const { return 4 + (mode == 1 ? 2 : ((k + 1) * arity <= n_in ? arity : n_in - k * arity)) + 1; }
    FR_HD size_t max_total() const { return 4 + (mode == 1 ? 2 : arity) + 1; }      // the widest sponge of the batch
    FR_HD fr_t elem(size_t k, size_t q) const {
        if (q < 4) return q == 0 ? arity_f : (q == 1 ? level_f : (q == 2 ? fr_from_u64<PF>(position(k)) : label_f));
        if (q == total(k) - 1) return fr_one<PF>();
        const size_t c = q - 4;
        if (mode == 1) return c == 0 ? ldg(in0 + k) : (in1 ? ldg(in1 + k / cp_div) : fr_zero<PF>());
        return ldg(in0 + k * arity + c);
    }
};

// The batch verifier's DS hashes (fri_verify_batch.hpp): the hashes of one (width, depth) step of every opening of every proof.
//   hash k = hash_with_ds_dynamic([hdr[4k] .. hdr[4k+3]] || pool[idx[off[k]]] .. pool[idx[off[k+1] - 1]] || 1), eager sponge, cap 0
// with the header (arity, level, position, label) given per hash and the children gathered from the plan's pool (off: CSR into idx).
// A pair leaf of an unhashed layer is such a hash with two children and level 2^32 - 1.
struct DsGatherStream {
    const uint64_t* hdr; const uint32_t* off; const uint32_t* idx; const fr_t* pool; size_t n_out, max_children;
    FR_HD uint64_t position(size_t k) const { return hdr[4 * k + 2]; }
    FR_HD size_t total(size_t k) const { return 4 + (size_t)(off[k + 1] - off[k]) + 1; }
    FR_HD size_t max_total() const { return 4 + max_children + 1; }
    FR_HD fr_t elem(size_t k, size_t q) const {
        if (q < 4) return fr_from_u64<PF>(hdr[4 * k + q]);
        if (q == total(k) - 1) return fr_one<PF>();
        return ldg(pool + idx[off[k] + (q - 4)]);
    }
};

// One Merkle level of B same-shape trees in one launch (the batched sum-check commits, sumcheck_batch.hpp): hash k belongs to tree
// k / nodes_per_tree and is node j = k % nodes_per_tree of that tree's level, position pos0 + j, under the tree's own label.
//   hash k = hash_with_ds_dynamic([arity, level, pos0 + j, labels[tree]] || children || 1), eager sponge, zero padded, cap 0
// with children in_tree[j*arity .. min((j+1)*arity, n_in)) (the last node of every tree may be ragged) and in_tree = in_ptrs[tree] (a
// device array of per-tree pointers: the witnesses) or in + tree * n_in (a contiguous B x n_in buffer: the folded layers and upper levels).
struct DsBatchStream {
    fr_t arity_f, level_f; uint64_t pos0; const uint64_t* labels; size_t arity, n_in, nodes_per_tree, n_out;
    const fr_t* const* in_ptrs; const fr_t* in;
    static inline DsBatchStream make(size_t arity, uint32_t level, uint64_t pos0, const uint64_t* labels, const fr_t* const* in_ptrs, const fr_t* in, size_t n_in, size_t trees) {
        DsBatchStream D;
        D.arity_f = fr_from_u64<PF>(arity); D.level_f = fr_from_u64<PF>(level); D.pos0 = pos0; D.labels = labels; D.arity = arity; D.n_in = n_in;
        D.nodes_per_tree = (n_in + arity - 1) / arity; D.n_out = D.nodes_per_tree * trees; D.in_ptrs = in_ptrs; D.in = in;
        return D;
    }
    FR_HD size_t tree(size_t k) const { return k / nodes_per_tree; }
    FR_HD uint64_t position(size_t k) const { return pos0 + k % nodes_per_tree; }
    FR_HD size_t total(size_t k) const { const size_t j = k % nodes_per_tree; return 4 + ((j + 1) * arity <= n_in ? arity : n_in - j * arity) + 1; }
    FR_HD size_t max_total() const { return 4 + arity + 1; }
    FR_HD fr_t elem(size_t k, size_t q) const {
        if (q < 4) return q == 0 ? arity_f : (q == 1 ? level_f : (q == 2 ? fr_from_u64<PF>(position(k)) : fr_from_u64<PF>(labels[tree(k)])));
        if (q == total(k) - 1) return fr_one<PF>();
        const size_t t = tree(k), j = k % nodes_per_tree;
        const fr_t* src = in_ptrs ? in_ptrs[t] : in + t * n_in;
        return ldg(src + j * arity + (q - 4));
    }
};

// The pair leaves of B same-shape unhashed FRI layers in one launch (the batched commit phase, fri_batch.hpp): DsStream mode 1 with per-tree
// positions.  Hash k belongs to tree k / n and is leaf j = k % n of it, position j, under the tree's own label:
//   hash k = hash_with_ds_dynamic([arity, 2^32 - 1, k % n, labels[k / n]] || f[k], cp ? cp[k / cp_div] : 0 || 1), eager sponge, cap 0
// with f the B x n trace-major layer and cp the B x (n / cp_div) next one (cp_div divides n, so k / cp_div stays inside tree k / n's slice).
struct DsBatchPairStream {
    fr_t arity_f, level_f; const uint64_t* labels; size_t n, n_out, cp_div; const fr_t* f; const fr_t* cp;
    static inline DsBatchPairStream make(size_t arity, const uint64_t* labels, const fr_t* f, const fr_t* cp, size_t n, size_t cp_div, size_t trees) {
        DsBatchPairStream D;
        D.arity_f = fr_from_u64<PF>(arity); D.level_f = fr_from_u64<PF>(0xFFFFFFFFu); D.labels = labels; D.n = n; D.n_out = n * trees;
        D.cp_div = cp_div ? cp_div : 1; D.f = f; D.cp = cp;
        return D;
    }
    FR_HD uint64_t position(size_t k) const { return k % n; }
    FR_HD size_t total(size_t) const { return 7; }
    FR_HD size_t max_total() const { return 7; }
    FR_HD fr_t elem(size_t k, size_t q) const {
        if (q < 4) return q == 0 ? arity_f : (q == 1 ? level_f : (q == 2 ? fr_from_u64<PF>(position(k)) : fr_from_u64<PF>(labels[k / n])));
        if (q == 6) return fr_one<PF>();
        return q == 4 ? ldg(f + k) : (cp ? ldg(cp + k / cp_div) : fr_zero<PF>());
    }
};

// The pair leaves of B same-shape trees whose columns live wherever the caller put them (the batched Merkle build, merkle_batch.hpp):
// DsBatchPairStream read through two device arrays of per-tree pointers.  Hash k belongs to tree k / n and is leaf j = k % n of it:
//   hash k = hash_with_ds_dynamic([arity, 2^32 - 1, j, labels[k / n]] || f[k / n][j], cp[k / n] ? cp[k / n][j] : 0 || 1), eager sponge, cap 0
// A null cp[b] makes every second child of tree b zero (MerkleTree::new_pairs over a zero column, fri.rs:266).
struct DsBatchPairPtrStream {
    fr_t arity_f, level_f; const uint64_t* labels; size_t n, n_out; const fr_t* const* f; const fr_t* const* cp;
    static inline DsBatchPairPtrStream make(size_t arity, const uint64_t* labels, const fr_t* const* f, const fr_t* const* cp, size_t n, size_t trees) {
        DsBatchPairPtrStream D;
        D.arity_f = fr_from_u64<PF>(arity); D.level_f = fr_from_u64<PF>(0xFFFFFFFFu); D.labels = labels; D.n = n; D.n_out = n * trees; D.f = f; D.cp = cp;
        return D;
    }
    FR_HD uint64_t position(size_t k) const { return k % n; }
    FR_HD size_t total(size_t) const { return 7; }
    FR_HD size_t max_total() const { return 7; }
    FR_HD fr_t elem(size_t k, size_t q) const {
        if (q < 4) return q == 0 ? arity_f : (q == 1 ? level_f : (q == 2 ? fr_from_u64<PF>(position(k)) : fr_from_u64<PF>(labels[k / n])));
        if (q == 6) return fr_one<PF>();
        const size_t b = k / n, j = k % n;
        if (q == 4) return ldg(f[b] + j);
        const fr_t* c = cp[b];
        return c ? ldg(c + j) : fr_zero<PF>();
    }
};

// One Merkle level of trees of DIFFERENT lengths in one launch (the mixed-size batch build, merkle_batch.hpp): DsStream per segment.  Segment s is
// one tree that still has this level: its input pointer(s), its own n_in and label, and `first`, the index of its first hash in the launch (the
// prefix sums of the segments' hash counts; a segment has at least one hash).  Hash k belongs to the segment whose range [first, next first) holds
// k and is node or leaf j = k - first of that tree, position pos0 + j; out[k] is written, so a launch's block is the trees' slices back to back.
//   mode 0 (node level): hash k = hash_with_ds_dynamic([arity, level, pos0 + j, label_s] || in0_s[j*arity .. min((j+1)*arity, n_in_s)) || 1)
//   mode 1 (pair leaf) : hash k = hash_with_ds_dynamic([arity, level, pos0 + j, label_s] || in0_s[j], in1_s ? in1_s[j] : 0 || 1)
// eager sponge, zero padded, cap 0: per hash what DsStream mode 0 / DsBatchPairPtrStream give on that tree alone.  The segment of a hash is found by
// a binary search over `first` (n_seg <= the number of trees of the call; the table stays in cache over the 21 reads of a hash).
struct DsRaggedStream {
    struct Seg { const fr_t* in0; const fr_t* in1; uint64_t n_in, label, first; };
    fr_t arity_f, level_f; uint64_t pos0; size_t arity, n_seg, n_out; int mode; const Seg* segs;
    // the number of hashes a tree of n_in inputs has in a launch of this mode
    static inline size_t hashes(int mode, size_t arity, size_t n_in) { return mode == 1 ? n_in : (n_in + arity - 1) / arity; }
    // segs: the table in the memory the kernels read (n_seg entries); n_out: the sum of the segments' hash counts (what the table's `first` add up to)
    static inline DsRaggedStream make(int mode, size_t arity, uint32_t level, uint64_t pos0, const Seg* segs, size_t n_seg, size_t n_out) {
        DsRaggedStream D;
        D.arity_f = fr_from_u64<PF>(arity); D.level_f = fr_from_u64<PF>(level); D.pos0 = pos0; D.arity = arity; D.n_seg = n_seg; D.n_out = n_out; D.mode = mode; D.segs = segs;
        return D;
    }
    FR_HD size_t seg(size_t k) const {                                 // the last segment whose first hash is <= k
        size_t lo = 0, hi = n_seg;
        while (hi - lo > 1) { const size_t mid = (lo + hi) >> 1; if ((size_t)segs[mid].first <= k) lo = mid; else hi = mid; }
        return lo;
    }
    FR_HD static size_t children(const Seg& S, size_t j, int mode, size_t arity) { return mode == 1 ? 2 : ((j + 1) * arity <= (size_t)S.n_in ? arity : (size_t)S.n_in - j * arity); }
    FR_HD uint64_t position(size_t k) const { return pos0 + (k - (size_t)segs[seg(k)].first); }
    FR_HD size_t total(size_t k) const { const Seg& S = segs[seg(k)]; return 4 + children(S, k - (size_t)S.first, mode, arity) + 1; }
    FR_HD size_t max_total() const { return 4 + (mode == 1 ? 2 : arity) + 1; }
    FR_HD fr_t elem(size_t k, size_t q) const {
        if (q < 2) return q == 0 ? arity_f : level_f;
        const Seg& S = segs[seg(k)]; const size_t j = k - (size_t)S.first;
        if (q < 4) return q == 2 ? fr_from_u64<PF>(pos0 + j) : fr_from_u64<PF>(S.label);
        if (q == 4 + children(S, j, mode, arity)) return fr_one<PF>();
        const size_t c = q - 4;
        if (mode == 1) return c == 0 ? ldg(S.in0 + j) : (S.in1 ? ldg(S.in1 + j) : fr_zero<PF>());
        return ldg(S.in0 + j * arity + c);
    }
};
// The pair leaves of unhashed FRI layers of DIFFERENT lengths in one launch (the ragged commit phase, fri_mixed.hpp): DsBatchPairStream with a segment
// per tree.  Segment s (DsRaggedStream's table type; its in1 is not read) is the layer of one trace: in0_s its n_in_s elements, its label, and `first`,
// the index of its first hash.  Hash k is leaf j = k - first_s of that tree, position j:
//   hash k = hash_with_ds_dynamic([arity, 2^32 - 1, j, label_s] || in0_s[j], in1 ? in1[k / cp_div] : 0 || 1), eager sponge, cap 0
// with in1 ONE array for the launch, indexed by the launch's own hash index k: the next layers of the same trees back to back.  That is exact when
// cp_div divides every n_in_s (then first_s / cp_div is where tree s starts in in1, and k / cp_div never leaves its slice).  in1 == nullptr: zero
// partners (the last layer, fri.rs:266).
struct DsRaggedPairStream {
    typedef DsRaggedStream::Seg Seg;
    fr_t arity_f, level_f; size_t n_seg, n_out, cp_div; const Seg* segs; const fr_t* in1;
    static inline DsRaggedPairStream make(size_t arity, const Seg* segs, size_t n_seg, size_t n_out, const fr_t* in1, size_t cp_div) {
        DsRaggedPairStream D;
        D.arity_f = fr_from_u64<PF>(arity); D.level_f = fr_from_u64<PF>(0xFFFFFFFFu); D.n_seg = n_seg; D.n_out = n_out; D.cp_div = cp_div ? cp_div : 1; D.segs = segs; D.in1 = in1;
        return D;
    }
    FR_HD size_t seg(size_t k) const {                                 // the last segment whose first hash is <= k
        size_t lo = 0, hi = n_seg;
        while (hi - lo > 1) { const size_t mid = (lo + hi) >> 1; if ((size_t)segs[mid].first <= k) lo = mid; else hi = mid; }
        return lo;
    }
    FR_HD uint64_t position(size_t k) const { return k - (size_t)segs[seg(k)].first; }
    FR_HD size_t total(size_t) const { return 7; }
    FR_HD size_t max_total() const { return 7; }
    FR_HD fr_t elem(size_t k, size_t q) const {
        if (q < 2) return q == 0 ? arity_f : level_f;
        if (q == 6) return fr_one<PF>();
        if (q == 5) return in1 ? ldg(in1 + k / cp_div) : fr_zero<PF>();
        const Seg& S = segs[seg(k)]; const size_t j = k - (size_t)S.first;
        return q == 2 ? fr_from_u64<PF>(j) : (q == 3 ? fr_from_u64<PF>(S.label) : ldg(S.in0 + j));
    }
};
// The segment table of one launch, built on the host: add() the participating trees in order, then hand `segs` to the executor's memory.
struct DsRaggedTable {
    std::vector<DsRaggedStream::Seg> segs; size_t n_out = 0;
    void add(int mode, size_t arity, const fr_t* in0, const fr_t* in1, size_t n_in, uint64_t label) {
        segs.push_back(DsRaggedStream::Seg{in0, in1, (uint64_t)n_in, label, (uint64_t)n_out}); n_out += DsRaggedStream::hashes(mode, arity, n_in);
    }
};

// B streaming transcripts (transcript/src/lib.rs:79-101, lazy duplex) advanced in one launch, one workgroup per active instance
// (the batched sum-check provers, sumcheck_batch.hpp).  Instance b keeps state[17 b .. 17 b + 16] and its rate cursor pos[b] in
// device memory between launches; active a runs instance inst[a] (inst == nullptr: inst0 + a).  Active a runs nseg segments: segment
// s = a * nseg + s' absorbs the elements idx[el_off[s] .. el_off[s + 1]) gathered from the pools (an index with bit 31 set reads
// pool1, else pool0), then — every segment but an unfinished last one — permutes and squeezes state[0] into out[s] (a challenge).
//   reset_from  : the active instances a >= reset_from start from Transcript::new's state (zeros, capacity `init_cap`, cursor 0) instead of the
//                 stored one (0: all of them; n_active: none).  The mixed-size provers' joiners are the tail of a launch's active instances.
//   finish_last : 0 leaves the last segment absorbed but not permuted (the cursor then records where the next absorb goes)
struct TrBatchStream {
    fr_t* state; uint32_t* pos; const uint32_t* inst; size_t inst0, n_active, nseg;
    const uint32_t* el_off; const uint32_t* idx; const fr_t* pool0; const fr_t* pool1; fr_t* out;
    fr_t init_cap; size_t reset_from; int finish_last;
    static constexpr uint32_t kPool1 = 0x80000000u;
    FR_HD size_t instance(size_t a) const { return inst ? (size_t)inst[a] : inst0 + a; }
    FR_HD bool resets(size_t a) const { return a >= reset_from; }
    FR_HD bool finishes(size_t s) const { return finish_last || s + 1 < nseg; }
    FR_HD fr_t elem(size_t j) const { const uint32_t x = idx[j]; return x & kPool1 ? ldg(pool1 + (x & ~kPool1)) : ldg(pool0 + x); }
};

// tr_hash_fields_tagged (fri.rs:28-35): the stream prefix || fields || suffix under the capacity FSv1-TRANSCRIPT-INIT (lazy duplex,
// transcript/src/lib.rs:79-101).  Frames (prefix, suffix) per column c < 4; the layout says which sponge reads which frame and fields:
//   Equal        : n sponges of k[0] fields at fields[0] + b * k[0], all under column 0's frame (one tag)
//   Columns      : sponge b < 4 is column b, fields[b] (k[b] of them)
//   BatchColumns : sponge b is column b & 3 of trace b >> 2, its k[b & 3] fields at batch[b] (a device array of device pointers)
//   Ragged       : sponge b is items[b] (a device array): its own frame, fields, length and output slot, so every sponge of a launch may have
//                  another tag and another length.  The kernels of this layout are instantiations of their own (sponge_as<true>(b, &slot), not sponge(b)) and write
//                  digest b to out[items[b].out]; the other layouts keep out[b].  k == 0 is an item like any other: it hashes the frame alone and
//                  its fields pointer (which may be null) is never read.
struct TrStream {
    enum Layout { Equal, Columns, BatchColumns, Ragged };
    struct Item { const fr_t* prefix; const fr_t* suffix; const fr_t* fields; uint32_t np, ns; uint64_t k, out; };
    Layout layout; size_t n;
    const fr_t* prefix[4]; int np[4]; const fr_t* suffix[4]; int ns[4]; const fr_t* fields[4]; size_t k[4];
    const fr_t* const* batch; fr_t cap; const Item* items;
    // n sponges of k fields each under one frame (frame = prefix || suffix, np + ns elements)
    static inline TrStream equal(const fr_t* frame, int np, int ns, const fr_t* fields, size_t k, size_t n, const fr_t& cap) {
        TrStream T{}; T.layout = Equal; T.n = n; T.cap = cap; T.batch = nullptr;
        T.prefix[0] = frame; T.np[0] = np; T.suffix[0] = frame + np; T.ns[0] = ns; T.fields[0] = fields; T.k[0] = k;
        return T;
    }
    // sponge b with its frame and fields resolved: kernels take this once per sponge, outside their absorb loops
    struct Sponge {
        const fr_t* prefix; const fr_t* fields; const fr_t* suffix; size_t np, k, n_total;
        FR_HD size_t total() const { return n_total; }
        FR_HD fr_t elem(size_t q) const { return q < np ? ldg(prefix + q) : (q < np + k ? ldg(fields + (q - np)) : ldg(suffix + (q - np - k))); }
    };
    FR_HD Sponge sponge(size_t b) const {
        const int c = layout == Equal ? 0 : (int)(b & 3);
        const fr_t* f = layout == Equal ? fields[0] + b * k[0] : (layout == Columns ? fields[b] : batch[b]);
        return Sponge{prefix[c], f, suffix[c], (size_t)np[c], k[c], (size_t)np[c] + k[c] + (size_t)ns[c]};
    }
    // the Ragged layout: ONE load of the item per workgroup or lane, then the same view
    FR_HD static Sponge sponge_of(const Item& it) { return Sponge{it.prefix, it.fields, it.suffix, (size_t)it.np, (size_t)it.k, (size_t)it.np + (size_t)it.k + (size_t)it.ns}; }
    template <bool RAGGED> FR_HD Sponge sponge_as(size_t b, size_t* slot) const {
        if (RAGGED) { const Item it = items[b]; *slot = (size_t)it.out; return sponge_of(it); }
        *slot = b; return sponge(b);
    }
};

// The items of a Ragged launch, built once for the device driver (capi_poseidon.hip) and its host twin (hostcheck.cpp): sponge i of the caller
// absorbs frames[i] around fields[i][0 .. k[i]) and writes slot i.  Workgroups are dispatched in index order, so the items go LONGEST FIRST (by
// absorbed length, ties by the caller's index): a long chain never starts behind short ones once a launch exceeds what is resident, and the 64
// lanes of a wave of the lane form get neighbouring lengths.  `out` restores the caller's order.
struct TrFrameRef { const fr_t* frame; int np, ns; };
inline std::vector<size_t> tr_ragged_order(const TrFrameRef* frames, const size_t* k, size_t n) {
    std::vector<size_t> ord(n); std::iota(ord.begin(), ord.end(), (size_t)0);
    std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return (size_t)frames[x].np + k[x] + (size_t)frames[x].ns > (size_t)frames[y].np + k[y] + (size_t)frames[y].ns; });
    return ord;
}
inline std::vector<TrStream::Item> tr_ragged_items(const TrFrameRef* frames, const fr_t* const* fields, const size_t* k, size_t n) {
    const std::vector<size_t> ord = tr_ragged_order(frames, k, n);
    std::vector<TrStream::Item> items(n);
    for (size_t j = 0; j < n; ++j) {
        const size_t i = ord[j]; const TrFrameRef& f = frames[i];
        items[j] = TrStream::Item{f.frame, f.frame + f.np, k[i] ? fields[i] : nullptr, (uint32_t)f.np, (uint32_t)f.ns, (uint64_t)k[i], (uint64_t)i};
    }
    return items;
}
inline TrStream tr_ragged_stream(const TrStream::Item* items, size_t n, const fr_t& cap) {
    TrStream T{}; T.layout = TrStream::Ragged; T.n = n; T.cap = cap; T.batch = nullptr; T.items = items; return T;
}

// hash_leaf_pair(f_i, s_i) (fri.rs:38-44): ONE t = 17 permutation of the template `init` (capi_poseidon.hip ctx_leaf_init)
// with elements 4, 5 = (f[i], s_i), s_i = f_next[i / m] (zero when f_next == nullptr: fri.rs:266).  Elements 0..8 are the absorbed ones,
// 9..15 of the template are zero, element 16 is the capacity.
struct LeafStream {
    const fr_t* init; const fr_t* f; const fr_t* f_next; size_t m, n;
    FR_HD size_t total(size_t) const { return 9; }
    FR_HD fr_t cap() const { return ldg(init + 16); }
    FR_HD fr_t elem(size_t i, size_t q) const {
        if (q == 4) return ldg(f + i);
        if (q == 5) return f_next ? ldg(f_next + i / m) : fr_zero<PF>();
        return ldg(init + q);
    }
};

}  // namespace stark
