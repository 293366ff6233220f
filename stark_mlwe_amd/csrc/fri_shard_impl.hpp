// stark_mlwe_amd/csrc/fri_shard_impl.hpp — one trace block-sharded over the ranks of the context's communicator: the commit phase
// (fri.rs:231-312), the query phase (fri.rs:355-466, 613-640) and build_f0 (fri.rs:535-569) as ONE C-ABI call each — dist.py's DistProver
// in C++, so that a host without Python (the reference's Rust process) drives a multi-GPU prove with one call per prove.
// Included at the end of capi_fri.hip (it uses that file's fold / challenge / merge / query helpers).
//
// Structure (as the sharded LDE in capi_ntt.hip): a shard PLAN that every rank derives identically from (n0, schedule, W), per-rank STATE,
// and numbered PHASES of local work between two collectives.  The collectives go through `ShardColl` (shard_coll.hpp): the communicator's
// one local rank, or W virtual ranks emulated on one GPU.  One driver per operation (shard_build, shard_prove) runs for the local ranks of
// either; each real entry point and its diagnostic twin only build the ShardColl, so the W > 1 index arithmetic the emulation tests reach is
// what runs with RCCL.
//
// Rules that keep the collectives safe: every argument check happens before the first collective; the first collective of each entry point
// all-gathers a fixed-size header (n0, L, schedule, r, seed_z, f0 given) and every rank refuses when any two headers differ; the sequence
// of collectives depends only on that header, never on local data.

#include <array>
#include "shard_coll.hpp"

// ---- the plan: which layers stay block-local, and where each lower tree stops ------------------------------------------------------------
struct FriShardPlan {
    int W = 1; size_t n0 = 0, L = 0, T = 0;          // T: the first replicated layer (L + 1: every layer sharded)
    std::vector<size_t> sched, n, arity, stop;       // stop[l]: local length of the level at which a sharded layer's lower tree stops (1: replicated)
    std::vector<char> sharded;
    size_t m(size_t l) const { return l < L ? sched[l] : 1; }
    size_t here(size_t l) const { return sharded[l] ? n[l] / W : n[l]; }   // elements of layer l one rank holds
    size_t zoff(size_t l) const { size_t o = 0; for (size_t j = 0; j < l; ++j) o += sched[j]; return o; }   // layer l's z-powers in the fold table
};
// DistProver._shardable and sharded_stop_len (dist.py): a layer stays sharded while the previous one was, its arity is hashed, and the
// local block holds whole Merkle groups and whole fold groups; the lower tree climbs while the local level length is a multiple of the arity.
static bool fri_shard_plan(size_t n0, const size_t* sched, size_t L, int W, FriShardPlan& P, std::string& err) {
    if (W < 1 || (W & (W - 1))) { err = "the number of ranks must be a power of two"; return false; }
    if (!n0) { err = "empty layer"; return false; }
    if (n0 % (size_t)W) { err = "n0 must divide over the ranks"; return false; }
    if (L && !sched) { err = "schedule"; return false; }
    P = FriShardPlan(); P.W = W; P.n0 = n0; P.L = L; P.sched.assign(sched, sched + L);
    { const LayerShape sh = fri_layers(n0, sched, L, P.n, P.arity);                      // arity 1 passes: merkle_build_on refuses it (STARK_ERR_UNSUPPORTED)
      if (sh == LayerShape::empty_layer || sh == LayerShape::not_dividing) { err = layer_shape_text(sh); return false; } }
    bool prev = true; P.T = L + 1;
    for (size_t l = 0; l <= L; ++l) {
        const size_t m = P.m(l), a = P.arity[l];
        bool now = prev && hashed_arity(a) && P.n[l] % (size_t)W == 0;
        if (now) { const size_t nl = P.n[l] / W; now = nl % a == 0 && (l == L || nl % m == 0); }
        if (!now && P.T == L + 1) P.T = l;
        P.sharded.push_back(now ? 1 : 0); prev = now;
        size_t s = 1;
        if (now) { s = P.n[l] / W; while (s > 1 && s % a == 0) s /= a; }
        P.stop.push_back(s);
    }
    return true;
}

// ---- per-rank state -----------------------------------------------------------------------------------------------------------------------
struct FriShardRank {
    stark_ctx* ctx = nullptr; int rank = 0;
    std::vector<DevBuf> f;                    // layer l: this rank's block (sharded) or the whole layer (replicated); pooled
    std::vector<std::unique_ptr<stark_tree>> tree, top;   // sharded: the levels below the crossing level / the top built from the all-gathered level; replicated: the tree / null
    DevBuf zp, coll;                          // fold z-powers; the buffer of the collective in flight (in place: this rank's chunk sits at rank * chunk)
    std::vector<fr_t> roots;                  // L+1 roots, identical on every rank
    std::vector<fr_t> table;                  // query phase: the all-reduced value table, downloaded
};
static int32_t coll_alloc(stark_ctx* ctx, FriShardRank& K, size_t bytes) { STARK_HIP(ctx, K.coll.alloc(ctx, bytes)); return STARK_OK; }   // alloc releases the previous buffer first

// ---- collective 0 of every entry point: all ranks hold the same arguments ------------------------------------------------------------------
static constexpr size_t SHARD_HDR_WORDS = 72;         // magic, n0, L, r, seed_z, f0 given, schedule[0..64) (a dividing schedule has L <= 63), pad
static int32_t shard_header_agree(const ShardColl& C, std::vector<FriShardRank>& K, const FriShardPlan& P, size_t r, uint64_t seed_z, int f0_given) {
    stark_ctx* ctx = C.ctx;
    std::vector<uint64_t> h(SHARD_HDR_WORDS, 0);
    h[0] = 0x5348415244465249ull; h[1] = P.n0; h[2] = P.L; h[3] = r; h[4] = seed_z; h[5] = (uint64_t)f0_given;
    for (size_t l = 0; l < P.L && l < 64; ++l) h[6 + l] = P.sched[l];
    const size_t bytes = SHARD_HDR_WORDS * 8;
    std::vector<void*> buf;
    for (auto& k : K) {
        STARK_TRY(coll_alloc(ctx, k, (size_t)C.W * bytes));
        STARK_TRY(ctx_upload_staged(ctx, (char*)k.coll.p + (size_t)k.rank * bytes, h.data(), bytes));
        buf.push_back(k.coll.p);
    }
    STARK_TRY(C.all_gather(buf, bytes));
    std::vector<uint64_t> all((size_t)C.W * SHARD_HDR_WORDS);
    bool same = true;
    for (auto& k : K) {
        STARK_HIP(ctx, hipMemcpyAsync(all.data(), k.coll.p, (size_t)C.W * bytes, hipMemcpyDeviceToHost, ctx->stream));
        STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t q = 0; q < (size_t)C.W; ++q) if (memcmp(all.data() + q * SHARD_HDR_WORDS, h.data(), bytes) != 0) same = false;
        k.coll.reset();
    }
    if (!same) return ctx->fail(STARK_ERR_INVALID_ARG, "sharded FRI: the ranks disagree on (n0, L, schedule, r, seed_z, f0)");
    return STARK_OK;
}

// ---- build_f0 (fri.rs:535-569), sharded: column c is gathered to rank c mod W, the four digests are all-reduced, the merge is block-local ------
// cols[i][c]: column c of local rank i (its block of n0 / W rows); f0[i]: its block of f0.
static int32_t shard_build_f0(const ShardColl& C, std::vector<FriShardRank>& K, size_t n0, const std::vector<std::array<const fr_t*, 4>>& cols,
                              const std::vector<fr_t*>& f0) {
    stark_ctx* ctx = C.ctx; const int W = C.W; const size_t nl = n0 / W;
    static const char* const TAGS[4] = {"ALI/A", "ALI/S", "ALI/E", "ALI/T"};                                          // fri.rs:551-554
    // collectives 1-4: every column to the rank that runs its serial sponge
    std::vector<DevBuf> whole(4 * K.size());
    for (int c = 0; c < 4; ++c) {
        const int root = c % W; void* recv = nullptr; std::vector<const void*> send;
        for (size_t i = 0; i < K.size(); ++i) {
            send.push_back(cols[i][c]);
            if (K[i].rank == root) { STARK_HIP(ctx, whole[4 * i + c].alloc(ctx, n0 * sizeof(fr_t))); recv = whole[4 * i + c].p; }
        }
        STARK_TRY(C.gather(send, recv, nl * sizeof(fr_t), root));
    }
    // phase: the digests of the owned columns (one launch of four concurrent chains; a rank that owns fewer repeats its first column), in
    // rows c of a zeroed 4 x 4-word table
    std::vector<DevBuf> dig(K.size()); std::vector<void*> buf;
    for (size_t i = 0; i < K.size(); ++i) {
        STARK_HIP(ctx, dig[i].alloc(ctx, 8 * sizeof(fr_t)));          // rows 0..3: the table; 4..7: the four chains' outputs
        STARK_HIP(ctx, hipMemsetAsync(dig[i].p, 0, 4 * sizeof(fr_t), ctx->stream));
        std::vector<int> own; for (int c = 0; c < 4; ++c) if (c % W == K[i].rank) own.push_back(c);
        if (!own.empty()) {
            const char* tags[4]; const fr_t* cp[4];
            for (int j = 0; j < 4; ++j) { const int c = own[j < (int)own.size() ? j : 0]; tags[j] = TAGS[c]; cp[j] = whole[4 * i + c].fr(); }
            STARK_TRY(tr_hash_columns4_dev(ctx, tags, cp, n0, dig[i].fr() + 4));
            for (size_t j = 0; j < own.size(); ++j) STARK_HIP(ctx, hipMemcpyAsync(dig[i].fr() + own[j], dig[i].fr() + 4 + j, sizeof(fr_t), hipMemcpyDeviceToDevice, ctx->stream));
        }
        buf.push_back(dig[i].p);
    }
    // collective 5: every row is non-zero on exactly one rank, so the SUM is the selection
    STARK_TRY(C.all_reduce(buf, 16));
    for (auto& w : whole) w.reset();
    // phase: (seed, z, beta) from the four digests, then the block-local merge at global positions
    const fr_t omega = fr_root_of_unity<PallasFr>((unsigned)ilog2(n0));                                             // FriDomain::new_radix2(n0).omega, fri.rs:53-56
    for (size_t i = 0; i < K.size(); ++i) {
        fr_t h[4]; STARK_HIP(ctx, hipMemcpyAsync(h, dig[i].p, 4 * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        fr_t seed_f, z, beta; STARK_TRY(ali_challenges(ctx, h, n0, &seed_f, &z, &beta));
        STARK_TRY(ali_merge_dev_impl(ctx, cols[i][0], cols[i][1], cols[i][2], cols[i][3], nullptr, host::h_zero(), omega, z, nl, f0[i], nullptr,
                                     (uint64_t)K[i].rank * nl, n0, false));
    }
    return STARK_OK;
}
// ---- the commit phase (fri.rs:231-312; DistProver.commit) ------------------------------------------------------------------------------------
// phase 0: layer buffers, the copy of f0 and the block-local folds; the transition layer T is folded straight into this rank's chunk of the
//          whole layer.  Collective 6: all-gather of layer T (in place).
// phase 1: the replicated folds; leaf hashes and lower trees of the sharded layers (global DS positions), whole trees of the replicated ones;
//          every sharded layer's crossing level into this rank's chunk of one buffer.  Collective 7: ONE all-gather of those levels.
// phase 2: the tops of the sharded layers, identical on every rank; the L+1 roots.
static int32_t shard_commit_phase(stark_ctx* ctx, const FriShardPlan& P, FriShardRank& K, int phase, const fr_t* f0_local, const std::vector<fr_t>& z,
                                  const std::vector<stark_params*>& mps, size_t& top_words) {
    const size_t L = P.L, W = P.W, q = K.rank; hipStream_t st = ctx->stream;
    if (phase == 0) {
        K.ctx = ctx; K.f.clear(); K.f.resize(L + 1); K.tree.clear(); K.tree.resize(L + 1); K.top.clear(); K.top.resize(L + 1);
        for (size_t l = 0; l <= L; ++l) STARK_TRY(K.f[l].take(ctx, P.here(l) * sizeof(fr_t)));
        if (L) STARK_HIP(ctx, K.zp.alloc(ctx, P.zoff(L) * sizeof(fr_t)));
        const size_t nl0 = P.n0 / W;
        STARK_HIP(ctx, hipMemcpyAsync(P.T == 0 ? K.f[0].fr() + q * nl0 : K.f[0].fr(), f0_local, nl0 * sizeof(fr_t), hipMemcpyDeviceToDevice, st));
        for (size_t l = 0; l < std::min(P.T, L); ++l) {          // sharded -> sharded, or the last sharded layer into its chunk of the whole layer T
            STARK_TRY(zpows_launch(ctx, st, z[l], P.sched[l], K.zp.fr() + P.zoff(l)));
            fr_t* dst = P.sharded[l + 1] ? K.f[l + 1].fr() : K.f[l + 1].fr() + q * (P.n[l + 1] / W);
            STARK_TRY(fold_launch(ctx, st, K.f[l].fr(), P.here(l), K.zp.fr() + P.zoff(l), P.sched[l], dst));
        }
        return STARK_OK;
    }
    if (phase == 1) {
        for (size_t l = P.T; l < L; ++l) {                        // replicated folds (whole layers, the same on every rank)
            STARK_TRY(zpows_launch(ctx, st, z[l], P.sched[l], K.zp.fr() + P.zoff(l)));
            STARK_TRY(fold_launch(ctx, st, K.f[l].fr(), P.n[l], K.zp.fr() + P.zoff(l), P.sched[l], K.f[l + 1].fr()));
        }
        top_words = 0; for (size_t l = 0; l <= L; ++l) if (P.sharded[l]) top_words += P.stop[l];
        if (top_words) STARK_TRY(coll_alloc(ctx, K, W * top_words * sizeof(fr_t)));
        size_t toff = 0;
        for (size_t l = 0; l <= L; ++l) {                         // a sharded layer: its lower tree at global DS positions; a replicated one: the whole tree
            const bool sh = P.sharded[l]; const size_t nl = P.here(l), m = P.m(l);
            const fr_t* f_next = l == L ? nullptr : !sh || P.sharded[l + 1] ? K.f[l + 1].fr() : K.f[l + 1].fr() + q * (nl / m);    // this block's parents, fri.rs:283
            STARK_TRY(commit_layer_on(ctx, st, mps[l], P.arity[l], l, K.f[l].fr(), f_next, nl, m, sh ? q * nl : 0, sh ? P.stop[l] : 0, K.tree[l]));
            if (!sh) continue;
            const stark_tree* T = K.tree[l].get();
            if (T->lens.back() != P.stop[l]) return ctx->fail(STARK_ERR_INVALID_ARG, "sharded FRI: lower tree stopped at an unplanned level");
            STARK_HIP(ctx, hipMemcpyAsync(K.coll.fr() + q * top_words + toff, T->levels.back(), P.stop[l] * sizeof(fr_t), hipMemcpyDeviceToDevice, st));
            toff += P.stop[l];
        }
        return STARK_OK;
    }
    // phase 2
    size_t toff = 0;
    K.roots.assign(L + 1, host::h_zero());
    for (size_t l = 0; l <= L; ++l) {
        if (P.sharded[l]) {
            const size_t s = P.stop[l], nin = W * s;
            DevBuf in; STARK_TRY(in.take(ctx, nin * sizeof(fr_t)));
            if (hipMemcpy2DAsync(in.p, s * sizeof(fr_t), K.coll.fr() + toff, top_words * sizeof(fr_t), s * sizeof(fr_t), W, hipMemcpyDeviceToDevice, st) != hipSuccess)
                return ctx->fail(STARK_ERR_HIP, "sharded FRI: unpack the crossing level");
            const uint32_t lv0 = (uint32_t)(K.tree[l]->levels.size() - 1);
            STARK_TRY(merkle_build_on(ctx, st, mps[l], P.arity[l], (uint64_t)l, nullptr, nin, 0, nullptr, 1, 0, lv0, 1, std::move(in), K.top[l]));
            toff += s;
        }
        const stark_tree* T = (P.sharded[l] ? K.top[l] : K.tree[l]).get();
        if (T->lens.back() != 1) return ctx->fail(STARK_ERR_INVALID_ARG, "sharded FRI: a tree without a root");
        STARK_HIP(ctx, hipMemcpyAsync(&K.roots[l], T->levels.back(), sizeof(fr_t), hipMemcpyDeviceToHost, st));
    }
    K.coll.reset();
    return STARK_OK;
}
static int32_t shard_commit(const ShardColl& C, const FriShardPlan& P, std::vector<FriShardRank>& K, const std::vector<const fr_t*>& f0_local, uint64_t seed_z) {
    stark_ctx* ctx = C.ctx; const size_t L = P.L;
    std::vector<stark_params*> mps; std::vector<fr_t> z; STARK_TRY(fri_prelude(ctx, P.n, P.arity, seed_z, mps, z));
    size_t top_words = 0;
    for (size_t i = 0; i < K.size(); ++i) STARK_TRY(shard_commit_phase(ctx, P, K[i], 0, f0_local[i], z, mps, top_words));
    if (P.T <= L) {                                                                        // collective 6: the first replicated layer
        std::vector<void*> buf; for (auto& k : K) buf.push_back(k.f[P.T].p);
        STARK_TRY(C.all_gather(buf, P.n[P.T] / P.W * sizeof(fr_t)));
    }
    for (size_t i = 0; i < K.size(); ++i) STARK_TRY(shard_commit_phase(ctx, P, K[i], 1, f0_local[i], z, mps, top_words));
    if (top_words) {                                                                       // collective 7: the crossing levels of every sharded layer
        std::vector<void*> buf; for (auto& k : K) buf.push_back(k.coll.p);
        STARK_TRY(C.all_gather(buf, top_words * sizeof(fr_t)));
    }
    for (size_t i = 0; i < K.size(); ++i) STARK_TRY(shard_commit_phase(ctx, P, K[i], 2, f0_local[i], z, mps, top_words));
    STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));                                     // the roots are on the host
    return STARK_OK;
}

// ---- the query phase (fri.rs:355-466, 613-640; DistProver.queries) ------------------------------------------------------------------------
// phase 3: the plan from the roots (the same on every rank); this rank's requests into their rows of a zeroed nreq x 4 table, one launch.
// Collective 8: all-reduce SUM.  Phase 4: one download, then assemble_proof (the same canonical bytes on every rank).
static int32_t shard_query_fill(stark_ctx* ctx, const FriShardPlan& P, FriShardRank& K, const FriPlan& plan) {
    const size_t nreq = plan.req.size();
    STARK_TRY(coll_alloc(ctx, K, std::max<size_t>(nreq, 1) * sizeof(fr_t)));
    STARK_HIP(ctx, hipMemsetAsync(K.coll.p, 0, nreq * sizeof(fr_t), ctx->stream));
    // a value of a sharded layer or of a lower tree is owned by the rank whose block holds it, any other (replicated layer, tree top) by rank 0
    struct FriOpening { const fr_t* src; size_t len; uint64_t owner, index; };
    auto resolve = [&](const FriRequest& r, FriOpening& o) -> int32_t {
        if (r.which > P.L) return ctx->fail(STARK_ERR_INVALID_ARG, "query phase: layer out of range");
        const size_t l = r.which;
        if (r.kind == 0) {
            o = {K.f[l].fr(), P.here(l), 0, r.index};
            if (P.sharded[l]) { const uint64_t nl = P.n[l] / P.W; o.owner = r.index / nl; o.index = r.index % nl; }
            return STARK_OK;
        }
        const stark_tree* T = K.tree[l].get(); const uint32_t nlev = (uint32_t)T->levels.size();
        if (P.sharded[l] && r.level + 1 < nlev) { const uint64_t ln = T->lens[r.level]; o = {T->levels[r.level], T->lens[r.level], r.index / ln, r.index % ln}; }
        else if (P.sharded[l]) {
            const stark_tree* U = K.top[l].get(); const uint32_t v = r.level - (nlev - 1);
            if (v >= U->levels.size()) return ctx->fail(STARK_ERR_INVALID_ARG, "query phase: tree level out of range");
            o = {U->levels[v], U->lens[v], 0, r.index};
        } else {
            if (r.level >= nlev) return ctx->fail(STARK_ERR_INVALID_ARG, "query phase: tree level out of range");
            o = {T->levels[r.level], T->lens[r.level], 0, r.index};
        }
        return STARK_OK;
    };
    MerkleGatherList G;                                                                    // the rows of the other ranks stay zero for the all-reduce
    for (size_t i = 0; i < nreq; ++i) {
        FriOpening o; STARK_TRY(resolve(plan.req[i], o));
        if (o.owner == (uint64_t)K.rank) STARK_TRY(add_opening(ctx, G, o.src, o.len, o.index, i));
    }
    return gather_rows(ctx, G, K.coll.fr(), nullptr);
}
static int32_t shard_queries(const ShardColl& C, const FriShardPlan& P, std::vector<FriShardRank>& K, size_t r, std::vector<std::unique_ptr<stark_proof>>& out) {
    stark_ctx* ctx = C.ctx;
    DeviceHasher H0(ctx); MemoHasher H(H0);
    FriPlan plan; STARK_TRY(make_query_plan(ctx, plan, P.n0, P.sched.data(), P.L, K[0].roots.data(), r, H));
    const size_t nreq = plan.req.size();
    std::vector<void*> buf;
    for (auto& k : K) {
        if (memcmp(k.roots.data(), K[0].roots.data(), k.roots.size() * sizeof(fr_t)) != 0) return ctx->fail(STARK_ERR_INVALID_ARG, "sharded FRI: virtual ranks hold different roots");
        STARK_TRY(shard_query_fill(ctx, P, k, plan)); buf.push_back(k.coll.p);
    }
    STARK_TRY(C.all_reduce(buf, nreq * 4));                                                                // collective 8
    for (auto& k : K) {
        k.table.assign(nreq, host::h_zero());
        if (nreq) STARK_HIP(ctx, hipMemcpyAsync(k.table.data(), k.coll.p, nreq * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& k : K) {
        k.coll.reset();
        out.emplace_back(new stark_proof());
        STARK_TRY(assemble_from_values(ctx, plan.shape, r, H, k.table.data(), nreq, out.back().get()));
    }
    return STARK_OK;
}

// ---- the drivers: one per operation, for the local ranks of a ShardColl -------------------------------------------------------------------
// Array arguments are this rank's blocks, or the whole arrays when C is emulated (ShardColl::block).  Every argument check runs before the
// first collective.
static int32_t shard_args(stark_ctx* ctx, int W, size_t n0, const size_t* sched, size_t L, FriShardPlan& P) {
    std::string err;
    if (!fri_shard_plan(n0, sched, L, W, P, err)) return ctx->fail(STARK_ERR_INVALID_ARG, "sharded FRI: " + err);
    return STARK_OK;
}
static void shard_ranks(const ShardColl& C, std::vector<FriShardRank>& K) {
    K = std::vector<FriShardRank>(C.local());
    for (size_t i = 0; i < K.size(); ++i) { K[i].ctx = C.ctx; K[i].rank = C.rank(i); }
}
// the commit phase: P and K (one state per local rank) hold the result
static int32_t shard_build(const ShardColl& C, const fr_t* f0, size_t n0, const size_t* sched, size_t L, uint64_t seed_z, FriShardPlan& P, std::vector<FriShardRank>& K) {
    STARK_TRY(shard_args(C.ctx, C.W, n0, sched, L, P));
    shard_ranks(C, K);
    std::vector<const fr_t*> f0s; for (size_t i = 0; i < K.size(); ++i) f0s.push_back(f0 + C.block(i) * (n0 / C.W));
    int32_t rc = shard_header_agree(C, K, P, 0, seed_z, 1);
    if (rc == STARK_OK) rc = shard_commit(C, P, K, f0s, seed_z);
    if (rc) (void)hipStreamSynchronize(C.ctx->stream);                                     // before the caller frees the state
    return rc;
}
// the prove, from f0 or from the four columns: out[i] receives local rank i's proof (the same bytes on every rank)
static int32_t shard_prove(const ShardColl& C, const fr_t* a, const fr_t* s, const fr_t* e, const fr_t* t, const fr_t* f0_opt, size_t n0, const size_t* sched, size_t L,
                           size_t r, uint64_t seed_z, stark_proof** out) {
    stark_ctx* ctx = C.ctx;
    FriShardPlan P; STARK_TRY(shard_args(ctx, C.W, n0, sched, L, P));
    if (!is_pow2(n0) || n0 <= 1) return ctx->fail(STARK_ERR_INVALID_ARG, "n0 must be a power of two (radix-2 domain)");
    if (!r) return ctx->fail(STARK_ERR_INVALID_ARG, "r >= 1");
    const size_t nl = n0 / C.W;
    for (size_t i = 0; i < C.local(); ++i) out[i] = nullptr;
    const auto t0 = Clock::now();
    std::vector<FriShardRank> K; shard_ranks(C, K);
    STARK_TRY(shard_header_agree(C, K, P, r, seed_z, f0_opt ? 1 : 0));
    DevBuf f0buf; std::vector<const fr_t*> f0;
    if (f0_opt) { for (size_t i = 0; i < K.size(); ++i) f0.push_back(f0_opt + C.block(i) * nl); }
    else {
        STARK_HIP(ctx, f0buf.alloc(ctx, K.size() * nl * sizeof(fr_t)));
        std::vector<std::array<const fr_t*, 4>> cols; std::vector<fr_t*> dst;
        for (size_t i = 0; i < K.size(); ++i) {
            const size_t o = C.block(i) * nl;
            cols.push_back({a + o, s + o, e + o, t + o}); dst.push_back(f0buf.fr() + i * nl); f0.push_back(dst.back());
        }
        STARK_TRY(shard_build_f0(C, K, n0, cols, dst));
    }
    STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const auto t1 = Clock::now();
    STARK_TRY(shard_commit(C, P, K, f0, seed_z));
    const auto t2 = Clock::now();
    std::vector<std::unique_ptr<stark_proof>> pf; STARK_TRY(shard_queries(C, P, K, r, pf));
    const auto t3 = Clock::now();
    for (auto& p : pf) { p->ms[0] = ms_between(t0, t1); p->ms[1] = ms_between(t1, t2); p->ms[2] = ms_between(t2, t3); }
    hand_out(pf, out); return STARK_OK;
}

struct stark_fri_shard {
    CtxRef ref_;
    ShardColl C; uint64_t seed_z = 0;                        // the collective of the build, which the query phase reuses
    FriShardPlan P; std::vector<FriShardRank> K;             // K: the one local rank
    stark_fri_shard(stark_ctx* ctx, uint64_t z) : C(ShardColl::real(ctx)), seed_z(z) { ref_.bind(ctx); }
};

extern "C" {

int32_t stark_fri_shard_layout(size_t n0, const size_t* schedule, size_t L, int32_t nranks, int32_t* sharded, size_t* stop_len) {
    if (!sharded || !stop_len || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    FriShardPlan P; std::string err;
    if (!fri_shard_plan(n0, schedule, L, nranks, P, err)) return STARK_ERR_INVALID_ARG;
    for (size_t l = 0; l <= L; ++l) { sharded[l] = P.sharded[l]; stop_len[l] = P.stop[l]; }
    return STARK_OK;
}
int32_t stark_fri_build_sharded_dev(stark_ctx_t* ctx, const uint64_t* f0_block, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, stark_fri_shard_t** out) {
    if (!ctx || !f0_block || !out || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    std::unique_ptr<stark_fri_shard> S(new stark_fri_shard(ctx, seed_z));
    STARK_TRY(shard_build(S->C, as_fr(f0_block), n0, schedule, L, seed_z, S->P, S->K));
    *out = S.release(); return STARK_OK;
}
int32_t stark_fri_shard_num_layers(stark_fri_shard_t* h) { return h ? (int32_t)(h->P.L + 1) : STARK_ERR_INVALID_ARG; }
int32_t stark_fri_shard_root(stark_fri_shard_t* h, int32_t l, uint64_t* out4) {
    if (!h || !out4 || l < 0 || (size_t)l > h->P.L) return STARK_ERR_INVALID_ARG;
    store_fr(out4, h->K[0].roots[l]); return STARK_OK;
}
int32_t stark_fri_shard_is_sharded(stark_fri_shard_t* h, int32_t l) { return (h && l >= 0 && (size_t)l <= h->P.L) ? (int32_t)h->P.sharded[l] : STARK_ERR_INVALID_ARG; }
int32_t stark_fri_shard_free(stark_fri_shard_t* h) { if (!h) return STARK_ERR_INVALID_ARG; delete h; return STARK_OK; }   // layers and levels return to the pool
int32_t stark_fri_shard_prove_queries(stark_fri_shard_t* h, size_t r, stark_proof_t** out) {
    if (!h || !out) return STARK_ERR_INVALID_ARG;
    stark_ctx* ctx = h->C.ctx; STARK_TRY(ctx_enter(ctx));
    if (!r) return ctx->fail(STARK_ERR_INVALID_ARG, "r >= 1");
    STARK_TRY(shard_header_agree(h->C, h->K, h->P, r, h->seed_z, 1));
    std::vector<std::unique_ptr<stark_proof>> pf; STARK_TRY(shard_queries(h->C, h->P, h->K, r, pf));
    *out = pf[0].release(); return STARK_OK;
}
int32_t stark_deep_fri_prove_sharded_dev(stark_ctx_t* ctx, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t, const uint64_t* f0_opt, size_t n0,
                                         const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out) {
    if (!ctx || !out || (!schedule && L) || (!f0_opt && (!a || !s || !e || !t))) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return shard_prove(ShardColl::real(ctx), as_fr(a), as_fr(s), as_fr(e), as_fr(t), as_fr(f0_opt), n0, schedule, L, r, seed_z, out);
}

// Diagnostic twins: `nranks` virtual ranks on this one GPU, the same drivers, every collective as device copies.
int32_t stark_diag_fri_build_sharded_emulated_dev(stark_ctx_t* ctx, int32_t nranks, const uint64_t* f0_whole, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z,
                                                  uint64_t* roots_out) {
    if (!ctx || !f0_whole || !roots_out || (!schedule && L)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    FriShardPlan P; std::vector<FriShardRank> K;
    STARK_TRY(shard_build(ShardColl::emulate(ctx, nranks), as_fr(f0_whole), n0, schedule, L, seed_z, P, K));
    for (size_t q = 0; q < K.size(); ++q) for (size_t l = 0; l <= L; ++l) store_fr(roots_out + (q * (L + 1) + l) * 4, K[q].roots[l]);
    return STARK_OK;
}
int32_t stark_diag_deep_fri_prove_sharded_emulated_dev(stark_ctx_t* ctx, int32_t nranks, const uint64_t* a, const uint64_t* s, const uint64_t* e, const uint64_t* t,
                                                       const uint64_t* f0_opt, size_t n0, const size_t* schedule, size_t L, size_t r, uint64_t seed_z, stark_proof_t** out) {
    if (!ctx || !out || (!schedule && L) || (!f0_opt && (!a || !s || !e || !t))) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return shard_prove(ShardColl::emulate(ctx, nranks), as_fr(a), as_fr(s), as_fr(e), as_fr(t), as_fr(f0_opt), n0, schedule, L, r, seed_z, out);
}

}  // extern "C"
