// tools/merkle_climb_check.cpp — stand-alone host check of the Merkle climbs (stark_mlwe_amd/csrc/merkle_batch.hpp): its own main, no Python, no GPU;
// built with AddressSanitizer + UBSan by tools/merkle_climb_sanitize.sh.  Runs merkle_ragged_plan over arity 2, 4, 8, 16 and mixed and equal batches of
// 1 to 6 trees of 1, 2, 15, 16, 17, 32, 33, 256 or 257 leaves and checks that the slices of a level tile its block and that every table's `first` are
// the prefix sums of its hash counts; then runs both climbs over an executor whose blocks have exactly the planned sizes and whose hash_level reads
// every element a hash absorbs and writes every hash, so a slice, a table or a pointer that is off by one is an error of the sanitizer.  One JSON line.
#include <cstdio>
#include <memory>
#include <vector>
#include "merkle_batch.hpp"

using namespace stark;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

struct CheckExec {
    std::vector<std::unique_ptr<fr_t[]>> blocks; std::vector<std::vector<DsRaggedStream::Seg>> tables; size_t launches = 0, hashes = 0;
    int32_t level_block(size_t n_fr, fr_t** out) { blocks.emplace_back(new fr_t[n_fr]()); *out = blocks.back().get(); return 0; }
    int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** x) { tables.push_back(h); *x = tables.back().data(); return 0; }
    template <class DS> int32_t hash_level(const DS& D, fr_t* out) {
        ++launches;
        for (size_t k = 0; k < D.n_out; ++k) {
            fr_t acc = fr_zero<PF>();
            for (size_t q = 0; q < D.total(k); ++q) acc = fr_add<PF>(acc, D.elem(k, q));
            out[k] = acc; ++hashes;
        }
        return 0;
    }
};

static void check_plan(const MerkleRaggedPlan& P, size_t arity, const std::vector<size_t>& n, bool leaf_table) {
    const size_t B = n.size();
    CHECK(P.lens.size() == B && P.at.size() == B && P.block.size() == P.depth && P.tree.size() == P.segs.size());
    for (size_t v = 0; v < P.depth; ++v) {
        size_t o = 0, first = 0, s = P.t0[v];
        for (size_t b = 0; b < B; ++b) {
            if (P.lens[b].size() <= v) continue;
            CHECK(P.at[b][v] == o); o += P.lens[b][v];
            CHECK(P.lens[b][v] == (v ? (P.lens[b][v - 1] + arity - 1) / arity : n[b]));
            if (!v && !leaf_table) continue;
            CHECK(s < P.t0[v] + P.n_seg[v] && s < P.segs.size());
            if (s >= P.segs.size()) return;
            CHECK(P.tree[s] == b && P.segs[s].first == first && P.segs[s].n_in == (v ? P.lens[b][v - 1] : n[b]) && P.segs[s].label == 500 + b);
            first += P.lens[b][v]; ++s;
        }
        CHECK(o == P.block[v] && s == P.t0[v] + P.n_seg[v] && P.n_out[v] == first);
    }
    for (size_t b = 0; b < B; ++b) CHECK(!P.lens[b].empty() && P.lens[b].back() == 1);
}

int main() {
    const size_t lengths[] = {1, 2, 15, 16, 17, 32, 33, 256, 257};
    std::vector<std::vector<size_t>> batches;
    uint64_t x = 0xC11Bu;                                                     // a fixed stream of picks
    for (size_t B = 1; B <= 6; ++B) {
        for (size_t l : lengths) batches.push_back(std::vector<size_t>(B, l));
        for (int r = 0; r < 8; ++r) { std::vector<size_t> n(B); for (size_t& e : n) { x = x * 6364136223846793005ull + 1442695040888963407ull; e = lengths[(x >> 33) % 9]; } batches.push_back(n); }
    }
    size_t plans = 0, launches = 0, hashes = 0;
    for (size_t arity : {2, 4, 8, 16}) for (const std::vector<size_t>& n : batches) {
        const size_t B = n.size(); std::vector<uint64_t> labels(B); for (size_t b = 0; b < B; ++b) labels[b] = 500 + b;
        std::vector<std::vector<fr_t>> leaves(B); std::vector<const fr_t*> lp(B);
        for (size_t b = 0; b < B; ++b) { leaves[b].assign(n[b], fr_one<PF>()); lp[b] = leaves[b].data(); }
        for (int leaf_table = 0; leaf_table < 2; ++leaf_table) { check_plan(merkle_ragged_plan(arity, B, n.data(), labels.data(), leaf_table != 0), arity, n, leaf_table != 0); ++plans; }
        {   // the ragged climb, level 0 read in place, the top level into the caller's slots (as the sum-check commit runs it)
            CheckExec X; MerkleRaggedPlan P = merkle_ragged_plan(arity, B, n.data(), labels.data(), false); std::vector<fr_t*> base;
            std::unique_ptr<fr_t[]> top(new fr_t[P.depth > 1 ? P.block[P.depth - 1] : 1]());
            CHECK(merkle_climb_ragged(X, P, lp.data(), top.get(), base, [](const DsRaggedStream::Seg*) { return 0; }) == 0);
            CHECK(X.launches == (P.depth ? P.depth - 1 : 0) && X.tables.size() <= 1 && (P.depth < 2 || base[P.depth - 1] == top.get()));
            launches += X.launches; hashes += X.hashes;
        }
        {   // the mixed build: pair leaves into a block of its own, then the climb (as merkle_build_mixed_batch runs it)
            std::vector<std::vector<size_t>> lens, at; std::vector<fr_t*> base;
            struct Copy : CheckExec { int32_t copy_ragged(const DsRaggedStream& D, fr_t* dst) { for (size_t i = 0; i < D.n_out; ++i) { const DsRaggedStream::Seg& S = D.segs[D.seg(i)]; dst[i] = S.in0[i - S.first]; } return 0; } } XC;
            for (int pairs = 0; pairs < 2; ++pairs) {
                std::vector<const fr_t*> cp(lp); cp.back() = nullptr;
                CHECK(merkle_build_mixed_batch(XC, arity, B, labels.data(), lp.data(), n.data(), pairs, pairs ? cp.data() : nullptr, lens, at, base) == 0);
                for (size_t b = 0; b < B; ++b) CHECK(lens[b].front() == n[b] && lens[b].back() == 1);
            }
            launches += XC.launches; hashes += XC.hashes;
        }
        bool equal = true; for (size_t e : n) equal = equal && e == n[0];
        if (equal) {   // the same-shape climb at a pitch and behind a pointer table, with and without top slots
            for (int ptrs = 0; ptrs < 2; ++ptrs) for (int with_top = 0; with_top < 2; ++with_top) {
                CheckExec X; std::vector<size_t> lens; std::vector<fr_t*> base; std::vector<fr_t> in(B * n[0], fr_one<PF>()); std::unique_ptr<fr_t[]> top(new fr_t[B]());
                CHECK(merkle_climb(X, arity, B, labels.data(), ptrs ? lp.data() : nullptr, ptrs ? nullptr : in.data(), n[0], with_top ? top.get() : nullptr, lens, base) == 0);
                CHECK(lens == merkle_level_lens(n[0], arity) && X.launches == lens.size() - 1 && X.blocks.size() == (lens.size() > 1 ? lens.size() - 1 - with_top : 0));
                CHECK(!with_top || lens.size() < 2 || base.back() == top.get());
                launches += X.launches; hashes += X.hashes;
            }
        }
    }
    std::printf("{\"plans\": %zu, \"launches\": %zu, \"hashes\": %zu, \"failures\": %d}\n", plans, launches, hashes, failures);
    return failures ? 1 : 0;
}
