// tools/ntt_plan_check.cpp — stand-alone host check of the batched NTT / LDE launch plan (stark_mlwe_amd/csrc/ntt_mixed_plan.hpp): its own main, no
// Python, no GPU; built with AddressSanitizer + UBSan by tools/ntt_plan_sanitize.sh.  Builds both plans and asks ntt_mixed_one_shape about every launch
// for batches of equal lengths (every transform launch must hold, at the pitch of the scratch layout) and of mixed lengths (a launch of two shapes
// must not), with and without a coset, and checks that every range a launch names lies inside the plan's scratch.  Prints one JSON line.
#include <cstdio>
#include <vector>
#include "ntt_mixed_plan.hpp"

using namespace stark;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

// every scratch range of the plan inside [0, scratch_elems); every column index below ncols; tile ranges partition each launch
static void check_bounds(const NttMixedPlan& plan, size_t ncols) {
    for (const NttMixedLaunch& L : plan.launches) {
        uint32_t t = 0;
        for (const NttMixedCol& c : L.cols) {
            CHECK(c.col < ncols && c.first_tile == t);
            const uint64_t len = L.kind == NTT_MIXED_PAD ? c.len : 1ull << L.shapes.at(c.shape).log_n;
            t += L.kind == NTT_MIXED_PAD ? (uint32_t)((c.len - c.first + NTT_PAD_BLOCK - 1) / NTT_PAD_BLOCK) : L.shapes.at(c.shape).tiles;
            const int nz = L.kind == NTT_MIXED_PAD ? -1 : L.shapes.at(c.shape).log_nonzero;       // a pass that skips the padding reads 2^nz elements
            if (c.src.mem == NTT_MEM_SCRATCH) CHECK(c.src.off + (L.kind == NTT_MIXED_PAD ? c.head : nz >= 0 ? 1ull << nz : len) <= plan.scratch_elems);
            if (c.dst.mem == NTT_MEM_SCRATCH) CHECK(c.dst.off + len <= plan.scratch_elems);
        }
        CHECK(t == L.ntiles);
    }
}
// equal: all lengths equal, so every transform launch is one shape at `pitch`; else only launches of one shape record may hold
static int check_plan(const NttMixedPlan& plan, size_t ncols, bool equal, uint64_t pitch) {
    check_bounds(plan, ncols);
    int held = 0;
    for (const NttMixedLaunch& L : plan.launches) {
        NttOneShape S; const bool one = ntt_mixed_one_shape(L, &S);
        held += one;
        if (L.kind == NTT_MIXED_PAD) { CHECK(!one); continue; }
        CHECK(!one || L.shapes.size() == 1);
        if (!equal) continue;
        CHECK(one && L.ntiles == L.cols.size() * L.shapes[0].tiles);
        if (!one) continue;
        for (const NttMixedEnd* E : {&S.src, &S.dst}) {
            if (E->mem != NTT_MEM_SCRATCH) { CHECK(E->off == 0 && E->pitch == 0); continue; }
            CHECK(E->pitch == (L.cols.size() > 1 ? pitch : 0) && E->off + (L.cols.size() - 1) * E->pitch < plan.scratch_elems);
        }
    }
    return held;
}

int main() {
    const NttTileOpts o;
    int plans = 0, held = 0;
    struct Lde { std::vector<size_t> ln; int lb; bool equal; };
    const std::vector<Lde> ldes = {{{8, 8, 8, 8}, 3, true}, {{4, 4, 4}, 1, true}, {{0, 0, 0}, 0, true}, {{0, 0, 0}, 2, true}, {{9, 9, 10}, 2, false},
                                   {{8, 0, 18, 5, 8, 9, 3}, 3, false}, {{}, 3, true}};
    const std::vector<std::vector<size_t>> ntts = {{11, 11, 11}, {5, 12, 3, 12}, {0, 0}, {21, 3, 21}, {}};
    for (int coset = 0; coset < 2; ++coset) {
        for (const Lde& c : ldes) {
            const uint64_t pitch = c.ln.empty() ? 0 : (1ull << (c.ln[0] + c.lb)) + (1ull << c.ln[0]);
            held += check_plan(ntt_mixed_lde_plan(c.ln.data(), c.ln.size(), c.lb, coset != 0, o), c.ln.size(), c.equal, pitch); ++plans;
        }
        for (int inverse = 0; inverse < 2; ++inverse)
            for (const std::vector<size_t>& ln : ntts) {
                bool equal = true; for (size_t l : ln) equal = equal && l == ln[0];
                const NttMixedPlan plan = ntt_mixed_ntt_plan(ln.data(), ln.size(), inverse != 0, coset != 0, o);
                held += check_plan(plan, ln.size(), equal, ln.empty() ? 0 : 1ull << ln[0]); ++plans;
                if (ln == std::vector<size_t>{5, 12, 3, 12}) {       // the strided launch holds caller columns 1 and 3 alone, and is one shape
                    CHECK(plan.launches.size() >= 2 && plan.launches[0].cols.size() == 2 && plan.launches[0].cols[0].col == 1 && plan.launches[0].cols[1].col == 3);
                    CHECK(ntt_mixed_one_shape(plan.launches[0], nullptr));
                }
            }
    }
    std::printf("{\"plans\": %d, \"one_shape_launches\": %d, \"failures\": %d}\n", plans, held, failures);
    return failures ? 1 : 0;
}
