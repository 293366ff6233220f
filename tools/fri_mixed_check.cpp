// tools/fri_mixed_check.cpp — stand-alone host check of the ragged commit phase (stark_mlwe_amd/csrc/fri_mixed.hpp) and of the classes and passes of the
// mixed prove (fri_plan.hpp): its own main, no Python, no GPU; built with AddressSanitizer + UBSan by tools/fri_mixed_sanitize.sh.  Over the twelve
// traces of tests/fri_mixed_cases.py it checks mixed_prove_classes and mixed_prove_passes, then runs FriMixedCommit on every pass of every class (whole
// classes, the passes under 5000 rows, every class reversed, every trace alone) over an executor whose blocks have exactly the sizes the driver asks for
// and whose steps read every element they are given and write every element they owe: a slice, a segment table, a partner index or a root pointer that is
// off by one is an error of the sanitizer.  Checked by value: the layout invariant, the fold runs, the tree shapes, where every root comes from.  One JSON line.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "fri_mixed.hpp"

using namespace stark;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

struct Trace { size_t n0; std::vector<size_t> sched; size_t r; };
static const std::vector<Trace> kTraces = {
    {1 << 6, {4, 2}, 4}, {1 << 10, {16, 8}, 8}, {1 << 3, {4, 2}, 4}, {1 << 7, {128}, 4}, {1 << 12, {16, 8}, 4}, {1 << 8, {}, 4},
    {1 << 11, {4, 2}, 8}, {1 << 7, {16, 8}, 8}, {2, {}, 4}, {1 << 6, {4, 2}, 2}, {1 << 10, {16, 8}, 8}, {1 << 13, {16, 8}, 4}};

// Exact-size blocks; every step reads all it is given and writes all it owes (sums stand in for the hashes).
struct CheckExec {
    std::vector<std::unique_ptr<uint8_t[]>> mem; std::vector<size_t> mem_bytes;
    size_t folds = 0, ragged_folds = 0, leaf_launches = 0, pair_launches = 0, level_launches = 0, gathers = 0, forks = 0, joins = 0; bool on_side = false;
    int32_t alloc(size_t bytes, void** out) { mem.emplace_back(new uint8_t[bytes]()); mem_bytes.push_back(bytes); *out = mem.back().get(); return 0; }
    int32_t upload(void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); return 0; }
    template <class T> int32_t put(const std::vector<T>& h, T** out) {
        void* p = nullptr; alloc((h.empty() ? 1 : h.size()) * sizeof(T), &p); if (!h.empty()) std::memcpy(p, (const void*)h.data(), h.size() * sizeof(T)); *out = (T*)p; return 0;
    }
    int32_t zpows_many(const ZpowJob* jobs, size_t n_jobs, size_t max_m, fr_t* zp) {
        for (size_t s = 0; s < n_jobs; ++s) { CHECK(jobs[s].m <= max_m); fr_t acc = fr_one<PF>(); for (size_t t = 0; t < jobs[s].m; ++t) { zp[jobs[s].off + t] = acc; acc = fr_mul<PF>(acc, jobs[s].z); } }
        return 0;
    }
    int32_t fold(const fr_t* f, size_t n, const fr_t* zp, size_t m, fr_t* out) { ++folds; const FoldSeg one{0, 0}; fri_fold_ragged_host(f, n, &one, 1, zp, m, out); return 0; }
    int32_t fold_ragged(const fr_t* f, size_t n, const FoldSeg* segs, size_t n_seg, const fr_t* zp, size_t m, fr_t* out) {
        ++ragged_folds; CHECK(n_seg > 1 && segs[0].first_out == 0);
        for (size_t s = 1; s < n_seg; ++s) CHECK(segs[s].first_out > segs[s - 1].first_out && segs[s].first_out < n / m && segs[s].zp_off != segs[s - 1].zp_off);
        fri_fold_ragged_host(f, n, segs, n_seg, zp, m, out); return 0;
    }
    int32_t leaf_pairs(const fr_t* f, const fr_t* f_next, size_t n, size_t m, fr_t* h) {
        ++leaf_launches;
        for (size_t i = 0; i < n; ++i) h[i] = fr_add<PF>(f[i], f_next ? f_next[i / m] : fr_zero<PF>());
        return 0;
    }
    template <class DS> int32_t hash_level(size_t, const DS& D, fr_t* out) {
        if (std::is_same<DS, DsRaggedPairStream>::value) ++pair_launches; else ++level_launches;
        for (size_t k = 0; k < D.n_out; ++k) { fr_t acc = fr_zero<PF>(); for (size_t q = 0; q < D.total(k); ++q) acc = fr_add<PF>(acc, D.elem(k, q)); out[k] = acc; }
        return 0;
    }
    int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** x) { DsRaggedStream::Seg* d = nullptr; put(h, &d); *x = d; return 0; }
    int32_t gather(const MerkleGatherList& G, fr_t* out) { ++gathers; for (size_t i = 0; i < G.size(); ++i) out[G.row_of(i)] = G.base[G.src[i]][G.index[i]]; return 0; }
    int32_t fork() { ++forks; return 0; }
    void side(bool on) { on_side = on; }
    int32_t join() { ++joins; return 0; }
};

static size_t passes_run = 0, trees_checked = 0;
static void run_pass(const std::vector<size_t>& n0, const std::vector<size_t>& sched) {
    const size_t Bp = n0.size(), L = sched.size();
    CheckExec X; FriMixedCommit<CheckExec> C(X); std::string err;
    CHECK(C.shape(Bp, n0.data(), sched.data(), L, err) == 0);
    if (failures) return;
    for (size_t l = 0; l <= L; ++l) {                                            // the layout: prefix sums, and the invariant that carries the partner rule
        CHECK(C.at[l][0] == 0);
        for (size_t b = 0; b < Bp; ++b) CHECK(C.at[l][b + 1] - C.at[l][b] == C.n[b][l]);
        if (l < L) for (size_t b = 0; b <= Bp; ++b) CHECK(C.at[l + 1][b] * sched[l] == C.at[l][b]);
        CHECK(C.parts[l].size() == 1 || (l == L && C.parts[l].size() == 2));     // the arity differs on the last layer only
        for (size_t b = 0; b < Bp; ++b) { CHECK(C.arity[b][l] == pick_arity_for_layer(C.n[b][l], l < L ? sched[l] : 1)); if (l == L) CHECK(C.arity[b][l] == (C.n[b][l] > 1 ? 2u : 1u)); }
    }
    for (size_t l = 0; l < L; ++l) for (size_t b = 0; b < Bp; ++b) {             // one challenge per distinct (l, n_l), shared by equal sizes
        const auto& K = C.zkeys[C.zkey_of[l][b]]; CHECK(K.l == l && K.n == C.n[b][l]);
        for (size_t c = 0; c < b; ++c) CHECK((C.n[c][l] == C.n[b][l]) == (C.zkey_of[l][c] == C.zkey_of[l][b]));
    }
    std::vector<fr_t> z(C.zkeys.size()); for (size_t k = 0; k < z.size(); ++k) z[k] = fr_from_u64<PF>(3 + k);
    CHECK(C.init(z.data()) == 0);
    for (size_t i = 0; i < C.at[0][Bp]; ++i) C.f[0][i] = fr_from_u64<PF>(i + 1);
    CHECK(C.run() == 0);
    bool equal = true; for (size_t e : n0) equal = equal && e == n0[0];
    CHECK(X.folds + X.ragged_folds == L && (equal ? X.ragged_folds == 0 : true) && X.gathers == 1 && X.forks == 1 && X.joins == 1 && !X.on_side);
    for (size_t b = 0; b < Bp; ++b) for (size_t l = 0; l <= L; ++l) {            // every tree: its own level list, its root the top of it
        const std::vector<size_t> lens = merkle_level_lens(C.n[b][l], C.arity[b][l]);
        CHECK(C.levels(b, l) == lens.size());
        for (size_t v = 0; v < lens.size(); ++v) { size_t len = 0; const fr_t* p = C.level_at(b, l, v, &len); CHECK(len == lens[v]); fr_t s = fr_zero<PF>(); for (size_t i = 0; i < len; ++i) s = fr_add<PF>(s, p[i]); (void)s; }
        size_t len = 0; const fr_t* top = C.level_at(b, l, lens.size() - 1, &len);
        CHECK(len == 1 && fr_eq(top[0], C.roots[b * (L + 1) + l]));
        CHECK(C.layer_at(b, l) == C.f[l] + C.at[l][b]); ++trees_checked;
    }
    ++passes_run;
}

int main() {
    const size_t B = kTraces.size();
    std::vector<size_t> n0(B), r(B), flat, off(1, 0);
    for (size_t i = 0; i < B; ++i) { n0[i] = kTraces[i].n0; r[i] = kTraces[i].r; flat.insert(flat.end(), kTraces[i].sched.begin(), kTraces[i].sched.end()); off.push_back(flat.size()); }
    flat.push_back(0);                                                           // never read: keeps data() valid behind the last schedule
    const auto classes = mixed_prove_classes(B, flat.data(), off.data());
    const std::vector<std::vector<size_t>> want = {{0, 2, 6, 9}, {1, 4, 7, 10, 11}, {3}, {5, 8}};
    CHECK(classes == want);
    CHECK(mixed_prove_groups(B, n0.data(), flat.data(), off.data(), r.data()).size() == 11);      // what option 0 makes of the same call: only traces 1 and 10 share a shape
    for (const auto& G : classes) {
        std::vector<size_t> nn; for (size_t i : G) nn.push_back(n0[i]);
        const std::vector<size_t>& sched = kTraces[G[0]].sched;
        for (size_t rows : {(size_t)1 << 22, (size_t)5000, (size_t)1}) {
            const std::vector<size_t> passes = mixed_prove_passes(nn.size(), nn.data(), rows, 32768);
            size_t p0 = 0;
            for (size_t k : passes) {
                size_t sum = 0; for (size_t j = 0; j < k; ++j) sum += nn[p0 + j];
                CHECK(k >= 1 && (k == 1 || sum <= rows));
                if (p0 + k < nn.size()) CHECK(sum + nn[p0 + k] > rows);           // greedy: the next trace did not fit
                run_pass(std::vector<size_t>(nn.begin() + p0, nn.begin() + p0 + k), sched);
                p0 += k;
            }
            CHECK(p0 == nn.size());
            if (rows == 5000 && G.size() == 5) CHECK((passes == std::vector<size_t>{1, 2, 1, 1}));
        }
        run_pass(std::vector<size_t>(nn.rbegin(), nn.rend()), sched);
        CHECK(mixed_prove_passes(nn.size(), nn.data(), (size_t)1 << 22, 2).size() == (nn.size() + 1) / 2);
    }
    {   // a schedule that does not divide, an empty pass, and arity 1 over more than one leaf are refused by shape()
        CheckExec X; FriMixedCommit<CheckExec> C(X); std::string err; const size_t bad[] = {64, 20}, s42[] = {4, 2}, odd[] = {6}, s2[] = {2};
        CHECK(C.shape(2, bad, s42, 2, err) == -1); CHECK(C.shape(0, bad, s42, 2, err) == -1); CHECK(C.shape(1, odd, s2, 1, err) == -2);
    }
    std::printf("{\"classes\": %zu, \"passes\": %zu, \"trees\": %zu, \"failures\": %d}\n", classes.size(), passes_run, trees_checked, failures);
    return failures ? 1 : 0;
}
