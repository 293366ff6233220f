// stark_mlwe_amd/csrc/ntt_mixed_plan.hpp — the launch plan of stark_ntt_mixed_batch_dev / stark_lde_mixed_batch_dev: columns of any lengths in one pass;
// and the rules every batched NTT / LDE call shares (pass cutting, overlap check, which extensions skip their padding).
// Host-only C++ (no HIP) apart from the inline pieces the kernels share (NTT_HD), so the CPU diagnostic build (hostcheck.cpp) compiles the identical
// rules: the split of a transform into passes, the tile width, the tile lookup of a ragged launch, the pass cutting, the overlap check and the plan.
//
// Step schedule.  A transform of 2^m points has P(m) = 1, 2 or 3 passes (ntt_split); its passes occupy steps 3 - P .. 2 of a three-step schedule, so
// steps 0 and 1 hold strided passes only and step 2 every column's last pass.  A step is one RAGGED launch per kernel instantiation it needs (strided or
// last, with or without the load-time pre-scale): at most 1 + 2 + 2 = 5 launches for a mixed transform, whatever the batch and however many distinct
// sizes occur.  A mixed LDE is the inverse transforms (at most 3 launches: none is pre-scaled), one ragged pad/copy launch and the forward transforms.
// A launch whose columns all have one shape (every launch of a batch of equal lengths, and often the strided launches of a mixed one) needs no lookup:
// ntt_mixed_one_shape says how the NttBatchAddr kernels address it instead.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define NTT_HD __host__ __device__ inline
#else
#define NTT_HD inline
#endif

namespace stark {

// LDS words of a tile with E elements and NT stage twiddles (both SoA blocks 16-byte aligned)
NTT_HD constexpr size_t ntt_tile_words(size_t E, size_t NT) { return ((9 * E + 3) & ~(size_t)3) + ((9 * NT + 3) & ~(size_t)3); }
inline size_t ntt_lds_bytes(int log_b, int log_c) { return ntt_tile_words((size_t)1 << (log_b + log_c), log_b > 0 ? (size_t)1 << (log_b - 1) : 1) * 4; }

// The passes of a transform of 2^log_n points: sizes into b[0 .. P), every one at most 2^10.  Returns P.
inline int ntt_split(int log_n, int b[3]) {
    b[0] = b[1] = b[2] = 0;
    if (log_n <= 10) { b[0] = log_n; return 1; }
    if (log_n <= 20) { b[0] = (log_n + 1) / 2; b[1] = log_n - b[0]; return 2; }
    b[0] = (log_n + 2) / 3; b[1] = (log_n - b[0] + 1) / 2; b[2] = log_n - b[0] - b[1]; return 3;
}

// What the tile width depends on besides the pass: options "ntt_log_tile" (and whether it was set by hand) and the LDS a workgroup may use.
struct NttTileOpts { int log_tile = 11; bool forced = false; size_t max_lds = 160 * 1024; };
// Columns (strided pass) / rows (last pass) per tile for sub-NTTs of 2^log_b points, at most 2^cap.  total_log: log2 of all elements the launch
// covers; small launches take smaller tiles so that the grid still fills the chip.
inline int ntt_pick_log_c(const NttTileOpts& o, int log_b, int cap, int total_log) {
    int le = o.log_tile; if (!o.forced && total_log - le < 9) le = std::max(8, std::min(le, total_log - 8));
    int lc = std::max(2, le - log_b); lc = std::max(0, std::min(lc, cap));
    while (lc > 0 && ntt_lds_bytes(log_b, lc) > o.max_lds) --lc;      // 2^10-point sub-NTTs: two columns per tile (36 B per element in LDS)
    return lc;
}
inline int ntt_floor_log2(uint64_t x) { int k = 0; while (x >> (k + 1)) ++k; return k; }

// Tile lookup of a ragged launch: first_tile[c] is the launch-wide index of column c's first tile (first_tile[0] == 0, strictly increasing: every
// column of a launch has at least one tile).  Returns the column c with first_tile[c] <= t (< first_tile[c + 1]); the tile inside the column is
// t - first_tile[c].  The pass kernels and the pad kernel call exactly this; hostcheck exports it.
NTT_HD uint32_t ntt_ragged_locate(const uint32_t* first_tile, uint32_t ncols, uint32_t t) {
    uint32_t lo = 0, hi = ncols;                      // invariant: first_tile[lo] <= t, and hi == ncols or first_tile[hi] > t
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (first_tile[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}

// Two of the `batch` byte ranges [p[i], p[i] + bytes[i]) overlap (the outputs of a batched call must not; an empty range overlaps nothing).
inline bool ntt_batch_ranges_overlap(const void* const* p, size_t batch, const size_t* bytes) {
    std::vector<std::pair<uintptr_t, size_t>> a;
    for (size_t i = 0; i < batch; ++i) if (bytes[i]) a.emplace_back((uintptr_t)p[i], bytes[i]);
    std::sort(a.begin(), a.end());
    for (size_t i = 1; i < a.size(); ++i) if (a[i].first - a[i - 1].first < a[i - 1].second) return true;   // sorted by start: the first overlap is one of neighbours
    return false;
}

// `batch` columns of 2^log_out[i] output elements, in the caller's order, cut into consecutive passes of at most `max_elems` output elements (context
// option "ntt_batch_max_elems"): a greedy run over the sum, which on equal lengths is max(1, max_elems >> log_out) columns per pass and what is left in
// the last (the same-size drivers cut with this rule too).  A column larger than the limit is a pass of its own (the drivers run a pass of one column
// through the single-column path).  Returns the columns per pass.
inline std::vector<size_t> ntt_mixed_passes(size_t batch, const size_t* log_out, size_t max_elems) {
    std::vector<size_t> passes; size_t cols = 0; uint64_t sum = 0;
    for (size_t i = 0; i < batch; ++i) {
        const uint64_t e = log_out[i] >= 63 ? ~0ull >> 1 : 1ull << log_out[i];
        if (cols && sum + e > max_elems) { passes.push_back(cols); cols = 0; sum = 0; }
        ++cols; sum += e;
    }
    if (cols) passes.push_back(cols);
    return passes;
}

// ---- the plan of one pass -----------------------------------------------------------------------------------------------------------------------
// Where a column of a launch is read or written: the caller's input i, the caller's output i (the same vector for an in-place transform), or an
// element offset into the pass's scratch.
enum NttMixedMem : int { NTT_MEM_IN = 0, NTT_MEM_OUT = 1, NTT_MEM_SCRATCH = 2 };
struct NttMixedRef { int mem = NTT_MEM_SCRATCH; uint64_t off = 0; };
// One pass of the transforms of one size: what NttPassArgs is filled from (capi_ntt.hip), at most 31 per launch.
struct NttMixedShape {
    int log_n = 0, P = 1, pass = 0;       // the transform, its number of passes, this pass
    int log_b = 0, log_c = 0, log_m = 0;  // sub-NTT size, tile width, log2 of the sub-problem this pass splits (strided passes)
    int log_nonzero = -1;                 // first pass of a zero-padded transform whose padding is never written: only elements j < 2^log_nonzero are read
    uint32_t tiles = 0;                   // tiles of ONE column of this shape
};
struct NttMixedCol {
    uint32_t col = 0, shape = 0, first_tile = 0;
    NttMixedRef src, dst;
    uint64_t first = 0, head = 0, len = 0;   // pad launch only: dst[i] = i < head ? src[i] : 0 over first <= i < len (shape unused, tiles of NTT_PAD_BLOCK elements)
};
enum NttMixedKind : int { NTT_MIXED_INVERSE = 0, NTT_MIXED_PAD = 1, NTT_MIXED_FORWARD = 2 };
static const uint32_t NTT_PAD_BLOCK = 256;
struct NttMixedLaunch {
    int kind = NTT_MIXED_FORWARD, step = 0; bool strided = false, pre = false;
    uint32_t ntiles = 0; size_t lds = 0;                  // the grid; the dynamic LDS of the largest tile
    std::vector<NttMixedShape> shapes; std::vector<NttMixedCol> cols;      // cols in launch order: larger tiles first
};
struct NttMixedPlan { std::vector<NttMixedLaunch> launches; uint64_t scratch_elems = 0; };
// One transform of a pass: column `col`, 2^log_n points (log_n >= 1) from src to dst; `work` holds the intermediate of a transform of several passes
// (it may be src: a strided pass works in place; never dst).
struct NttMixedItem { uint32_t col; int log_n; int log_nonzero; NttMixedRef src, dst; uint64_t work; };

// Appends the launches of the transforms `items` (all forward or all inverse; pre_first: the first pass of each applies the coset pre-scale on load).
inline void ntt_mixed_add_transforms(NttMixedPlan& plan, int kind, const std::vector<NttMixedItem>& items, bool pre_first, const NttTileOpts& o) {
    for (int step = 0; step < 3; ++step) {
        for (int form = 0; form < 2; ++form) {                        // without the pre-scale, then with it
            NttMixedLaunch L; L.kind = kind; L.step = step; L.strided = step < 2; L.pre = form == 1;
            std::vector<size_t> in; uint64_t total = 0;
            for (size_t k = 0; k < items.size(); ++k) {
                int b[3]; const int P = ntt_split(items[k].log_n, b), j = step - (3 - P);
                if (j < 0 || (pre_first && j == 0) != L.pre) continue;
                in.push_back(k); total += 1ull << items[k].log_n;
            }
            if (in.empty()) continue;
            const int total_log = ntt_floor_log2(total);
            struct Entry { size_t k; NttMixedShape s; };
            std::vector<Entry> es;
            for (size_t k : in) {
                const NttMixedItem& it = items[k]; NttMixedShape s; int b[3];
                s.log_n = it.log_n; s.P = ntt_split(it.log_n, b); s.pass = step - (3 - s.P); s.log_b = b[s.pass];
                s.log_m = it.log_n; for (int q = 0; q < s.pass; ++q) s.log_m -= b[q];
                if (L.strided) s.log_c = ntt_pick_log_c(o, s.log_b, s.log_m - s.log_b, total_log);
                else s.log_c = s.P == 1 ? 0 : ntt_pick_log_c(o, s.log_b, b[0], total_log);
                const bool nz = L.strided && s.pass == 0 && it.log_nonzero >= 0 && it.log_nonzero < it.log_n && it.log_nonzero >= s.log_m - s.log_b;
                s.log_nonzero = nz ? it.log_nonzero : -1;
                s.tiles = (uint32_t)((1ull << it.log_n) >> (s.log_b + s.log_c));
                es.push_back(Entry{k, s});
            }
            std::stable_sort(es.begin(), es.end(), [](const Entry& a, const Entry& c) { return a.s.log_b + a.s.log_c > c.s.log_b + c.s.log_c; });
            for (const Entry& e : es) {
                const NttMixedItem& it = items[e.k]; NttMixedCol c; c.col = it.col;
                size_t sh = 0;
                while (sh < L.shapes.size() && !(L.shapes[sh].log_n == e.s.log_n && L.shapes[sh].log_nonzero == e.s.log_nonzero)) ++sh;
                if (sh == L.shapes.size()) L.shapes.push_back(e.s);
                c.shape = (uint32_t)sh; c.first_tile = L.ntiles; L.ntiles += e.s.tiles;
                if (e.s.pass == 0) c.src = it.src; else { c.src.mem = NTT_MEM_SCRATCH; c.src.off = it.work; }
                if (e.s.pass == e.s.P - 1) c.dst = it.dst; else { c.dst.mem = NTT_MEM_SCRATCH; c.dst.off = it.work; }
                L.lds = std::max(L.lds, ntt_lds_bytes(e.s.log_b, e.s.log_c));
                L.cols.push_back(c);
            }
            plan.launches.push_back(std::move(L));
        }
    }
}

// One end (all sources or all destinations) of a launch whose columns share ONE shape record, as the NttBatchAddr kernels address it: mem NTT_MEM_IN /
// NTT_MEM_OUT: the caller's vectors of the launch's columns, in launch order; NTT_MEM_SCRATCH: the k-th column of the launch at off + k * pitch.
struct NttMixedEnd { int mem = NTT_MEM_SCRATCH; uint64_t off = 0, pitch = 0; };
struct NttOneShape { NttMixedEnd src, dst; };
// A transform launch needs neither the tile lookup nor the shape table: one shape, and each end wholly the caller's memory of one kind or wholly scratch
// at one pitch.  Then its k-th column owns the tiles [k * tiles, (k + 1) * tiles), which is the order of the NttBatchAddr kernels.
inline bool ntt_mixed_one_shape(const NttMixedLaunch& L, NttOneShape* out) {
    if (L.kind == NTT_MIXED_PAD || L.shapes.size() != 1 || L.cols.empty()) return false;
    NttOneShape S;
    for (int e = 0; e < 2; ++e) {
        auto ref = [&](size_t k) -> const NttMixedRef& { return e ? L.cols[k].dst : L.cols[k].src; };
        NttMixedEnd& E = e ? S.dst : S.src; E.mem = ref(0).mem;
        for (size_t k = 1; k < L.cols.size(); ++k) if (ref(k).mem != E.mem) return false;
        if (E.mem != NTT_MEM_SCRATCH) continue;
        E.off = ref(0).off;
        if (L.cols.size() > 1) { if (ref(1).off < E.off) return false; E.pitch = ref(1).off - E.off; }
        for (size_t k = 1; k < L.cols.size(); ++k) if (ref(k).off != E.off + k * E.pitch) return false;
    }
    if (out) *out = S;
    return true;
}

// ncols in-place transforms of 2^log_n[i] points (columns with log_n[i] == 0 take no part).  Scratch: the intermediates of the columns of several passes.
inline NttMixedPlan ntt_mixed_ntt_plan(const size_t* log_n, size_t ncols, bool inverse, bool coset, const NttTileOpts& o) {
    NttMixedPlan plan; std::vector<NttMixedItem> items;
    for (size_t i = 0; i < ncols; ++i) {
        if (log_n[i] == 0) continue;
        NttMixedItem it{(uint32_t)i, (int)log_n[i], -1, {NTT_MEM_IN, 0}, {NTT_MEM_OUT, 0}, plan.scratch_elems};
        if (log_n[i] > 10) plan.scratch_elems += 1ull << log_n[i];
        items.push_back(it);
    }
    ntt_mixed_add_transforms(plan, inverse ? NTT_MIXED_INVERSE : NTT_MIXED_FORWARD, items, coset && !inverse, o);
    return plan;
}

// The big forward transform of an LDE 2^log_n -> 2^(log_n + lb) takes its padding as zero without reading it: it has a strided first pass whose stride
// divides n, which reads only the n coefficient rows (NttPassArgs::nz_points).  Otherwise (tiny transforms) the padding is written for real.
inline bool ntt_lde_skips_padding(int log_n, int lb) {
    int b[3]; const int big = log_n + lb, P = ntt_split(big, b);
    return lb > 0 && P > 1 && big - b[0] <= log_n;
}
// ncols extensions 2^log_n[i] -> 2^(log_n[i] + lb) with one coset (coset: a pre-scale is applied, the shift is given and not one).  Column i owns
// X_i (N_i elements) and C_i (n_i elements) of the scratch.  lde_run's routing per column: the inverse transform reads the caller's column and leaves the
// coefficients in C_i at pitch n_i when the forward transform's first pass skips the padding, else in X_i with the tail [n_i, N_i) zeroed by the pad
// launch; its intermediate is the other region.  A one-point column is its own interpolation: the pad launch writes the point and its padding (straight
// into the output when lb == 0).  The forward transform works in X_i and its last pass stores into the caller's output.
inline NttMixedPlan ntt_mixed_lde_plan(const size_t* log_n, size_t ncols, int lb, bool coset, const NttTileOpts& o) {
    NttMixedPlan plan; std::vector<NttMixedItem> inv, fwd; NttMixedLaunch pad; pad.kind = NTT_MIXED_PAD; pad.step = 0;
    for (size_t i = 0; i < ncols; ++i) {
        const int ln = (int)log_n[i], big = ln + lb; const uint64_t n = 1ull << ln, N = 1ull << big;
        const uint64_t X = plan.scratch_elems, Cs = X + N; plan.scratch_elems += N + n;
        const bool skip = ntt_lde_skips_padding(ln, lb);
        const NttMixedRef coef{NTT_MEM_SCRATCH, skip ? Cs : X};
        if (ln > 0) inv.push_back(NttMixedItem{(uint32_t)i, ln, -1, {NTT_MEM_IN, 0}, coef, skip ? X : Cs});
        if (ln == 0 || (N > n && !skip)) {
            NttMixedCol c; c.col = (uint32_t)i; c.first_tile = pad.ntiles;
            if (ln == 0) { c.src.mem = NTT_MEM_IN; c.dst = big == 0 ? NttMixedRef{NTT_MEM_OUT, 0} : coef; c.first = 0; c.head = 1; }
            else { c.src = coef; c.dst = coef; c.first = n; c.head = 0; }
            c.len = N; pad.ntiles += (uint32_t)((c.len - c.first + NTT_PAD_BLOCK - 1) / NTT_PAD_BLOCK);
            pad.cols.push_back(c);
        }
        if (big > 0) fwd.push_back(NttMixedItem{(uint32_t)i, big, skip ? ln : -1, coef, {NTT_MEM_OUT, 0}, X});
    }
    ntt_mixed_add_transforms(plan, NTT_MIXED_INVERSE, inv, false, o);
    if (!pad.cols.empty()) plan.launches.push_back(std::move(pad));
    ntt_mixed_add_transforms(plan, NTT_MIXED_FORWARD, fwd, coset, o);
    return plan;
}

}  // namespace stark
