// stark_mlwe_amd/csrc/ntt_batch_plan.hpp — how stark_ntt_batch_dev / stark_lde_batch_dev cut a batch of columns into device passes.
// Host-only C++ (no HIP), so the CPU diagnostic build (hostcheck.cpp) compiles the identical rule.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace stark {

// `batch` columns of 2^log_out output elements each, in the caller's order, cut into consecutive passes of at most `max_elems` output elements
// (context option "ntt_batch_max_elems"): every pass takes per = max(1, max_elems >> log_out) columns, the last one what is left.  A column larger
// than the limit is a pass of its own — the drivers run a pass of one column through the single-column path.  Returns the columns per pass.
inline std::vector<size_t> ntt_batch_passes(size_t batch, int log_out, size_t max_elems) {
    const size_t per = std::max<size_t>(log_out < 0 || log_out >= 64 ? 0 : max_elems >> log_out, 1);
    std::vector<size_t> passes;
    for (size_t done = 0; done < batch; done += per) passes.push_back(std::min(per, batch - done));
    return passes;
}

// Two of the `batch` byte ranges [p[i], p[i] + bytes) overlap (the outputs of a batch call must not; bytes > 0).
inline bool ntt_batch_ranges_overlap(const void* const* p, size_t batch, size_t bytes) {
    std::vector<uintptr_t> a(batch);
    for (size_t i = 0; i < batch; ++i) a[i] = (uintptr_t)p[i];
    std::sort(a.begin(), a.end());
    for (size_t i = 1; i < batch; ++i) if (a[i] - a[i - 1] < bytes) return true;
    return false;
}

}  // namespace stark
