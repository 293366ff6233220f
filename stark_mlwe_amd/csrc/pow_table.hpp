// stark_mlwe_amd/csrc/pow_table.hpp — host side of the two-level power table c0 * g^j = lo[j mod 2^lo_bits] * hi[j >> lo_bits] that the NTT,
// DEEP-ALI and compute_powers kernels look powers up in (PowTable / pow_lookup / k_fill_pow_table: ntt_dev.hpp): the table as an owned
// device object, and the small cache of such tables that plans and contexts keep.
#pragma once
#include <cassert>
#include <utility>
#include <vector>
#include "ctx.hpp"

namespace stark {

struct DevPowTable {
    DevMem lo, hi; int lo_bits = 0;
    PowTable view() const { return PowTable{lo.fr(), hi.fr(), lo_bits}; }
    // c0 * g^j for j < 2^(lo_bits + hi_bits), filled on the context's stream.  The new halves replace the old ones only after both are allocated
    // and the fill is launched: a fill that fails leaves the table as it was.
    template <class F> int32_t fill(stark_ctx* ctx, const fr_t& g, const fr_t& c0, int lo_bits_, int hi_bits) {
        DevMem l, h;
        STARK_HIP(ctx, l.alloc(ctx, ((size_t)1 << lo_bits_) * sizeof(fr_t))); STARK_HIP(ctx, h.alloc(ctx, ((size_t)1 << hi_bits) * sizeof(fr_t)));
        const uint64_t tot = (1ull << lo_bits_) + (1ull << hi_bits);
        hipLaunchKernelGGL(k_fill_pow_table<F>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, l.fr(), h.fr(), lo_bits_, hi_bits, g, c0);
        STARK_HIP(ctx, hipGetLastError());
        lo = std::move(l); hi = std::move(h); lo_bits = lo_bits_; return STARK_OK;
    }
};

// A few power tables keyed by (base, bits), oldest first.  A miss on a full cache synchronises the context's stream (launches in flight may
// still read the oldest table) and evicts it, so a table handed out is only good for the work enqueued before the next miss — except `pin`.
struct PowCache {
    struct Entry { fr_t base; int bits; DevPowTable tab; };
    size_t capacity; std::vector<Entry> tabs;
    explicit PowCache(size_t cap) : capacity(cap) { assert(cap >= 2); }   // `pin` below needs a second slot
    // The table of (base, bits); on a miss it is filled as c0 * base^j with the given split.  `pin` (optional) is a table fetched before that the
    // caller uses together with this one: it is never the one evicted (hence the capacity of at least 2).  (The same key twice is the same
    // table, which is correct.)
    template <class F> int32_t get(stark_ctx* ctx, const fr_t& base, int bits, const fr_t& c0, int lo_bits, int hi_bits, PowTable* out, const PowTable* pin = nullptr) {
        for (auto& e : tabs) if (e.bits == bits && fr_eq(e.base, base)) { *out = e.tab.view(); return STARK_OK; }
        if (tabs.size() >= capacity) {
            STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            tabs.erase(tabs.begin() + (pin && tabs.size() > 1 && tabs.front().tab.lo.fr() == pin->lo ? 1 : 0));
        }
        Entry e{base, bits, DevPowTable()}; STARK_TRY(e.tab.fill<F>(ctx, base, c0, lo_bits, hi_bits));
        tabs.push_back(std::move(e)); *out = tabs.back().tab.view(); return STARK_OK;
    }
};

}  // namespace stark
