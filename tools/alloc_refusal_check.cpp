// tools/alloc_refusal_check.cpp — stand-alone host check of the shared drivers' unwinding after a refused allocation: its own main, no Python, no GPU;
// built with AddressSanitizer + UBSan, leak detection on, by tools/alloc_refusal_sanitize.sh.  It compiles the host executors themselves
// (stark_mlwe_amd/csrc/hostcheck.cpp: the driver headers over HostArena, whose alloc fails on request with STARK_ERR_OOM) into this program and sweeps
// the drivers that take memory from the arena: request N = 1, 2, ... of a call is refused until a call ends with nothing refused.  These are the six
// exports of tests/test_alloc_refusal_host.py that refuse anything (hc_fri_commit_batch, hc_merkle_build_batch, hc_merkle_build_mixed_batch,
// hc_lagrange_eval_batch, hc_lagrange_eval_shard, hc_lagrange_eval_from_partials) and, beyond that test, hc_sumcheck_prove_batch and
// hc_lagrange_eval_batch_opt (the driver under "lagrange_shared_inverse" and "lagrange_share_cosets", with a coset pair among the points); the five exports
// whose drivers take nothing from the arena (the verify plans, the MLE pass loop, the transcript stream) are not here: nothing in them can be refused.
// A refused call must return the out-of-memory status, must stop at the refusal, and the unarmed repeat must give the bytes of the first, unarmed
// run; what a driver leaves behind on the way out (a block it still writes to, a table it frees twice, one it never frees) is an error of the
// sanitizers.  Inputs are seeded values: the comparison with the oracle is tests/test_alloc_refusal_host.py's.  One JSON line.
#include <cstdio>
#include <functional>
#include "../stark_mlwe_amd/csrc/hostcheck.cpp"

static int failures = 0;
static const int kNoBytes = -99;                                          // hc_sumcheck_prove_batch returned 0 bytes (its one report for every error)
#define CHECK(c) do { if (!(c)) { ++failures; std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

static uint64_t g_x = 0xA110Cu;
static uint64_t next64() { g_x = g_x * 6364136223846793005ull + 1442695040888963407ull; return g_x ^ (g_x >> 29); }
// n stored elements below the modulus (top limb below 2^62)
static std::vector<uint64_t> column(size_t n) { std::vector<uint64_t> v(4 * n); for (size_t i = 0; i < n; ++i) { for (int k = 0; k < 4; ++k) v[4 * i + k] = next64(); v[4 * i + 3] &= (1ull << 61) - 1; } return v; }

static size_t sweeps = 0, requests = 0, refusals = 0;
// run(out) -> 0 on success, the export's status otherwise; out receives the result's bytes.  refused_status: what the export returns for a refused
// allocation — STARK_ERR_OOM, except where the export has one report for every error
static void sweep(const char* name, const std::function<int(std::vector<uint64_t>&)>& run, int refused_status = kHcOom) {
    std::vector<uint64_t> want, got; uint64_t st[2];
    hc_set_alloc_refuse_at(0); CHECK(run(want) == 0); hc_alloc_refusal_stats(st); const uint64_t total = st[0]; CHECK(st[1] == 0);
    uint64_t fired = 0;
    for (uint64_t n = 1; n <= total + 1; ++n) {
        got.clear(); hc_set_alloc_refuse_at(n); const int rc = run(got); hc_alloc_refusal_stats(st); hc_set_alloc_refuse_at(0);
        if (!st[1]) { CHECK(rc == 0 && got == want && n == total + 1); break; }
        CHECK(rc == refused_status); CHECK(st[0] == n && st[1] == 1); ++fired;
        got.clear(); CHECK(run(got) == 0); CHECK(got == want);
    }
    CHECK(fired == total);
    if (fired != total) std::fprintf(stderr, "%s: %llu refusals for %llu requests\n", name, (unsigned long long)fired, (unsigned long long)total);
    ++sweeps; requests += total; refusals += fired;
}

int main() {
    void* tp = hc_params_new(1, 17, ""); void* cp17 = hc_params_new(2, 17, "POSEIDON-T17-X5-SEED"); void* p17 = hc_params_new(0, 17, ""); void* p9 = hc_params_new(0, 9, "");
    {   // the batched commit phase: hashed arities 16 and 8, unhashed 4 and 2, no fold at all
        struct Shape { size_t k; std::vector<size_t> sched; };
        for (const Shape& S : {Shape{8, {16, 8}}, Shape{6, {4, 2}}, Shape{5, {}}}) for (size_t B : {1, 3}) {
            const size_t n0 = (size_t)1 << S.k, L = S.sched.size();
            std::vector<std::vector<uint64_t>> f0(B); std::vector<const uint64_t*> ptr(B); for (size_t b = 0; b < B; ++b) { f0[b] = column(n0); ptr[b] = f0[b].data(); }
            sweep("fri_commit_batch", [&](std::vector<uint64_t>& out) { out.assign(4 * B * (L + 1), 0); return hc_fri_commit_batch(tp, B, ptr.data(), n0, S.sched.data(), L, 0xDEEFBAADull, out.data()); });
        }
    }
    {   // same-shape Merkle builds, plain and pairs (a NULL cp entry), and the mixed driver
        struct Shape { size_t arity, n; int pairs; void* p; };
        for (const Shape& S : {Shape{16, 257, 0, p17}, Shape{16, 17, 1, p17}, Shape{4, 64, 1, p9}, Shape{2, 5, 0, p9}, Shape{16, 1, 0, p17}}) {
            const size_t B = 3; std::vector<std::vector<uint64_t>> col(B), cc(B); std::vector<const uint64_t*> lp(B), cpp(B, nullptr); std::vector<uint64_t> labels(B);
            for (size_t b = 0; b < B; ++b) { col[b] = column(S.n); lp[b] = col[b].data(); labels[b] = 900 + b; if (S.pairs && b + 1 < B) { cc[b] = column(S.n); cpp[b] = cc[b].data(); } }
            const size_t cap = 2 * B * S.n + 64 * B;
            sweep("merkle_build_batch", [&](std::vector<uint64_t>& out) {
                out.assign(4 * cap + 64, 0);
                const int nl = hc_merkle_build_batch(S.p, S.arity, B, labels.data(), lp.data(), S.n, S.pairs, S.pairs ? cpp.data() : nullptr, out.data(), cap, (size_t*)(out.data() + 4 * cap));
                return nl < 0 ? nl : 0; });
        }
        for (int pairs = 0; pairs < 2; ++pairs) {
            const std::vector<size_t> n = {1, 2, 16, 17, 37, 256, 257, 300, 1}; const size_t B = n.size();
            std::vector<std::vector<uint64_t>> col(B), cc(B); std::vector<const uint64_t*> lp(B), cpp(B, nullptr); std::vector<uint64_t> labels(B); size_t tot = 0;
            for (size_t b = 0; b < B; ++b) { col[b] = column(n[b]); lp[b] = col[b].data(); labels[b] = 700 + b; tot += n[b]; if (pairs && b % 3) { cc[b] = column(n[b]); cpp[b] = cc[b].data(); } }
            const size_t cap = 2 * tot + 64 * B;
            sweep("merkle_build_mixed_batch", [&](std::vector<uint64_t>& out) {
                out.assign(4 * cap + B + 64 * B, 0);
                const int d = hc_merkle_build_mixed_batch(p17, 16, B, labels.data(), lp.data(), n.data(), pairs, pairs ? cpp.data() : nullptr, out.data(), cap, (size_t*)(out.data() + 4 * cap), (size_t*)(out.data() + 4 * cap + B));
                return d < 0 ? d : 0; });
        }
    }
    {   // the Lagrange driver: whole columns (one pass, and a pass per point), a block's share, the combination of the shares
        for (size_t n : {(size_t)1, (size_t)256, (size_t)1 << 12}) for (size_t mp : {0, 1}) {
            const size_t ncols = 3, npts = 3; std::vector<std::vector<uint64_t>> col(ncols); std::vector<const uint64_t*> cp(ncols);
            for (size_t c = 0; c < ncols; ++c) { col[c] = column(n); cp[c] = col[c].data(); }
            std::vector<uint64_t> z = column(npts); { const fr_t one = fr_one<PF>(); st4(z.data() + 4, one); }        // the second point lies in H
            sweep("lagrange_eval_batch", [&](std::vector<uint64_t>& out) { out.assign(4 * npts * ncols, 0); return hc_lagrange_eval_batch(ncols, cp.data(), n, nullptr, npts, z.data(), mp, out.data(), nullptr); });
            {   // the shared inverse and the coset classes: two more tables, four more uploads; the third point is the first times omega
                unsigned lg = 0; while (((size_t)1 << lg) < n) ++lg;
                std::vector<uint64_t> zc = z; st4(zc.data() + 8, fr_mul<PF>(ld4(zc.data()), fr_root_of_unity<PF>(lg)));
                for (int opt = 1; opt < 4; ++opt)
                    sweep("lagrange_eval_batch_opt", [&](std::vector<uint64_t>& out) { out.assign(4 * npts * ncols, 0);
                        return hc_lagrange_eval_batch_opt(ncols, cp.data(), n, nullptr, npts, zc.data(), mp, 2, opt & 1, opt >> 1, out.data(), nullptr, nullptr); });
            }
            if (n < 256) continue;
            const size_t j0 = n / 4, nl = n / 2 + 1; std::vector<const uint64_t*> rows(ncols); for (size_t c = 0; c < ncols; ++c) rows[c] = col[c].data() + 4 * j0;
            std::vector<uint64_t> w(4); st4(w.data(), fr_root_of_unity<PF>(n == 256 ? 8u : 12u));
            sweep("lagrange_eval_shard", [&](std::vector<uint64_t>& out) { out.assign(4 * npts * ncols, 0); return hc_lagrange_eval_shard(ncols, rows.data(), nl, j0, n, w.data(), npts, z.data(), mp, -1, out.data(), nullptr); });
            const std::vector<uint64_t> parts = column(2 * npts * ncols);
            sweep("lagrange_eval_from_partials", [&](std::vector<uint64_t>& out) { out.assign(4 * npts * ncols, 0); return hc_lagrange_eval_from_partials(2, parts.data(), ncols, n, w.data(), npts, z.data(), out.data()); });
        }
    }
    {   // the batched sum-check provers (ScBatch over the arena: layers, pointer tables, transcript pools, the commit climbs).  The export reports every error
        // as "0 bytes" and has no status to tell a refusal by: kNoBytes stands for that report here, and what the sweep checks for this driver is that the
        // refused run reports an error, stops at the refusal and leaves nothing behind
        for (int mf = 0; mf < 2; ++mf) for (size_t k : {0, 1, 4}) {
            const size_t B = 3, n = (size_t)1 << k; std::vector<std::vector<uint64_t>> w(B); std::vector<const uint64_t*> wp(B); const std::vector<uint64_t> labels = {2025, 7, 2025};
            for (size_t b = 0; b < B; ++b) { w[b] = column(n); wp[b] = w[b].data(); }
            sweep("sumcheck_prove_batch", [&](std::vector<uint64_t>& out) {
                std::vector<uint8_t> buf(1 << 20); size_t lens[3] = {0, 0, 0};
                const size_t tot = hc_sumcheck_prove_batch(tp, cp17, mf, B, wp.data(), k, labels.data(), 2, buf.data(), buf.size(), lens);
                if (!tot) return kNoBytes;
                out.assign((tot + 7) / 8 + 3, 0); std::memcpy(out.data(), buf.data(), tot); for (int b = 0; b < 3; ++b) out[out.size() - 3 + b] = lens[b];
                return 0; }, kNoBytes);
        }
    }
    hc_params_free(tp); hc_params_free(cp17); hc_params_free(p17); hc_params_free(p9);
    std::printf("{\"sweeps\": %zu, \"requests\": %zu, \"refusals\": %zu, \"failures\": %d}\n", sweeps, requests, refusals, failures);
    return failures ? 1 : 0;
}
