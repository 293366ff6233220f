// tools/mfma_finish_check.cpp — stand-alone host check (its own main, no GPU, no Python) of the residue-table form of the t = 17 full rounds, of
// the lane product of the 8-round partial blocks with the base lane in the tile (finish with base), and of the blocks' H rows of up to 16 + 7 K-steps:
// the fragment tables (host_util.hpp mfma_frags), the fold + finishing step and the limb-form hand-over to the next S-box (mfma_digits.hpp, the
// statements the kernels compile: finish to limbs, S-box on lazy limbs, the lazy chain's finish with a constant, slot and chain step, the signed-residue lanes through nine limbs and by the byte-domain finish, the word-column finish to nine limbs),
// against the portable field code.  Meant for a
// sanitizer build; tools/mfma_finish_sanitize.sh builds it with AddressSanitizer + UBSan and runs it:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I stark_mlwe_amd/csrc tools/mfma_finish_check.cpp -o tools/bin/mfma_finish_check
#include <cstdio>
#include <cstdint>
#include <vector>
#include "fr.hpp"
#include "host_util.hpp"
#include "mfma_digits.hpp"
using namespace stark;

static fr_t finish(const int32_t* S) { int64_t col[9]; mfma_cols_of_sums(S, col); return mfma_finish_cols(col); }
// sum_c S_c 256^c mod r as a plain integer, through the field code
static fr_t reference(const int32_t* S) {
    fr_t acc = host::h_zero(), w = host::h_one(); const fr_t k256 = fr_from_u64<PF>(256);
    for (int c = 0; c < 32; ++c, w = host::h_mul(w, k256)) {
        const fr_t term = host::h_mul(fr_from_u64<PF>((uint64_t)(S[c] < 0 ? -(int64_t)S[c] : (int64_t)S[c])), w);
        acc = S[c] < 0 ? host::h_sub(acc, term) : host::h_add(acc, term);
    }
    return fr_to_canonical<PF>(acc);
}
// V = k r + d (k any sign, d in {-1, 0, 1}) -> 32 digit sums with V = sum S_c 256^c: signed radix-256 digits at c < 31, S_31 carries the surplus
static std::vector<int32_t> split_kr(int64_t k, int d) {
    const bool neg = k < 0 || (k == 0 && d < 0);
    const uint64_t ak = (uint64_t)(k < 0 ? -k : k); const int dd = neg ? -d : d;          // |V| = ak r + dd >= 0
    uint32_t w[10]; uint64_t c = 0;
    for (int i = 0; i < 8; ++i) { const uint64_t t = ak * PF::P(i) + c; w[i] = (uint32_t)t; c = t >> 32; }
    w[8] = (uint32_t)c; w[9] = (uint32_t)(c >> 32);
    int64_t cy = dd;
    for (int i = 0; i < 10 && cy; ++i) { const int64_t t = (int64_t)w[i] + cy; w[i] = (uint32_t)t; cy = t >> 32; }
    std::vector<int32_t> S(32); int carry = 0;
    for (int b = 0; b < 31; ++b) { const int v = (int)((w[b >> 2] >> (8 * (b & 3))) & 0xff) + carry; carry = v >= 128; S[b] = carry ? v - 256 : v; }
    int64_t rest = carry;
    for (int b = 31; b < 38; ++b) rest += (int64_t)((w[b >> 2] >> (8 * (b & 3))) & 0xff) << (8 * (b - 31));
    S[31] = (int32_t)rest;
    if (neg) for (auto& v : S) v = -v;
    return S;
}
int main() {
    const int32_t LIM = (1 << 24) - 1; long bad = 0, n = 0;
    std::vector<std::vector<int32_t>> cases;
    cases.push_back(std::vector<int32_t>(32, LIM)); cases.push_back(std::vector<int32_t>(32, -LIM)); cases.push_back(std::vector<int32_t>(32, 0));
    { std::vector<int32_t> a(32), b(32); for (int c = 0; c < 32; ++c) { a[c] = c & 1 ? -LIM : LIM; b[c] = -a[c]; } cases.push_back(a); cases.push_back(b); }
    for (int c : {0, 31}) for (int32_t v : {1, -1, LIM, -LIM}) { std::vector<int32_t> s(32, 0); s[c] = v; cases.push_back(s); }
    // V = k 2^254 - 1, k 2^254, k 2^254 + 1: S_31 = k 2^6 (+-), the rest from the signed digits of -1 / 0 / +1
    for (int32_t k : {-(1 << 17), -1, 0, 1, 1 << 17}) for (int d : {-1, 0, 1}) { std::vector<int32_t> s(32, 0); s[31] = k * 64; s[0] = d; cases.push_back(s); }
    // V = k r - 1, k r, k r + 1: the two ends of the range the conditional subtractions see
    for (int64_t k : {-(int64_t)(1 << 17), (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)(1 << 17)}) for (int d : {-1, 0, 1}) {
        const std::vector<int32_t> s = split_kr(k, d);
        for (int c = 0; c < 32; ++c) if (s[c] > LIM || s[c] < -LIM || (c < 31 && (s[c] > 128 || s[c] < -128))) { fprintf(stderr, "crafted case outside the domain\n"); return 1; }
        cases.push_back(s);
    }
    uint64_t x = 0x9e3779b97f4a7c15ull; auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int i = 0; i < 20000; ++i) { std::vector<int32_t> s(32); for (auto& v : s) v = (int32_t)(rnd() % (2 * (uint64_t)LIM + 1)) - LIM; cases.push_back(s); }
    { int idx = 0;                                      // k r + d is d mod r whatever k: checked without the reference as well
      for (int64_t k : {-(int64_t)(1 << 17), (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)(1 << 17)}) for (int d : {-1, 0, 1}) {
        const fr_t got = finish(split_kr(k, d).data()); fr_t want = host::h_zero(); if (d > 0) want.v[0] = 1; if (d < 0) { for (int i = 0; i < 8; ++i) want.v[i] = PF::P(i); want.v[0] -= 1; }
        ++n; ++idx; if (!fr_eq(got, want)) { if (bad < 5) fprintf(stderr, "k r + d: mismatch in crafted case %d\n", idx - 1); ++bad; }
      } }
    for (const auto& s : cases) { ++n; if (!fr_eq(finish(s.data()), reference(s.data()))) { if (bad < 5) fprintf(stderr, "finishing step: mismatch in case %ld\n", n - 1); ++bad; } }
    // the tables: one emulated product per matrix against the dense field product (states of S-box outputs: the tables carry 2^20)
    const host::KernelConsts kc = host::make_kernel_consts(host::consts_transcript());
    if (!kc.ok || kc.mds_frag.size() != (size_t)17 * 17 * 64 * 16) { fprintf(stderr, "tables missing\n"); return 1; }
    const fr_t k20 = fr_from_u64<PF>(1ull << FR29_SBOX_SHIFT);
    for (int pre = 0; pre < 2; ++pre) for (int rep = 0; rep < 8; ++rep) {
        const std::vector<int8_t>& F = pre ? kc.mds_pre_frag : kc.mds_frag; const std::vector<fr_t>& M = pre ? kc.mds_pre : kc.mds;
        fr_t st[17], xd[17];
        for (int e = 0; e < 17; ++e) { for (int i = 0; i < 8; ++i) st[e].v[i] = (uint32_t)rnd(); st[e].v[7] &= 0x3fffffffu; if (rep == 0) st[e] = e & 1 ? host::h_zero() : host::h_sub(host::h_zero(), host::h_one()); xd[e] = recode_signed(st[e]); }
        for (int i = 0; i < 17; ++i) {
            int32_t S[32];
            for (int r = 0; r < 32; ++r) { int64_t acc = 0;
                for (int e = 0; e < 17; ++e) for (int kh = 0; kh < 2; ++kh) { const int8_t* a = &F[((((size_t)i * 17 + e) * 64) + (r + 32 * kh)) * 16];
                    const int8_t* b = reinterpret_cast<const int8_t*>(xd[e].v) + 16 * kh; for (int j = 0; j < 16; ++j) acc += (int64_t)a[j] * b[j]; }
                S[r] = (int32_t)acc; }
            fr_t want = host::h_zero(); for (int e = 0; e < 17; ++e) want = host::h_add(want, host::h_mul(host::h_mul(M[(size_t)i * 17 + e], k20), st[e]));
            ++n; if (!fr_eq(finish(S), want)) { if (bad < 5) fprintf(stderr, "product: mismatch pre %d rep %d row %d\n", pre, rep, i); ++bad; }
        }
    }
    // ---- the lane product of the 8-round partial blocks (poseidon_pair.hpp pair_block8): the base lane enters the tile as a NINTH K-step against the
    // fragment of the constant 1 (the last KiB of blk8_lfrag).  (i) finish with base: for every crafted total above (the extremes +-(2^24 - 1), the
    // multiples of r and of 2^254) and 2000 of the random ones, and base in {0, 1, r - 1, random}: the y part S = total - unit K-step(base), the
    // kernel's sum S + unit K-step(base) finished, against (sum_c S_c 256^c + base) mod r.  (ii) whole lane rows of block 0 and of the last block
    // through the tables: eight y and a base at 0 / r - 1 / random, against base + sum_p w_{p,j} 2^20 y_p in the field code.
    if (kc.blk8_lfrag.size() != (size_t)(8 * 16 * 8 + 1) * 1024 || kc.blk8_efrag.size() != (size_t)8 * 8 * 16 * 1024) { fprintf(stderr, "block-8 tables missing\n"); return 1; }
    const int8_t* unit = kc.blk8_lfrag.data() + kc.blk8_lfrag.size() - 1024;
    auto kstep = [](const int8_t* frag, const fr_t& xd, int64_t* S) {
        for (int r = 0; r < 32; ++r) for (int kh = 0; kh < 2; ++kh) { const int8_t* a = frag + (size_t)(r + 32 * kh) * 16; const int8_t* b = reinterpret_cast<const int8_t*>(xd.v) + 16 * kh; for (int j = 0; j < 16; ++j) S[r] += (int64_t)a[j] * b[j]; } };
    auto rand_fr = [&]() { fr_t v; for (int i = 0; i < 8; ++i) v.v[i] = (uint32_t)rnd(); v.v[7] &= 0x3fffffffu; return v; };
    fr_t rm1; for (int i = 0; i < 8; ++i) rm1.v[i] = PF::P(i); rm1.v[0] -= 1;
    fr_t one = host::h_zero(); one.v[0] = 1;
    const size_t ncraft = cases.size() - 20000;
    for (size_t ci = 0; ci < ncraft + 2000; ++ci) for (int bi = 0; bi < 4; ++bi) {
        const fr_t base = bi == 0 ? host::h_zero() : bi == 1 ? one : bi == 2 ? rm1 : rand_fr();
        int64_t U[32] = {0}; kstep(unit, recode_signed(base), U);
        int32_t Sy[32], St[32]; bool in_domain = true;
        for (int c = 0; c < 32; ++c) { if (U[c] > 32 * 128 * 128 || U[c] < -32 * 128 * 128) { fprintf(stderr, "unit K-step beyond its bound\n"); return 1; }
            const int64_t y = (int64_t)cases[ci][c] - U[c]; Sy[c] = (int32_t)y; St[c] = (int32_t)(y + U[c]); if (St[c] > LIM || St[c] < -LIM) in_domain = false; }
        if (!in_domain) { fprintf(stderr, "with base: total outside the domain\n"); return 1; }
        ++n; if (!fr_eq(finish(St), fr_add<PF>(reference(Sy), base))) { if (bad < 5) fprintf(stderr, "finish with base: mismatch in case %zu base %d\n", ci, bi); ++bad; }
    }
    for (int blk : {0, 7}) for (int rep = 0; rep < 6; ++rep) {
        fr_t y[8], yd[8];
        for (int p = 0; p < 8; ++p) { y[p] = rep == 0 ? rm1 : rep == 1 ? host::h_zero() : rep == 2 ? ((p & 1) ? rm1 : host::h_zero()) : rand_fr(); yd[p] = recode_signed(y[p]); }
        for (int j = 1; j < 17; ++j) {
            const fr_t base = rep == 0 ? rm1 : rep == 1 ? host::h_zero() : rep == 2 ? rm1 : rand_fr();
            int64_t S64[32] = {0};
            for (int p = 0; p < 8; ++p) kstep(kc.blk8_lfrag.data() + (((size_t)blk * 16 + (j - 1)) * 8 + p) * 1024, yd[p], S64);
            kstep(unit, recode_signed(base), S64);
            int32_t S[32]; for (int c = 0; c < 32; ++c) { if (S64[c] > 9 * 32 * 128 * 128 || S64[c] < -9 * 32 * 128 * 128) { fprintf(stderr, "lane row beyond its bound\n"); return 1; } S[c] = (int32_t)S64[c]; }
            fr_t want = base;
            for (int p = 0; p < 8; ++p) want = host::h_add(want, host::h_mul(host::h_mul(kc.sparse[(size_t)(8 * blk + p) * 33 + 16 + j], k20), y[p]));
            ++n; if (!fr_eq(finish(S), want)) { if (bad < 5) fprintf(stderr, "lane row: mismatch block %d rep %d lane %d\n", blk, rep, j); ++bad; }
        }
    }
    // ---- the H rows of the 8-round partial blocks: H_q = E_q + sum_{p<q} Gamma_{q,p} y_p as ONE tile of 16 + q K-steps, E fragments (unscaled) against the
    // lanes and blk8_gfrag (Gamma * 2^20) against the y.  Rows 1, 4 and 7 (17, 20 and 23 K-steps) of block 0 and of the last block, lanes and y at
    // r - 1 / 0 / alternating / random, against sum_j u_{q,j} s_j + sum_p (sum_j u_{q,j} w_{p,j}) 2^20 y_p in the field code; the bound of the longest row checked.
    if (kc.blk8_gfrag.size() != (size_t)8 * 28 * 1024) { fprintf(stderr, "block-8 Gamma fragments missing\n"); return 1; }
    for (int blk : {0, 7}) for (int q : {1, 4, 7}) for (int rep = 0; rep < 6; ++rep) {
        fr_t sl[16], y[7]; int64_t S64[32] = {0};
        for (int j = 0; j < 16; ++j) sl[j] = rep == 0 ? rm1 : rep == 1 ? host::h_zero() : rep == 2 ? ((j & 1) ? rm1 : host::h_zero()) : rand_fr();
        for (int p = 0; p < q; ++p) y[p] = rep == 0 ? rm1 : rep == 1 ? host::h_zero() : rep == 2 ? ((p & 1) ? host::h_zero() : rm1) : rand_fr();
        const fr_t* uq = &kc.sparse[(size_t)(8 * blk + q) * 33];
        fr_t want = host::h_zero();
        for (int j = 0; j < 16; ++j) { kstep(kc.blk8_efrag.data() + (((size_t)blk * 8 + q) * 16 + j) * 1024, recode_signed(sl[j]), S64); want = host::h_add(want, host::h_mul(uq[1 + j], sl[j])); }
        for (int p = 0; p < q; ++p) {
            kstep(kc.blk8_gfrag.data() + ((size_t)blk * 28 + q * (q - 1) / 2 + p) * 1024, recode_signed(y[p]), S64);
            fr_t g = host::h_zero(); for (int j = 0; j < 16; ++j) g = host::h_add(g, host::h_mul(uq[1 + j], kc.sparse[(size_t)(8 * blk + p) * 33 + 17 + j]));
            want = host::h_add(want, host::h_mul(host::h_mul(g, k20), y[p]));
        }
        int32_t S[32]; for (int c = 0; c < 32; ++c) { if (S64[c] > (16 + q) * 32 * 128 * 128 || S64[c] < -(16 + q) * 32 * 128 * 128 || S64[c] > LIM || S64[c] < -LIM) { fprintf(stderr, "H row beyond its bound\n"); return 1; } S[c] = (int32_t)S64[c]; }
        ++n; if (!fr_eq(finish(S), want)) { if (bad < 5) fprintf(stderr, "H row: mismatch block %d row %d rep %d\n", blk, q, rep); ++bad; }
    }
    // ---- the limb-form hand-over of the fused full-round rows (poseidon_pair.hpp pair_mds_sbox_mfma).  (i) finish to limbs (mfma_finish_limbs) on every case
    // above: limbs 0..7 below 2^29, the top limb below 2^24, the value inside (2^254 - 2^145, 2^255 + 2^145) — top limb in [2^22 - 1, 2^23] —, and its
    // canonical form equal to the finishing step's.  (ii) the S-box on those limbs plus a round constant from rc_full29 (sbox_lazy29) against fr_pow5_r29 of the
    // canonical sum, for every crafted case against eight constants and every random case against one.  (iii) every limb at its maximum, the top limbs at the
    // ends of their ranges: the same steps with 128-bit columns (Lazy29Wide) agree and no column reaches 2^64.
    if (kc.rc_full29.size() != (size_t)8 * 17 * 9) { fprintf(stderr, "rc_full29 missing\n"); return 1; }
    auto finish_limbs = [](const int32_t* S, uint32_t* l) { int64_t col[9]; mfma_cols_of_sums(S, col); mfma_finish_limbs(col, l); };
    for (size_t ci = 0; ci < cases.size(); ++ci) {
        uint32_t l[9]; finish_limbs(cases[ci].data(), l);
        bool ok = l[8] < (1u << 24) && l[8] >= (1u << 22) - 1 && l[8] <= (1u << 23);
        for (int i = 0; i < 8; ++i) ok = ok && l[i] <= FR_M29;
        fr_t z = fr29_pack_reduce<PF>(l); fr_cond_sub<PF>(z.v, 0u);
        const fr_t canon = finish(cases[ci].data());
        ++n; if (!ok || !fr_eq(z, canon)) { if (bad < 5) fprintf(stderr, "finish to limbs: case %zu\n", ci); ++bad; }
        for (int e = 0; e < (ci < ncraft ? 8 : 1); ++e) {
            const size_t idx = (ci * 7 + (size_t)e * 17) % (8 * 17);
            const fr_t want = fr_pow5_r29<PF>(fr_add<PF>(canon, kc.rc_full[idx]));
            ++n; if (!fr_eq(sbox_lazy29(l, &kc.rc_full29[9 * idx]), want)) { if (bad < 5) fprintf(stderr, "S-box on lazy limbs: case %zu constant %zu\n", ci, idx); ++bad; }
        }
    }
    for (uint32_t l8 : {0u, 1u << 22, 3u * (1u << 22) - 1}) for (uint32_t c8 : {0u, (1u << 22) - 1}) {
        uint32_t l[9], c[9]; for (int i = 0; i < 8; ++i) l[i] = c[i] = FR_M29; l[8] = l8; c[8] = c8;
        Lazy29Wide wide; const fr29_t x5 = wide.pow5(l, c);
        ++n; if ((wide.max_col >> 64) != 0 || !fr_eq(sbox_lazy29(l, c), fr29_pack_reduce<PF>(x5.l))) { if (bad < 5) fprintf(stderr, "S-box on lazy limbs: column overflow at l8 %u c8 %u\n", l8, c8); ++bad; }
    }
    // ---- the lazy chain of the 8-round blocks (poseidon_pair.hpp blk8_round_x / blk8_round_y).  (i) the finish with a constant in the columns (0, 1, r - 1
    // and a scaled round constant from rc_partial_scaled29) on every case above: limbs in range, the value inside (2^254 - 2^145, 2^255 + 2^145), canonical form
    // = finish + constant; the mailbox slot returns the same limbs.  (ii) one chain step on it: x5 = pow5_lazy29 of a lazy u, recoded unreduced (digits sum to
    // the canonical x5 under the unit fragment's finish), u' = x5 + slot within pow5_lazy29's contract, and pow5 of u' equal to fr_pow5_r29 of the canonical sum.
    if (kc.rc_partial_scaled29.size() != (size_t)65 * 9) { fprintf(stderr, "rc_partial_scaled29 missing\n"); return 1; }
    for (int i = 0; i < 9; ++i) if (kc.rc_partial_scaled29[64 * 9 + i] != 0) { fprintf(stderr, "rc_partial_scaled29: the closing entry is not zero\n"); return 1; }
    for (size_t ci = 0; ci < cases.size(); ++ci) for (int k = 0; k < (ci < ncraft ? 4 : 1); ++k) {
        const int kk = ci < ncraft ? k : (int)(ci & 3);
        const fr_t cst = kk == 0 ? host::h_zero() : kk == 1 ? one : kk == 2 ? rm1 : kc.rc_partial_scaled[ci % 64];
        const fr29_t c29l = fr29_unpack(cst);
        int64_t col[9]; uint32_t l[9]; mfma_cols_of_sums(cases[ci].data(), col, c29l.l); mfma_finish_limbs(col, l);
        bool ok = l[8] < (1u << 24) && l[8] >= (1u << 22) - 1 && l[8] <= (1u << 23);
        for (int i = 0; i < 8; ++i) ok = ok && l[i] <= FR_M29;
        fr_t z = fr29_pack_reduce<PF>(l); fr_cond_sub<PF>(z.v, 0u);
        const fr_t hq = fr_add<PF>(finish(cases[ci].data()), cst);
        const fr_t slot = lazy29_to_slot(l);
        fr29_t zero9; for (int i = 0; i < 9; ++i) zero9.l[i] = 0;
        const fr29_t back = lazy29_add_slot(zero9, slot);
        for (int i = 0; i < 9; ++i) ok = ok && back.l[i] == l[i];
        ++n; if (!ok || !fr_eq(z, hq)) { if (bad < 5) fprintf(stderr, "finish with constant: case %zu constant %d\n", ci, kk); ++bad; }
        // a chain step: u = a canonical value plus a constant (as the chain enters a block), or every limb at its maximum
        fr29_t u = lazy29_add_c29(fr29_unpack(ci & 1 ? rm1 : rand_fr()).l, c29l.l);
        if (ci == 0) { for (int i = 0; i < 8; ++i) u.l[i] = 2 * FR_M29; u.l[8] = (3u << 22) + (1u << 20); }
        fr_t ucan = fr29_canon_lazy<PF>([&] { fr29_t t = u; fr29_norm(t); return t; }());
        const fr29_t x5 = pow5_lazy29(u);
        const fr_t x5can = fr29_pack_reduce<PF>(x5.l);
        const fr_t yd = recode_lazy29(x5);
        int64_t U[32] = {0}; kstep(unit, yd, U); int32_t S[32]; for (int c = 0; c < 32; ++c) S[c] = (int32_t)U[c];
        bool step_ok = fr_eq(x5can, fr_pow5_r29<PF>(ucan)) && fr_eq(finish(S), x5can) && (fr29_pack(x5.l).v[7] >> 24) <= 0x42;
        const fr29_t un = lazy29_add_slot(x5, slot);
        for (int i = 0; i < 9; ++i) step_ok = step_ok && un.l[i] < (1u << 30);
        step_ok = step_ok && fr_eq(fr29_pack_reduce<PF>(pow5_lazy29(un).l), fr_pow5_r29<PF>(fr_add<PF>(x5can, hq)));
        ++n; if (!step_ok) { if (bad < 5) fprintf(stderr, "chain step: case %zu constant %d\n", ci, kk); ++bad; }
    }
    // ---- the lanes between two blocks from the signed residue (mfma_finish_recoded: floor quotient, sign-extended pack, recode) on every case above: the top
    // limb in [-1, 2^22], and the digits, taken through the unit fragment's K-step and the canonical finish as the next block's products take them, give the
    // canonical value of the row
    for (size_t ci = 0; ci < cases.size(); ++ci) {
        int64_t col[9]; uint32_t l[9]; mfma_cols_of_sums(cases[ci].data(), col); mfma_finish_limbs_floor(col, l);
        bool ok = (int32_t)l[8] >= -1 && (int32_t)l[8] <= (1 << 22);
        for (int i = 0; i < 8; ++i) ok = ok && l[i] <= FR_M29;
        mfma_cols_of_sums(cases[ci].data(), col); const fr_t d = mfma_finish_recoded(col);
        int64_t U[32] = {0}; kstep(unit, d, U); int32_t S[32]; for (int c = 0; c < 32; ++c) S[c] = (int32_t)U[c];
        ++n; if (!ok || !fr_eq(finish(S), finish(cases[ci].data()))) { if (bad < 5) fprintf(stderr, "signed-residue lane: case %zu\n", ci); ++bad; }
    }
    // ---- the same lanes by the byte-domain finish (mfma_word_cols / mfma_finish_bytes: what blk8_lane_rows runs).  The form with 64-bit pairs on every case
    // above (it holds for any |S_c| < 2^24); the form with int32 pairs, the lane rows' own, on every case inside its domain |S_c| <= 9 * 32 * 128 * 128 and on
    // 20 000 random cases and the extreme patterns drawn inside it.  No carry out of word 7, and the digits, taken through the unit fragment's K-step and the
    // canonical finish, give the canonical value of the row.
    {
        const int32_t L9 = 9 * 32 * 128 * 128;
        std::vector<std::vector<int32_t>> narrow;
        for (const auto& s : cases) { bool in = true; for (int32_t v : s) in = in && v <= L9 && v >= -L9; if (in) narrow.push_back(s); }
        narrow.push_back(std::vector<int32_t>(32, L9)); narrow.push_back(std::vector<int32_t>(32, -L9));
        { std::vector<int32_t> a(32), b(32); for (int c = 0; c < 32; ++c) { a[c] = c & 1 ? -L9 : L9; b[c] = -a[c]; } narrow.push_back(a); narrow.push_back(b); }
        for (int32_t k : {-(1 << 16), 1 << 16}) for (int d : {-1, 0, 1}) { std::vector<int32_t> s(32, 0); s[31] = k * 64; s[0] = d; narrow.push_back(s); }
        for (int i = 0; i < 20000; ++i) { std::vector<int32_t> s(32); for (auto& v : s) v = (int32_t)(rnd() % (2 * (uint64_t)L9 + 1)) - L9; narrow.push_back(s); }
        auto check_bytes = [&](const std::vector<int32_t>& s, bool wide, size_t ci) {
            int64_t col[8]; int32_t qh; int64_t carry;
            if (wide) mfma_word_cols_of_sums<true>(s.data(), col); else mfma_word_cols_of_sums<false>(s.data(), col);
            const fr_t d = mfma_finish_bytes(col, &qh, &carry);
            int64_t U[32] = {0}; kstep(unit, d, U); int32_t S[32]; for (int c = 0; c < 32; ++c) S[c] = (int32_t)U[c];
            ++n; if (carry != 0 || qh >= (1 << 19) || qh <= -(1 << 19) || !fr_eq(finish(S), finish(s.data()))) { if (bad < 5) fprintf(stderr, "byte-domain finish (%s pairs): case %zu\n", wide ? "64-bit" : "int32", ci); ++bad; }
        };
        for (size_t ci = 0; ci < cases.size(); ++ci) check_bytes(cases[ci], true, ci);
        for (size_t ci = 0; ci < narrow.size(); ++ci) { check_bytes(narrow[ci], false, ci); check_bytes(narrow[ci], true, ci); }
    }
    // ---- the word-column finish to nine limbs (mfma_word_cols_mad / mfma_words_add_c29 / mfma_finish_words: what the fused full-round rows, the H_q rows and
    // the last block's lane rows run) on every case above, with no constant and with 0 / 1 / r - 1 / a scaled round constant in the columns: no carry out of
    // word 7, limbs 0..7 below 2^29 and the top limb below 2^24, the value inside (r - 2^147, 3 r + 2^147) (top limb in [2^22 - 1, 3 * 2^22]; the cases reach
    // |S_c| = 2^24 - 1, beyond the 23-K-step rows), the canonical form equal to the finishing step's (+ the constant), also by the two conditional
    // subtractions of mfma_finish_words_canonical, and the S-box on the limbs plus a round constant equal to fr_pow5_r29 of the canonical sum.
    for (size_t ci = 0; ci < cases.size(); ++ci) for (int k = -1; k < (ci < ncraft ? 4 : 1); ++k) {
        const int kk = k < 0 ? -1 : ci < ncraft ? k : (int)(ci & 3);
        const fr_t cst = kk <= 0 ? host::h_zero() : kk == 1 ? one : kk == 2 ? rm1 : kc.rc_partial_scaled[ci % 64];
        const fr29_t c29l = fr29_unpack(cst);
        int64_t col[8]; uint32_t l[9]; int32_t qh; int64_t carry;
        mfma_word_cols_mad_of_sums(cases[ci].data(), col, kk < 0 ? nullptr : c29l.l); mfma_finish_words(col, l, &qh, &carry);
        bool ok = carry == 0 && qh < (1 << 20) && qh > -(1 << 20) && l[8] >= (1u << 22) - 1 && l[8] <= 3u * (1u << 22);
        for (int i = 0; i < 8; ++i) ok = ok && l[i] <= FR_M29;
        fr_t z = fr29_pack_reduce<PF>(l); fr_cond_sub<PF>(z.v, 0u); fr_cond_sub<PF>(z.v, 0u);
        const fr_t canon = fr_add<PF>(finish(cases[ci].data()), cst);
        ++n; if (!ok || !fr_eq(z, canon) || !fr_eq(mfma_finish_words_canonical(col), canon)) { if (bad < 5) fprintf(stderr, "word-column finish: case %zu constant %d\n", ci, kk); ++bad; }
        const size_t idx = (ci * 7 + (size_t)(kk + 1) * 17) % (8 * 17);
        ++n; if (!fr_eq(sbox_lazy29(l, &kc.rc_full29[9 * idx]), fr_pow5_r29<PF>(fr_add<PF>(canon, kc.rc_full[idx])))) { if (bad < 5) fprintf(stderr, "S-box on word-finish limbs: case %zu constant %zu\n", ci, idx); ++bad; }
    }
    // ---- the once-per-permutation edges on the row pipeline (poseidon_pair.hpp pair_leaf_round0_mfma, pair_squeeze_row_mfma, and the byte-domain finish on
    // rows of 17 K-steps folded by the multiply-add chain).
    // (i) The leaf's round 0: rows of TWO K-steps — fragments (i, 4), (i, 5) of mds_frag against x4, x5 (r - 1 / 0 / mixed / random) —, the word-column finish to
    // limbs and round 1's S-box with the table (K_i + rc_full[17 + i]) of host_util.hpp leaf_round0_consts, against fr_pow5_r29 of K_i + M[i][4] x4 + M[i][5] x5
    // + rc in the field code; the digit sums inside two K-steps' bound.
    {
        const host::PoseidonConsts tc = host::consts_transcript();
        fr_t init[17], K[17]; uint32_t krc29[17 * 9]; host::leaf_template(init); host::leaf_round0_consts(tc, init, K, krc29);
        for (int rep = 0; rep < 16; ++rep) {
            const fr_t x[2] = {rep == 0 ? rm1 : rep == 1 ? host::h_zero() : rep == 2 ? rm1 : rep == 3 ? host::h_zero() : rand_fr(),
                               rep == 0 ? rm1 : rep == 1 ? host::h_zero() : rep == 2 ? host::h_zero() : rep == 3 ? rm1 : rand_fr()};
            for (int i = 0; i < 17; ++i) {
                int64_t S64[32] = {0};
                for (int e = 0; e < 2; ++e) kstep(&kc.mds_frag[((size_t)i * 17 + 4 + e) * 1024], recode_signed(x[e]), S64);
                int32_t S[32]; for (int c = 0; c < 32; ++c) { if (S64[c] > 2 * 32 * 128 * 128 || S64[c] < -2 * 32 * 128 * 128) { fprintf(stderr, "round-0 row beyond its bound\n"); return 1; } S[c] = (int32_t)S64[c]; }
                int64_t col[8]; uint32_t l[9]; mfma_word_cols_mad_of_sums(S, col); mfma_finish_words(col, l);
                fr_t want = K[i];
                for (int e = 0; e < 2; ++e) want = host::h_add(want, host::h_mul(host::h_mul(tc.mds[(size_t)i * 17 + 4 + e], k20), x[e]));
                ++n; if (!fr_eq(sbox_lazy29(l, &krc29[9 * i]), fr_pow5_r29<PF>(fr_add<PF>(want, tc.rc_full[17 + i])))) { if (bad < 5) fprintf(stderr, "leaf round 0: rep %d row %d\n", rep, i); ++bad; }
            }
        }
    }
    // (ii) The squeeze row: row 0 of mds_frag, 17 K-steps, the word-column fold and the canonical finish against the row0 dot product in the field code.
    for (int rep = 0; rep < 12; ++rep) {
        fr_t st[17]; int64_t S64[32] = {0};
        for (int e = 0; e < 17; ++e) st[e] = rep == 0 ? rm1 : rep == 1 ? host::h_zero() : rep == 2 ? ((e & 1) ? rm1 : host::h_zero()) : rep == 3 ? ((e & 1) ? host::h_zero() : rm1) : rand_fr();
        fr_t want = host::h_zero();
        for (int e = 0; e < 17; ++e) { kstep(&kc.mds_frag[(size_t)e * 1024], recode_signed(st[e]), S64); want = host::h_add(want, host::h_mul(host::h_mul(kc.row0[e], k20), st[e])); }
        int32_t S[32]; for (int c = 0; c < 32; ++c) { if (S64[c] > 17 * 32 * 128 * 128 || S64[c] < -17 * 32 * 128 * 128) { fprintf(stderr, "squeeze row beyond its bound\n"); return 1; } S[c] = (int32_t)S64[c]; }
        int64_t col[8]; mfma_word_cols_mad_of_sums(S, col);
        ++n; if (!fr_eq(mfma_finish_words_canonical(col), want)) { if (bad < 5) fprintf(stderr, "squeeze row: rep %d\n", rep); ++bad; }
    }
    // (iii) The entry to the partial rounds: the byte-domain finish on columns folded by the multiply-add chain, rows of 17 K-steps — the extremes
    // |S_c| = 8 912 896, every case above inside that domain (k r +- 1 and k 2^254 +- 1 up to |k| = 2^17 among them) and 20 000 random rows: no carry out of word
    // 7, and the digits, taken through the unit fragment's K-step and the canonical finish, give the canonical value of the row.
    {
        const int32_t L17 = 17 * 32 * 128 * 128;
        std::vector<std::vector<int32_t>> rows;
        rows.push_back(std::vector<int32_t>(32, L17)); rows.push_back(std::vector<int32_t>(32, -L17));
        { std::vector<int32_t> a(32), b(32); for (int c = 0; c < 32; ++c) { a[c] = c & 1 ? -L17 : L17; b[c] = -a[c]; } rows.push_back(a); rows.push_back(b); }
        for (const auto& s : cases) { bool in = true; for (int32_t v : s) in = in && v <= L17 && v >= -L17; if (in) rows.push_back(s); }
        for (int i = 0; i < 20000; ++i) { std::vector<int32_t> s(32); for (auto& v : s) v = (int32_t)(rnd() % (2 * (uint64_t)L17 + 1)) - L17; rows.push_back(s); }
        for (size_t ci = 0; ci < rows.size(); ++ci) {
            int64_t col[8]; int32_t qh; int64_t carry;
            mfma_word_cols_mad_of_sums(rows[ci].data(), col);
            const fr_t d = mfma_finish_bytes(col, &qh, &carry);
            int64_t U[32] = {0}; kstep(unit, d, U); int32_t S[32]; for (int c = 0; c < 32; ++c) S[c] = (int32_t)U[c];
            ++n; if (carry != 0 || qh >= (1 << 19) || qh <= -(1 << 19) || !fr_eq(finish(S), finish(rows[ci].data()))) { if (bad < 5) fprintf(stderr, "byte-domain finish on multiply-add columns: case %zu\n", ci); ++bad; }
        }
    }
    printf("{\"check\": \"residue tables and finishing step against the portable field code\", \"cases\": %ld, \"mismatches\": %ld}\n", n, bad);
    return bad ? 1 : 0;
}
