// stark_mlwe_amd/csrc/host_util.hpp — host-side scalar logic of the product (no device code).
//
// What a Rust host would get from `blake3`, `rand::StdRng` and arkworks when it drives the C-ABI:
//   * BLAKE3 (hash mode)            -> Poseidon constant derivation (utils/src/lib.rs:16-22)
//   * ChaCha12 block function        -> `StdRng::from_seed` + `gen::<u64>()` (fri.rs:66-71,185-186)
//   * from_le_bytes_mod_order, tags  -> transcript framing constants (transcript/src/lib.rs:13-41)
//   * constant tables for the kernels: LU factors of the MDS matrix and the sparse factorisation of
//     the partial rounds (algebraically identical to the dense rounds of poseidon/src/lib.rs:31-68);
//     for t = 17 the int8 residue tables of the matrix-core products, those of the 8-round partial
//     blocks in two families: unscaled (host checks) and with the S-box chain scaled by lambda_q,
//     which is what the device gets (KernelConsts blk8_* / blk8s_*).
// Written independently of oracle/ (which is test infrastructure and is never linked here).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "fr.hpp"
#include "fr29.hpp"
#include "poseidon_params.hpp"

namespace stark {
namespace host {

// ------------------------------------------------------------------------------------------------
// BLAKE3, hash mode, arbitrary length, 32-byte digest (spec: chunks of 1024 B, blocks of 64 B,
// binary tree of chaining values).  Compact recursive formulation.
// ------------------------------------------------------------------------------------------------
struct Blake3 {
    static constexpr uint32_t kIV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
    enum : uint32_t { F_CHUNK_START = 1, F_CHUNK_END = 2, F_PARENT = 4, F_ROOT = 8 };
    static uint32_t ror(uint32_t x, unsigned n) { return (x >> n) | (x << (32 - n)); }
    static void mix(uint32_t* v, int a, int b, int c, int d, uint32_t x, uint32_t y) {
        v[a] += v[b] + x; v[d] = ror(v[d] ^ v[a], 16); v[c] += v[d]; v[b] = ror(v[b] ^ v[c], 12);
        v[a] += v[b] + y; v[d] = ror(v[d] ^ v[a], 8);  v[c] += v[d]; v[b] = ror(v[b] ^ v[c], 7);
    }
    // full 16-word compression output
    static void compress(const uint32_t h[8], const uint8_t block[64], uint32_t blen, uint64_t ctr, uint32_t flags, uint32_t out[16]) {
        static const uint8_t sched[7][16] = {
            {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8},
            {3, 4, 10, 12, 13, 2, 7, 14, 6, 5, 9, 0, 11, 15, 8, 1}, {10, 7, 12, 9, 14, 3, 13, 15, 4, 0, 11, 2, 5, 8, 1, 6},
            {12, 13, 9, 11, 15, 10, 14, 8, 7, 2, 5, 3, 0, 1, 6, 4}, {9, 14, 11, 5, 8, 12, 15, 1, 13, 3, 0, 10, 2, 6, 4, 7},
            {11, 15, 5, 0, 1, 9, 8, 6, 14, 10, 2, 12, 3, 4, 7, 13}};
        uint32_t m[16], v[16];
        for (int i = 0; i < 16; ++i) m[i] = (uint32_t)block[4 * i] | (uint32_t)block[4 * i + 1] << 8 | (uint32_t)block[4 * i + 2] << 16 | (uint32_t)block[4 * i + 3] << 24;
        for (int i = 0; i < 8; ++i) v[i] = h[i];
        for (int i = 0; i < 4; ++i) v[8 + i] = kIV[i];
        v[12] = (uint32_t)ctr; v[13] = (uint32_t)(ctr >> 32); v[14] = blen; v[15] = flags;
        for (int r = 0; r < 7; ++r) {
            const uint8_t* s = sched[r];
            mix(v, 0, 4, 8, 12, m[s[0]], m[s[1]]);   mix(v, 1, 5, 9, 13, m[s[2]], m[s[3]]);
            mix(v, 2, 6, 10, 14, m[s[4]], m[s[5]]);  mix(v, 3, 7, 11, 15, m[s[6]], m[s[7]]);
            mix(v, 0, 5, 10, 15, m[s[8]], m[s[9]]);  mix(v, 1, 6, 11, 12, m[s[10]], m[s[11]]);
            mix(v, 2, 7, 8, 13, m[s[12]], m[s[13]]); mix(v, 3, 4, 9, 14, m[s[14]], m[s[15]]);
        }
        for (int i = 0; i < 8; ++i) { out[i] = v[i] ^ v[i + 8]; out[i + 8] = v[i + 8] ^ h[i]; }
    }
    struct Node { uint32_t h[8]; uint8_t block[64]; uint32_t blen; uint64_t ctr; uint32_t flags; };
    static void cv_of(const Node& n, uint32_t extra, uint32_t cv[8]) { uint32_t o[16]; compress(n.h, n.block, n.blen, n.ctr, n.flags | extra, o); memcpy(cv, o, 32); }
    static Node chunk_node(const uint8_t* p, size_t len, uint64_t index) {
        Node n; memcpy(n.h, kIV, 32); n.ctr = index;
        size_t off = 0; bool first = true;
        while (len - off > 64) {
            uint32_t o[16]; compress(n.h, p + off, 64, index, first ? F_CHUNK_START : 0, o); memcpy(n.h, o, 32);
            off += 64; first = false;
        }
        memset(n.block, 0, 64); memcpy(n.block, p + off, len - off); n.blen = (uint32_t)(len - off);
        n.flags = (first ? F_CHUNK_START : 0) | F_CHUNK_END;
        return n;
    }
    // node covering p[0..len) whose first chunk has index `index` (left subtree = largest power of two of chunks < total)
    static Node subtree(const uint8_t* p, size_t len, uint64_t index) {
        if (len <= 1024) return chunk_node(p, len, index);
        size_t chunks = (len + 1023) / 1024, left = 1; while (left * 2 < chunks) left *= 2;
        Node l = subtree(p, left * 1024, index), r = subtree(p + left * 1024, len - left * 1024, index + left);
        Node n; memcpy(n.h, kIV, 32); n.ctr = 0; n.blen = 64; n.flags = F_PARENT;
        uint32_t a[8], b[8]; cv_of(l, 0, a); cv_of(r, 0, b);
        for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) { n.block[4 * i + j] = (uint8_t)(a[i] >> (8 * j)); n.block[32 + 4 * i + j] = (uint8_t)(b[i] >> (8 * j)); }
        return n;
    }
    static void hash(const uint8_t* p, size_t len, uint8_t out[32]) {
        Node root = subtree(p, len, 0);
        if (root.flags & F_PARENT) root.ctr = 0;
        uint32_t cv[8]; cv_of(root, F_ROOT, cv);
        for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(cv[i] >> (8 * j));
    }
};

// ------------------------------------------------------------------------------------------------
// ChaCha12 keystream as consumed by rand 0.8.5 `StdRng` (64-bit block counter, zero stream id).
// ------------------------------------------------------------------------------------------------
struct ChaCha12Rng {
    uint32_t st[16]; uint32_t out[16]; unsigned have = 0;
    explicit ChaCha12Rng(const uint8_t seed[32]) {
        st[0] = 0x61707865u; st[1] = 0x3320646eu; st[2] = 0x79622d32u; st[3] = 0x6b206574u;
        for (int i = 0; i < 8; ++i) st[4 + i] = (uint32_t)seed[4 * i] | (uint32_t)seed[4 * i + 1] << 8 | (uint32_t)seed[4 * i + 2] << 16 | (uint32_t)seed[4 * i + 3] << 24;
        st[12] = st[13] = st[14] = st[15] = 0;
    }
    static uint32_t rol(uint32_t x, unsigned n) { return (x << n) | (x >> (32 - n)); }
    void block() {
        uint32_t x[16]; memcpy(x, st, 64);
        auto Q = [&](int a, int b, int c, int d) {
            x[a] += x[b]; x[d] = rol(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = rol(x[b] ^ x[c], 12);
            x[a] += x[b]; x[d] = rol(x[d] ^ x[a], 8);  x[c] += x[d]; x[b] = rol(x[b] ^ x[c], 7); };
        for (int i = 0; i < 6; ++i) { Q(0, 4, 8, 12); Q(1, 5, 9, 13); Q(2, 6, 10, 14); Q(3, 7, 11, 15); Q(0, 5, 10, 15); Q(1, 6, 11, 12); Q(2, 7, 8, 13); Q(3, 4, 9, 14); }
        for (int i = 0; i < 16; ++i) out[i] = x[i] + st[i];
        if (++st[12] == 0) ++st[13];
        have = 16;
    }
    uint32_t next_u32() { if (!have) block(); return out[16 - have--]; }
    uint64_t next_u64() { uint64_t lo = next_u32(), hi = next_u32(); return lo | hi << 32; }   // gen::<u64>()
};

// ------------------------------------------------------------------------------------------------
// Host field helpers on fr_t (Pallas Fr is the prover field).
// ------------------------------------------------------------------------------------------------
typedef PallasFr PF;
inline fr_t h_one() { return fr_one<PF>(); }
inline fr_t h_zero() { return fr_zero<PF>(); }
inline fr_t h_mul(const fr_t& a, const fr_t& b) { return fr_mul<PF>(a, b); }
inline fr_t h_add(const fr_t& a, const fr_t& b) { return fr_add<PF>(a, b); }
inline fr_t h_sub(const fr_t& a, const fr_t& b) { return fr_sub<PF>(a, b); }
inline fr_t h_u64(uint64_t x) { return fr_from_u64<PF>(x); }
// int_le(bytes[0..n)) mod r, n <= 64, as a Montgomery element (F::from_le_bytes_mod_order).
inline fr_t h_from_le_bytes_mod_order(const uint8_t* b, size_t n) {
    // Horner over 32-bit words, most significant first: acc = acc * 2^32 + w.
    fr_t acc = h_zero(); const fr_t two32 = h_u64(1ull << 32);
    size_t nw = (n + 3) / 4;
    for (size_t k = nw; k-- > 0;) {
        uint32_t w = 0; for (size_t j = 0; j < 4; ++j) if (4 * k + j < n) w |= (uint32_t)b[4 * k + j] << (8 * j);
        acc = h_add(h_mul(acc, two32), h_u64(w));
    }
    return acc;
}
// serialize_uncompressed / serialize_compressed of Fp: 32-byte LE canonical.
inline void h_to_bytes_le(const fr_t& a, uint8_t out[32]) {
    fr_t c = fr_to_canonical<PF>(a);
    for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(c.v[i] >> (8 * j));
}
// utils/src/lib.rs:16-22  fr_from_hash(tag, data).
inline fr_t h_fr_from_hash(const char* tag, const std::vector<uint8_t>& data) {
    std::vector<uint8_t> buf(tag, tag + strlen(tag)); buf.insert(buf.end(), data.begin(), data.end());
    uint8_t d[32]; Blake3::hash(buf.data(), buf.size(), d);
    uint8_t wide[64]; memset(wide, 0, 64); memcpy(wide, d, 32);            // utils/src/lib.rs:7-13
    return h_from_le_bytes_mod_order(wide, 64);
}
// transcript/src/lib.rs:13-29  domain_tag_to_field  /  :32-41 bytes_to_field_words.
inline fr_t h_tag(const char* s) {
    size_t n = strlen(s);
    if (n <= 32) { uint8_t le[32] = {0}; memcpy(le, s, n); return h_from_le_bytes_mod_order(le, 32); }
    fr_t acc = h_zero();
    for (size_t off = 0; off < n; off += 32) { uint8_t le[32] = {0}; size_t c = n - off < 32 ? n - off : 32; memcpy(le, s + off, c); acc = h_add(acc, h_from_le_bytes_mod_order(le, 32)); }
    return acc;
}
inline std::vector<fr_t> h_words(const char* s) {
    std::vector<fr_t> out; size_t n = strlen(s);
    for (size_t off = 0; off < n; off += 31) { uint8_t le[32] = {0}; size_t c = n - off < 31 ? n - off : 31; memcpy(le, s + off, c); out.push_back(h_from_le_bytes_mod_order(le, 32)); }
    return out;
}
// The frame of tr_hash_fields_tagged(tag, xs) (fri.rs:28-35 over transcript/src/lib.rs:55-101): the absorbed stream is
// [AB, w("FRI/FS"), AB, words(tag)..] || xs || [CH, AB, w("out")] under the capacity FSv1-TRANSCRIPT-INIT.  frame = prefix || suffix;
// returns the prefix length.
inline int tr_hash_frame(const char* tag, std::vector<fr_t>& frame) {
    const fr_t AB = h_tag("FSv1-ABSORB-BYTES"), CH = h_tag("FSv1-CHALLENGE");
    frame.clear();
    frame.push_back(AB); for (auto& w : h_words("FRI/FS")) frame.push_back(w);
    frame.push_back(AB); for (auto& w : h_words(tag)) frame.push_back(w);
    const int np = (int)frame.size();
    frame.push_back(CH); frame.push_back(AB); for (auto& w : h_words("out")) frame.push_back(w);
    return np;
}

// ------------------------------------------------------------------------------------------------
// Poseidon constants in the reference's form (poseidon/src/lib.rs:104-114, 176-216, 318-356).
// ------------------------------------------------------------------------------------------------
struct PoseidonConsts {
    int t = 0, rf = 0, rp = 0;
    std::vector<fr_t> mds;         // t*t row-major  mds[i*t+j]
    std::vector<fr_t> rc_full;     // rf*t
    std::vector<fr_t> rc_partial;  // rp
};
inline void put64(std::vector<uint8_t>& v, uint64_t x) { for (int j = 0; j < 8; ++j) v.push_back((uint8_t)(x >> (8 * j))); }
inline PoseidonConsts derive_consts(const std::string& seed, int t, int rf, int rp) {
    PoseidonConsts c; c.t = t; c.rf = rf; c.rp = rp;
    c.mds.resize((size_t)t * t); c.rc_full.resize((size_t)rf * t); c.rc_partial.resize(rp);
    for (int i = 0; i < t; ++i) for (int j = 0; j < t; ++j) { std::vector<uint8_t> d; put64(d, i); put64(d, j); d.insert(d.end(), seed.begin(), seed.end()); c.mds[(size_t)i * t + j] = h_fr_from_hash("POSEIDON-MDS", d); }
    for (int r = 0; r < rf; ++r) for (int i = 0; i < t; ++i) { std::vector<uint8_t> d; put64(d, r); put64(d, i); d.insert(d.end(), seed.begin(), seed.end()); c.rc_full[(size_t)r * t + i] = h_fr_from_hash("POSEIDON-RC-FULL", d); }
    for (int r = 0; r < rp; ++r) { std::vector<uint8_t> d; put64(d, r); d.insert(d.end(), seed.begin(), seed.end()); c.rc_partial[r] = h_fr_from_hash("POSEIDON-RC-PART", d); }
    return c;
}
inline int width_for_arity(size_t arity) { return arity <= 8 ? 9 : arity <= 16 ? 17 : arity <= 32 ? 33 : arity <= 64 ? 65 : arity <= 128 ? 129 : -1; }   // poseidon/src/lib.rs:155-166
inline int rp_for_width(int t) { switch (t) { case 9: return 60; case 17: return 64; case 33: return 68; case 65: return 76; case 129: return 84; default: return -1; } }  // :121-128
inline PoseidonConsts consts_for_width(int t) {          // poseidon_params_for_width + seed_for_t (:120-146,168-174)
    std::string seed = "POSEIDON-PALLAS-T"; for (int j = 0; j < 8; ++j) seed.push_back((char)(((uint64_t)t >> (8 * j)) & 0xff));
    return derive_consts(seed, t, 8, rp_for_width(t));
}
inline PoseidonConsts consts_transcript() { return derive_consts("POSEIDON-T17-X5-TRANSCRIPT", 17, 8, 64); }   // transcript/src/lib.rs:44-46

// ------------------------------------------------------------------------------------------------
// Kernel-form constants: in-place LU factors and the sparse partial-round factorisation.
//
// Partial rounds  s <- M * S_r(s)  (S_r touches lane 0 only) are rewritten as
//     s <- A_R S_R  A_{R-1} S_{R-1} ... A_1 S_1  (B_1 s)
// with M_R = M, M_k = A_k B_k, B_k = diag(1, Mhat_k), A_k = [[m00, v Mhat_k^-1], [w, I]],
// M_{k-1} = B_k M.  B_1 is merged into the MDS of the last first-half full round (mds_pre = B_1 M).
// B_k commutes with S_k, so the composition is unchanged: exact field arithmetic => identical bits.
// A dense matrix is applied in place as L*(U*x): U top-down, then unit-lower L bottom-up.
// ------------------------------------------------------------------------------------------------
struct KernelConsts {
    int t = 0, rf = 0, rp = 0;
    std::vector<fr_t> rc_full, rc_partial;
    std::vector<fr_t> lu, lu_pre;       // t*t each: U on/above the diagonal, strict lower = L (unit diagonal implied)
    std::vector<fr_t> row0;             // t: mds[0][*] (final round when only lane 0 is squeezed)
    std::vector<fr_t> sparse;           // rp*(2t-1): [a, u_1..u_{t-1}, w_1..w_{t-1}] in application order
    std::vector<fr_t> mds;              // t*t reference form (cooperative kernel: full rounds)
    std::vector<fr_t> mds_pre;          // t*t dense B_1*M (cooperative kernel: last first-half full round)
    std::vector<fr_t> gamma;            // (rp/4)*6: blocks of 4 partial rounds, gamma[q(q-1)/2+p] = sum_j u_{q,j} w_{p,j} (p < q)
    // the multiplier tables of every dot product again, as nine 29-bit limbs of c*2^261 mod r per entry (fr29.hpp)
    std::vector<uint32_t> lu29, lu_pre29, row0_29, sparse29, gamma29;
    std::vector<uint32_t> mds29, mds_pre29;   // dense forms for the one-wave kernel (every entry meets an S-box output: all scaled)
    std::vector<uint32_t> rc_full29;          // rf*t*9: fr29_unpack of every full-round constant as stored (an addend, not a multiplier: no R' factor, no scale)
    // t = 17 only: the dense matrices as int8 MFMA operand fragments (signed radix-256 digits of the residue tables), see mfma_frags
    std::vector<int8_t> mds_frag, mds_pre_frag;
    // t = 17 only: the partial rounds UNROLLED over all rp rounds for the five-wave latency kernel (poseidon_chain.hpp):
    //     X_{q+1} = c_{q+1} + sum_j u_{q,j} s_j^(0) + a_q y_q + sum_{p<q} Gamma_{q,p} y_p,   y_q = X_q^5,   Gamma_{q,p} = sum_j u_{q,j} w_{p,j}
    // Every entry multiplies a y that reaches it through THREE Montgomery steps by 2^261 on operands carrying 2^256, so it is stored as
    // nine 29-bit limbs of c * 2^25 * 2^256 mod r (= c * (2^261)^5 / (2^256)^4): the product lands back in the 2^256 domain.
    //   chain_a [rp][64]      lane 16 + c: limb c of a_q; lane 32 + c: limb c of Gamma_{q+1,q} (0 for the last round); other lanes 0
    //   chain_g [rp][9][64]   limb i of Gamma_{q,p} for lane q >= p + 2, else 0   (p = first index)
    //   chain_w [rp][t-1][9]  w_{p,j}
    std::vector<uint32_t> chain_a, chain_g, chain_w;
    // t = 17 and rp a multiple of 8: the partial rounds in BLOCKS OF 8 whose two long products run on the matrix cores (poseidon_pair.hpp pair_block8).
    // Inside block b (rounds 8b .. 8b+7), with the lanes s_j at their block-start values and y_q = (X_q + c_q)^5:
    //     X_{q+1} = E_q + a_q y_q + sum_{p<q} Gamma_{q,p} y_p,   E_q = sum_j u_{q,j} s_j,   Gamma_{q,p} = sum_j u_{q,j} w_{p,j};   s_j <- s_j + sum_p w_{p,j} y_p.
    //   blk8_efrag [rp/8][8][16]  fragment (mfma_frag_of) of u_{q,j}, UNSCALED: its inputs are lanes in stored form
    //   blk8_lfrag [rp/8][16][8]  fragment of w_{p,j} * 2^20 (its inputs are fr_pow5_r29 outputs, as in the full rounds), lane-major: row j = 1..16, then p;
    //                             after the last block ONE fragment of the constant 1: the K-step that adds the lane's own stored value
    //   blk8_gfrag [rp/8][28]     fragment of Gamma_{q,p} * 2^20 at q (q - 1) / 2 + p: the y_p enter row q's tile as q further K-steps (H_q = E_q + sum Gamma y_p)
    //   gamma8_29  [rp/8][28][9]  the same Gamma_{q,p} scaled like gamma29: host checks and tools only, not uploaded
    std::vector<int8_t> blk8_efrag, blk8_lfrag, blk8_gfrag;
    std::vector<uint32_t> gamma8_29;
    // The same blocks with the chain SCALED, the family the device gets: wave X carries lambda_q X_q instead of X_q, with lambda_0 = 1 and
    //     lambda_{q+1} = lambda_q^5 kappa / a      (kappa = 2^-20, fr_pow5_r29's scale; a = M[0][0], every round's a_q; q runs over all rp rounds),
    // so that yt_q = fr_pow5_r29(lambda_q X_q + lambda_q c_q) = kappa lambda_q^5 y_q enters the next chain value with coefficient exactly 1:
    //     lambda_{q+1} X_{q+1} = yt_q + lambda_{q+1} ( E_q + sum_{p<q} Gamma_{q,p} y_p ).
    // No a_q y_q product is left in a round; every lambda sits on a constant left factor (exact field arithmetic: identical bits):
    //   blk8_lambda        [rp + 1]      lambda_q, host side only (tests, tools)
    //   blk8s_efrag        [rp/8][8][16] fragment of u_{q,j} lambda_{q+1}
    //   blk8s_lfrag        [rp/8][16][8] fragment of w_{p,j} / (kappa lambda_p^5): its inputs are the yt_p.  No unit fragment of its own: blk8_lfrag's serves both
    //   blk8s_gfrag        [rp/8][28]    fragment of Gamma_{q,p} lambda_{q+1} / (kappa lambda_p^5)
    //   rc_partial_scaled  [rp]          lambda_q c_q, stored form
    //   rc_partial_scaled29 [rp + 1][9]  the same as nine 29-bit limbs of the stored value (fr29_unpack, like rc_full29: an addend), entry rp zero: the initial
    //                                    columns of the finish of the row that round q consumes (mfma_digits.hpp); after the last round no constant follows
    //   blk8_unscale29     [9]           1 / lambda_rp as a multiplier-table entry (fr29_const_from, no 2^20: it meets the chain value, not an S-box output):
    //                                    one product per permutation brings X_rp back
    // The fragments are still signed radix-256 digits of residues in [0, r): the digit-sum bounds of the unscaled family hold unchanged.
    // lambda needs M[0][0] != 0.  Every set that gets this far has it: the in-place LU of M (lu_pack, no pivoting) refuses a zero M[0][0] first, and such a
    // set is not ok at all.
    std::vector<fr_t> blk8_lambda, rc_partial_scaled;
    std::vector<int8_t> blk8s_efrag, blk8s_lfrag, blk8s_gfrag;
    std::vector<uint32_t> blk8_unscale29, rc_partial_scaled29;
    bool ok = false;
};
// scaled(i) == true: the entry multiplies an S-box output, which fr_pow5_r29 delivers as x^5 / 2^20 (fr29.hpp)
template <class Pred> inline std::vector<uint32_t> to_radix29(const std::vector<fr_t>& v, Pred scaled) {
    const fr_t k = fr_from_u64<PF>(1ull << FR29_SBOX_SHIFT);
    std::vector<uint32_t> o(v.size() * 9);
    for (size_t i = 0; i < v.size(); ++i) fr29_const_from<PF>(scaled(i) ? fr_mul<PF>(v[i], k) : v[i], &o[9 * i]);
    return o;
}
// A-operand fragments of v_mfma_i32_32x32x32_i8 for y = M * x with x an S-box output (poseidon_pair.hpp pair_mds_sbox_mfma): RESIDUE TABLES.
// The left factor is constant, so the reduction mod r is done here, once per parameter set.  For entry (i, e) and input digit position b,
//     C[i][e][b] = ( M[i][e] * 2^20 * 256^b ) mod r        a plain integer in [0, r)   (2^20: fr_pow5_r29's scale)
// written in SIGNED radix-256 digits d[0..31] in [-128, 127] (add 0x80 to every byte with carries, subtract 0x80 from every digit; C < r
// keeps the top byte below 0x80, so no 33rd digit).  With xd_e the signed digits of the STORED x_e (x * 2^256 mod r),
//     sum_{e,b} xd_e[b] * C[i][e][b]  ==  2^20 * sum_e M[i][e] * stored(x_e)  ==  stored((M x)_i)      (mod r),
// so the digit sums S[c] = sum_{e,b} d_{i,e,b}[c] * xd_e[b], c = 0..31, are ONE 32-row tile of a dense int8 product (no structural zeros), and
// sum_c S[c] 256^c needs no Montgomery step, only a reduction of its top bits.  Fragment (i*t + e) holds, for lane l (tile row = output digit
// c = l & 31, K half kh = l >> 5), the 16 bytes j -> d_{i,e,16 kh + j}[c]: the left operand of the K-step of element e.  t*t*64*16 bytes.
// One fragment (1 KiB): g is the Montgomery form of the coefficient, its scale included.
inline void mfma_frag_of(fr_t g, int8_t* out) {
    const fr_t k256 = fr_from_u64<PF>(256);
    int8_t d[32][32];                                                         // d[b][c]
    for (int b = 0; b < 32; ++b, g = h_mul(g, k256)) {                        // Montgomery form of coefficient * 256^b, b = 0, 1, ...
        const fr_t c = fr_to_canonical<PF>(g); int cy = 0;
        for (int k = 0; k < 32; ++k) { const int v = (int)((c.v[k >> 2] >> (8 * (k & 3))) & 0xff) + 0x80 + cy; cy = v >> 8; d[b][k] = (int8_t)((v & 0xff) - 0x80); }
    }
    for (int l = 0; l < 64; ++l) for (int j = 0; j < 16; ++j) out[(size_t)l * 16 + j] = d[16 * (l >> 5) + j][l & 31];
}
// rows x cols fragments of a row-major matrix, every entry times `scale` (Montgomery form; fr_one for none)
inline std::vector<int8_t> mfma_frags(const fr_t* mat, int rows, int cols, const fr_t& scale) {
    std::vector<int8_t> out((size_t)rows * cols * 64 * 16, 0);
    for (int i = 0; i < rows; ++i) for (int e = 0; e < cols; ++e) mfma_frag_of(h_mul(mat[(size_t)i * cols + e], scale), &out[((size_t)i * cols + e) * 64 * 16]);
    return out;
}
inline std::vector<int8_t> mfma_frags(const std::vector<fr_t>& mat, int t) { return mfma_frags(mat.data(), t, t, fr_from_u64<PF>(1ull << FR29_SBOX_SHIFT)); }
// Gauss-Jordan inverse of an n x n matrix (row-major); returns false when singular.
inline bool mat_inverse(std::vector<fr_t> a, int n, std::vector<fr_t>& inv) {
    inv.assign((size_t)n * n, h_zero()); for (int i = 0; i < n; ++i) inv[(size_t)i * n + i] = h_one();
    for (int c = 0; c < n; ++c) {
        int p = -1; for (int r = c; r < n; ++r) if (!fr_is_zero(a[(size_t)r * n + c])) { p = r; break; }
        if (p < 0) return false;
        if (p != c) for (int k = 0; k < n; ++k) { std::swap(a[(size_t)p * n + k], a[(size_t)c * n + k]); std::swap(inv[(size_t)p * n + k], inv[(size_t)c * n + k]); }
        fr_t pi = fr_inv<PF>(a[(size_t)c * n + c]);
        for (int k = 0; k < n; ++k) { a[(size_t)c * n + k] = h_mul(a[(size_t)c * n + k], pi); inv[(size_t)c * n + k] = h_mul(inv[(size_t)c * n + k], pi); }
        for (int r = 0; r < n; ++r) if (r != c) {
            fr_t f = a[(size_t)r * n + c]; if (fr_is_zero(f)) continue;
            for (int k = 0; k < n; ++k) { a[(size_t)r * n + k] = h_sub(a[(size_t)r * n + k], h_mul(f, a[(size_t)c * n + k])); inv[(size_t)r * n + k] = h_sub(inv[(size_t)r * n + k], h_mul(f, inv[(size_t)c * n + k])); }
        }
    }
    return true;
}
// Doolittle LU without pivoting, packed in place; false on a zero pivot.
inline bool lu_pack(const std::vector<fr_t>& m, int n, std::vector<fr_t>& lu) {
    lu = m;
    for (int k = 0; k < n; ++k) {
        if (fr_is_zero(lu[(size_t)k * n + k])) return false;
        fr_t pi = fr_inv<PF>(lu[(size_t)k * n + k]);
        for (int i = k + 1; i < n; ++i) {
            fr_t f = h_mul(lu[(size_t)i * n + k], pi); lu[(size_t)i * n + k] = f;
            for (int j = k + 1; j < n; ++j) lu[(size_t)i * n + j] = h_sub(lu[(size_t)i * n + j], h_mul(f, lu[(size_t)k * n + j]));
        }
    }
    return true;
}
inline KernelConsts make_kernel_consts(const PoseidonConsts& c) {
    KernelConsts k; k.t = c.t; k.rf = c.rf; k.rp = c.rp; k.rc_full = c.rc_full; k.rc_partial = c.rc_partial; k.mds = c.mds;
    const int t = c.t, n = t - 1;
    k.row0.assign(c.mds.begin(), c.mds.begin() + t);
    std::vector<fr_t> cur = c.mds;                    // M_R
    k.sparse.assign((size_t)c.rp * (2 * t - 1), h_zero());
    for (int r = c.rp - 1; r >= 0; --r) {
        std::vector<fr_t> hat((size_t)n * n), hinv;
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) hat[(size_t)i * n + j] = cur[(size_t)(i + 1) * t + (j + 1)];
        if (!mat_inverse(hat, n, hinv)) return k;
        fr_t* sp = &k.sparse[(size_t)r * (2 * t - 1)];
        sp[0] = cur[0];
        for (int j = 0; j < n; ++j) { fr_t acc = h_zero(); for (int q = 0; q < n; ++q) acc = h_add(acc, h_mul(cur[(size_t)0 * t + (q + 1)], hinv[(size_t)q * n + j])); sp[1 + j] = acc; }   // u = v * hat^-1
        for (int i = 0; i < n; ++i) sp[t + i] = cur[(size_t)(i + 1) * t + 0];                                                                                                        // w
        // next = B * M : row 0 of M unchanged; rows 1.. = hat * M[1:, :]
        std::vector<fr_t> nxt((size_t)t * t);
        for (int j = 0; j < t; ++j) nxt[j] = c.mds[j];
        for (int i = 0; i < n; ++i) for (int j = 0; j < t; ++j) { fr_t acc = h_zero(); for (int q = 0; q < n; ++q) acc = h_add(acc, h_mul(hat[(size_t)i * n + q], c.mds[(size_t)(q + 1) * t + j])); nxt[(size_t)(i + 1) * t + j] = acc; }
        cur.swap(nxt);
    }
    // cur == B_1 * M == mds_pre
    // Blocks of 4 partial rounds: within a block the lanes 1..t-1 are read at their block-start value and
    // the S-box outputs x_p enter later rounds through gamma_{q,p} = sum_j u_{q,j} * w_{p,j}  (p < q).
    if (c.rp % 4) return k;
    k.gamma.assign((size_t)(c.rp / 4) * 6, h_zero());
    for (int b = 0; b < c.rp / 4; ++b)
        for (int q = 1; q < 4; ++q)
            for (int p2 = 0; p2 < q; ++p2) {
                const fr_t* uq = &k.sparse[(size_t)(4 * b + q) * (2 * t - 1)];
                const fr_t* wp = &k.sparse[(size_t)(4 * b + p2) * (2 * t - 1)];
                fr_t acc = h_zero();
                for (int j = 1; j < t; ++j) acc = h_add(acc, h_mul(uq[j], wp[t - 1 + j]));
                k.gamma[(size_t)b * 6 + q * (q - 1) / 2 + p2] = acc;
            }
    if (!lu_pack(c.mds, t, k.lu)) return k;
    if (!lu_pack(cur, t, k.lu_pre)) return k;
    k.mds_pre = cur;
    // radix-2^29 tables.  Scaled by 2^20: what meets an S-box output — U of every L*U (entries on/above the diagonal;
    // L acts on U's result), row 0 of M, a_k and w_k of the sparse rounds (u_k meets the lanes, not an S-box output), gamma.
    const auto upper = [t](size_t i) { return (int)(i % t) >= (int)(i / t); };
    const auto all = [](size_t) { return true; };
    const auto a_and_w = [t](size_t i) { const int c = (int)(i % (2 * t - 1)); return c == 0 || c >= t; };
    k.lu29 = to_radix29(k.lu, upper); k.lu_pre29 = to_radix29(k.lu_pre, upper); k.row0_29 = to_radix29(k.row0, all);
    k.sparse29 = to_radix29(k.sparse, a_and_w); k.gamma29 = to_radix29(k.gamma, all);
    k.mds29 = to_radix29(k.mds, all); k.mds_pre29 = to_radix29(k.mds_pre, all);
    k.rc_full29.resize(k.rc_full.size() * 9);
    for (size_t i = 0; i < k.rc_full.size(); ++i) { const fr29_t u = fr29_unpack(k.rc_full[i]); for (int j = 0; j < 9; ++j) k.rc_full29[9 * i + j] = u.l[j]; }
    if (t == 17) { k.mds_frag = mfma_frags(k.mds, t); k.mds_pre_frag = mfma_frags(k.mds_pre, t); }      // the wave-pair kernels' full rounds (poseidon_pair.hpp)
    if (t == 17 && c.rp % 8 == 0) {                                             // blocks of 8 partial rounds on the matrix cores (poseidon_pair.hpp)
        const int nb = c.rp / 8, w = 2 * t - 1;
        const fr_t s20 = fr_from_u64<PF>(1ull << FR29_SBOX_SHIFT);
        std::vector<fr_t> g8((size_t)nb * 28, h_zero()), um((size_t)8 * n), wm((size_t)n * 8);
        // the scaled chain: lambda_q and yinv_q = 1 / (kappa lambda_q^5), the factor that turns yt_q back into y_q
        const fr_t kappa = fr_inv<PF>(s20), a_inv = fr_inv<PF>(c.mds[0]);
        std::vector<fr_t> yinv(c.rp), ums((size_t)8 * n), wms((size_t)n * 8);
        k.blk8_lambda.assign((size_t)c.rp + 1, h_one()); k.rc_partial_scaled.resize(c.rp);
        for (int q = 0; q < c.rp; ++q) {
            const fr_t l5k = h_mul(fr_pow5<PF>(k.blk8_lambda[q]), kappa);
            k.blk8_lambda[q + 1] = h_mul(l5k, a_inv); yinv[q] = fr_inv<PF>(l5k);
            k.rc_partial_scaled[q] = h_mul(k.blk8_lambda[q], c.rc_partial[q]);
        }
        k.rc_partial_scaled29.assign((size_t)(c.rp + 1) * 9, 0u);
        for (int q = 0; q < c.rp; ++q) { const fr29_t u = fr29_unpack(k.rc_partial_scaled[q]); for (int j = 0; j < 9; ++j) k.rc_partial_scaled29[(size_t)9 * q + j] = u.l[j]; }
        k.blk8_unscale29.resize(9); fr29_const_from<PF>(fr_inv<PF>(k.blk8_lambda[c.rp]), k.blk8_unscale29.data());
        for (int b = 0; b < nb; ++b) {
            for (int q = 0; q < 8; ++q) for (int j = 1; j < t; ++j) {
                um[(size_t)q * n + (j - 1)] = k.sparse[(size_t)(8 * b + q) * w + j];
                wm[(size_t)(j - 1) * 8 + q] = k.sparse[(size_t)(8 * b + q) * w + t - 1 + j];
            }
            const std::vector<int8_t> ef = mfma_frags(um.data(), 8, n, h_one()), lf = mfma_frags(wm.data(), n, 8, s20);
            k.blk8_efrag.insert(k.blk8_efrag.end(), ef.begin(), ef.end()); k.blk8_lfrag.insert(k.blk8_lfrag.end(), lf.begin(), lf.end());
            for (int q = 1; q < 8; ++q) for (int p2 = 0; p2 < q; ++p2) {
                fr_t acc = h_zero();
                for (int j = 0; j < n; ++j) acc = h_add(acc, h_mul(um[(size_t)q * n + j], wm[(size_t)j * 8 + p2]));
                g8[(size_t)b * 28 + q * (q - 1) / 2 + p2] = acc;
                k.blk8_gfrag.resize(k.blk8_gfrag.size() + 1024); mfma_frag_of(h_mul(acc, s20), &k.blk8_gfrag[k.blk8_gfrag.size() - 1024]);
                k.blk8s_gfrag.resize(k.blk8s_gfrag.size() + 1024); mfma_frag_of(h_mul(h_mul(acc, k.blk8_lambda[8 * b + q + 1]), yinv[8 * b + p2]), &k.blk8s_gfrag[k.blk8s_gfrag.size() - 1024]);
            }
            for (int q = 0; q < 8; ++q) for (int j = 0; j < n; ++j) {
                ums[(size_t)q * n + j] = h_mul(um[(size_t)q * n + j], k.blk8_lambda[8 * b + q + 1]);
                wms[(size_t)j * 8 + q] = h_mul(wm[(size_t)j * 8 + q], yinv[8 * b + q]);
            }
            const std::vector<int8_t> efs = mfma_frags(ums.data(), 8, n, h_one()), lfs = mfma_frags(wms.data(), n, 8, h_one());
            k.blk8s_efrag.insert(k.blk8s_efrag.end(), efs.begin(), efs.end()); k.blk8s_lfrag.insert(k.blk8s_lfrag.end(), lfs.begin(), lfs.end());
        }
        k.blk8_lfrag.resize(k.blk8_lfrag.size() + 1024); mfma_frag_of(h_one(), &k.blk8_lfrag[k.blk8_lfrag.size() - 1024]);
        k.gamma8_29 = to_radix29(g8, all);
    }
    if (t == 17 && c.rp == 64) {                                                                         // the five-wave latency kernel (poseidon_chain.hpp)
        const int rp = c.rp, w = 2 * t - 1;
        const fr_t scale = fr_from_u64<PF>(1ull << 25);
        auto limbs = [&](const fr_t& v, uint32_t* out) { const fr29_t u = fr29_unpack(h_mul(v, scale)); for (int i = 0; i < 9; ++i) out[i] = u.l[i]; };
        k.chain_a.assign((size_t)rp * 64, 0u); k.chain_g.assign((size_t)rp * 9 * 64, 0u); k.chain_w.assign((size_t)rp * (t - 1) * 9, 0u);
        for (int q = 0; q < rp; ++q) {
            uint32_t l[9]; limbs(k.sparse[(size_t)q * w], l);
            for (int i = 0; i < 9; ++i) k.chain_a[(size_t)q * 64 + 16 + i] = l[i];
            for (int j = 1; j < t; ++j) limbs(k.sparse[(size_t)q * w + t - 1 + j], &k.chain_w[((size_t)q * (t - 1) + (j - 1)) * 9]);
        }
        for (int q = 1; q < rp; ++q)
            for (int p2 = 0; p2 < q; ++p2) {
                const fr_t* uq = &k.sparse[(size_t)q * w]; const fr_t* wp = &k.sparse[(size_t)p2 * w];
                fr_t acc = h_zero();
                for (int j = 1; j < t; ++j) acc = h_add(acc, h_mul(uq[j], wp[t - 1 + j]));
                uint32_t l[9]; limbs(acc, l);
                if (q == p2 + 1) { for (int i = 0; i < 9; ++i) k.chain_a[(size_t)p2 * 64 + 32 + i] = l[i]; }             // Gamma_{p+1,p}: wave A's third row in round p
                else for (int i = 0; i < 9; ++i) k.chain_g[((size_t)p2 * 9 + i) * 64 + q] = l[i];                          // q >= p + 2: wave B, lane q
            }
    }
    k.ok = true;
    return k;
}

// hash_leaf_pair's 17-lane template (fri.rs:38-44): lanes 4 and 5 take (f, s), the other fifteen are constants.
inline void leaf_template(fr_t init[17]) {
    const fr_t AB = h_tag("FSv1-ABSORB-BYTES"), CH = h_tag("FSv1-CHALLENGE");
    for (int j = 0; j < 17; ++j) init[j] = h_zero();
    init[0] = AB; init[1] = h_words("FRI/leaf/poseidon")[0]; init[2] = AB; init[3] = h_words("FRI/leaf")[0];
    init[6] = CH; init[7] = AB; init[8] = h_words("leaf")[0]; init[16] = h_tag("FSv1-TRANSCRIPT-INIT");
}
// Round 0 of that permutation in closed form: after ARK and S-box the MDS output is K_i + M[i][4] x4 + M[i][5] x5 with
//     K_i = sum_{j != 4,5} M[i][j] (init_j + rc0_j)^5.
// krc29 (17 x 9 words): (K_i + rc_full[17 + i]) mod r, round 1's constant folded in, as the nine 29-bit limbs of the stored value (fr29_unpack, like rc_full29:
// an addend): what the leaf kernel's two-K-step round-0 rows add in front of round 1's S-box (poseidon_pair.hpp pair_leaf_round0_mfma).
inline void leaf_round0_consts(const PoseidonConsts& c, const fr_t* init, fr_t* K, uint32_t* krc29) {
    fr_t x[17]; for (int j = 0; j < 17; ++j) x[j] = fr_pow5<PF>(h_add(init[j], c.rc_full[j]));
    for (int i = 0; i < 17; ++i) {
        fr_t k = h_zero();
        for (int j = 0; j < 17; ++j) if (j != 4 && j != 5) k = h_add(k, h_mul(c.mds[(size_t)i * 17 + j], x[j]));
        K[i] = k;
        const fr29_t u = fr29_unpack(h_add(k, c.rc_full[17 + i]));
        for (int j = 0; j < 9; ++j) krc29[9 * i + j] = u.l[j];
    }
}
// every leaf constant of a parameter set (poseidon_params.hpp LeafConsts): what the context uploads and the host checks read
inline void leaf_consts(const PoseidonConsts& c, LeafConsts& lc) {
    memset(&lc, 0, sizeof lc);
    leaf_template(lc.init);      // lanes 4,5 = (f, s)
    leaf_round0_consts(c, lc.init, lc.K, lc.krc29);
    const fr_t k20 = fr_from_u64<PF>(1ull << FR29_SBOX_SHIFT);     // the S-box outputs x4, x5 arrive divided by 2^20 (fr_pow5_r29)
    for (int i = 0; i < 17; ++i) {
        lc.m4[i] = c.mds[(size_t)i * 17 + 4]; lc.m5[i] = c.mds[(size_t)i * 17 + 5];
        fr29_const_from<PF>(h_mul(lc.m4[i], k20), lc.m45_29 + 9 * i); fr29_const_from<PF>(h_mul(lc.m5[i], k20), lc.m45_29 + 9 * (17 + i));
    }
}

// Reference-form permutation on the host (dense MDS every round; poseidon/src/lib.rs:31-68,219-258).
// Used only by the host-check library to validate the kernel-form constants on CPU.
inline void permute_dense(fr_t* s, const PoseidonConsts& c) {
    const int t = c.t, half = c.rf / 2; std::vector<fr_t> o(t);
    auto mds = [&]() { for (int i = 0; i < t; ++i) { fr_t acc = h_zero(); for (int j = 0; j < t; ++j) acc = h_add(acc, h_mul(c.mds[(size_t)i * t + j], s[j])); o[i] = acc; } for (int i = 0; i < t; ++i) s[i] = o[i]; };
    for (int r = 0; r < half; ++r) { for (int i = 0; i < t; ++i) s[i] = fr_pow5<PF>(h_add(s[i], c.rc_full[(size_t)r * t + i])); mds(); }
    for (int r = 0; r < c.rp; ++r) { s[0] = fr_pow5<PF>(h_add(s[0], c.rc_partial[r])); mds(); }
    for (int r = half; r < c.rf; ++r) { for (int i = 0; i < t; ++i) s[i] = fr_pow5<PF>(h_add(s[i], c.rc_full[(size_t)r * t + i])); mds(); }
}

}  // namespace host
}  // namespace stark
