// tests/oracle_merkle_verify.cpp — TEST INFRASTRUCTURE ONLY: the oracle's verify_many_ds and verify_pairs_ds (oracle/merkle.hpp,
// merkle/src/lib.rs:587-701, :723-773) over the canonical MerkleProof bytes, so that tampered, truncated and empty proofs can be put to the oracle as they are put to the product.
// Built by tests/merkle_batch_cases.py into tests/_build/; the product never links or loads it.
#include <cstring>
#include "../oracle/merkle.hpp"

using namespace oracle;

namespace {
// the canonical encoding of DESIGN.md §7, bounds-checked: idxs | levels of 32-byte canonical elements | levels of group sizes | arity
struct Dec {
    const uint8_t* p; size_t n, o = 0; bool bad = false;
    uint64_t u64() { if (n - o < 8) { bad = true; return 0; } uint64_t x = 0; for (int j = 0; j < 8; ++j) x |= (uint64_t)p[o + j] << (8 * j); o += 8; return x; }
    size_t len(size_t item) { const uint64_t x = u64(); if (bad || x > (n - o) / item) { bad = true; return 0; } return (size_t)x; }
    Fr fr() {
        if (bad || n - o < 32) { bad = true; return Fr::zero(); }
        uint64_t c[4]; for (int i = 0; i < 4; ++i) { c[i] = 0; for (int j = 0; j < 8; ++j) c[i] |= (uint64_t)p[o + 8 * i + j] << (8 * j); }
        o += 32; if (Fr::geq_mod(c)) { bad = true; return Fr::zero(); } return Fr::from_canonical(c);
    }
    bool mproof(MerkleProof& m) {
        size_t k = len(8); for (size_t i = 0; i < k && !bad; ++i) m.indices.push_back((size_t)u64());
        size_t a = len(8); for (size_t i = 0; i < a && !bad; ++i) { size_t c = len(32); std::vector<Fr> l; for (size_t j = 0; j < c && !bad; ++j) l.push_back(fr()); m.siblings.push_back(l); }
        size_t b = len(8); for (size_t i = 0; i < b && !bad; ++i) { size_t c = len(1); std::vector<uint8_t> l; for (size_t j = 0; j < c && !bad; ++j) { l.push_back(p[o]); ++o; } m.group_sizes.push_back(l); }
        m.arity = (size_t)u64();
        return !bad && o == n;
    }
};
}  // namespace

// 1 accept, 0 reject (bytes that are no MerkleProof included), -1 where the reference would panic
extern "C" int om_verify_many_ds(size_t cfg_arity, uint64_t label, const uint64_t* root, const size_t* idx, size_t k, const uint64_t* values, const uint8_t* proof, size_t len) {
    Dec d{proof, len}; MerkleProof pr;
    if (!d.mproof(pr)) return 0;
    std::vector<size_t> ix(idx, idx + k); std::vector<Fr> v(k);
    for (size_t i = 0; i < k; ++i) v[i] = Fr::from_raw(values + 4 * i);
    try { return verify_many_ds(Fr::from_raw(root), ix, v, pr, label, poseidon_params_for_arity(cfg_arity)) ? 1 : 0; } catch (...) { return -1; }
}
// the same under MerkleCommitment's parameters (commitment/src/lib.rs:48-51: arity 16, "POSEIDON-T17-X5-SEED"): the openings inside a ProofMF
extern "C" int om_verify_many_ds_commitment(uint64_t label, const uint64_t* root, const size_t* idx, size_t k, const uint64_t* values, const uint8_t* proof, size_t len) {
    static const PoseidonParams params = generate_params_t17_x5(bytes_of("POSEIDON-T17-X5-SEED"));
    Dec d{proof, len}; MerkleProof pr;
    if (!d.mproof(pr)) return 0;
    std::vector<size_t> ix(idx, idx + k); std::vector<Fr> v(k);
    for (size_t i = 0; i < k; ++i) v[i] = Fr::from_raw(values + 4 * i);
    try { return verify_many_ds(Fr::from_raw(root), ix, v, pr, label, params) ? 1 : 0; } catch (...) { return -1; }
}
// the same for verify_pairs_ds over (f[i], cp[i])
extern "C" int om_verify_pairs_ds(size_t cfg_arity, uint64_t label, const uint64_t* root, const size_t* idx, size_t k, const uint64_t* f, const uint64_t* cp, const uint8_t* proof, size_t len) {
    Dec d{proof, len}; MerkleProof pr;
    if (!d.mproof(pr)) return 0;
    std::vector<size_t> ix(idx, idx + k); std::vector<std::pair<Fr, Fr>> ps(k);
    for (size_t i = 0; i < k; ++i) ps[i] = {Fr::from_raw(f + 4 * i), Fr::from_raw(cp + 4 * i)};
    try { return verify_pairs_ds(Fr::from_raw(root), ix, ps, pr, label, poseidon_params_for_arity(cfg_arity)) ? 1 : 0; } catch (...) { return -1; }
}
