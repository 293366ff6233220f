// stark_mlwe_amd/csrc/hostcheck.cpp — DIAGNOSTIC library (libstark_mlwe_hostcheck.so), CPU-only.
//
// Instantiates, on the host, the SAME inline code the kernels are built from (fr.hpp arithmetic,
// host_util.hpp constant derivation, poseidon_dev.hpp permutation / sponge bodies with a plain-array
// state) so that `pytest -m "not gpu"` can check the product's host logic and kernel bodies against
// the oracle without a GPU.  No product entry point loads or calls this library; it is not a
// fallback: libstark_mlwe_hip.so fails with STARK_ERR_HIP when no device is present.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>
#include "fr.hpp"
#include "host_util.hpp"
#include "poseidon_dev.hpp"
#include "fri_plan.hpp"
#include "fri_verify.hpp"
#include "fri_verify_batch.hpp"
#include "mfma_digits.hpp"
#include "poseidon_chain.hpp"
#include "fri_batch.hpp"
#include "fri_mixed.hpp"
#include "ntt_mixed_plan.hpp"
#include "sumcheck_impl.hpp"     // the provers' transcript labels, sumcheck_batch.hpp and sumcheck_verify_batch.hpp (host-only)
#include "mle_dev.hpp"
#include "merkle_batch.hpp"
#include "lagrange_dev.hpp"

using namespace stark;

static fr_t ld4(const uint64_t* p) { fr_t x; for (int i = 0; i < 4; ++i) { x.v[2 * i] = (uint32_t)p[i]; x.v[2 * i + 1] = (uint32_t)(p[i] >> 32); } return x; }
static void st4(uint64_t* p, const fr_t& x) { for (int i = 0; i < 4; ++i) p[i] = (uint64_t)x.v[2 * i] | ((uint64_t)x.v[2 * i + 1] << 32); }

// What the host executors hand out as "device" memory holds this byte (hc_set_alloc_fill; 0 unless a test sets it), as the device allocator's blocks
// do under the context option "pool_poison": a shared driver that reads a slot nothing filled reads this, not zero.
static int g_alloc_fill = 0;
static std::vector<uint64_t> hc_block(size_t bytes) { std::vector<uint64_t> v((bytes + 7) / 8 + 1); memset(v.data(), g_alloc_fill, v.size() * sizeof(uint64_t)); return v; }
static std::vector<fr_t> hc_fr_block(size_t n) { std::vector<fr_t> v(n); if (n) memset((void*)v.data(), g_alloc_fill, n * sizeof(fr_t)); return v; }
// The refusal countdown of the host executors (hc_set_alloc_refuse_at; process-wide like the fill), the twin of the device allocator's hook
// (stark_ctx::alloc_hook): allocation requests are counted from the arming, and request number g_refuse_at (0: none) fails with kHcOom, once.
static const int32_t kHcOom = -4;                                        // STARK_ERR_OOM
static uint64_t g_refuse_at = 0, g_alloc_requests = 0, g_alloc_refused = 0;
static bool hc_alloc_refused() { if (++g_alloc_requests != g_refuse_at) return false; g_refuse_at = 0; ++g_alloc_refused; return true; }
// what an export returns for a driver's status: the out-of-memory code as it is, -1 for everything else (as before)
static int hc_rc(int32_t rc) { return rc == kHcOom ? (int)kHcOom : -1; }
// THE memory of the host executors, the twin of DevArena (ctx.hpp): blocks of hc_block that live as long as it, upload and download = memcpy.
struct HostArena {
    std::vector<std::vector<uint64_t>> mem;
    int32_t alloc(size_t bytes, void** out) { if (hc_alloc_refused()) { *out = nullptr; return kHcOom; } mem.push_back(hc_block(bytes)); *out = mem.back().data(); return 0; }
    int32_t upload(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
    template <class T> int32_t put(const std::vector<T>& h, T** out) {
        void* p = nullptr; if (int32_t rc = alloc(std::max<size_t>(h.size(), 1) * sizeof(T), &p)) return rc;
        if (!h.empty()) if (int32_t rc = upload(p, h.data(), h.size() * sizeof(T))) return rc;
        *out = (T*)p; return 0;
    }
    int32_t download(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
};

struct HcParams { host::PoseidonConsts ref; host::KernelConsts kc; PoseidonDev dev; };
static void bind(HcParams* P) {
    P->kc = host::make_kernel_consts(P->ref);
    P->dev.t = P->kc.t; P->dev.rf = P->kc.rf; P->dev.rp = P->kc.rp; P->dev.rc_full = P->kc.rc_full.data(); P->dev.rc_partial = P->kc.rc_partial.data();
    P->dev.lu = P->kc.lu.data(); P->dev.lu_pre = P->kc.lu_pre.data(); P->dev.row0 = P->kc.row0.data(); P->dev.sparse = P->kc.sparse.data(); P->dev.mds = P->kc.mds.data(); P->dev.mds_pre = P->kc.mds_pre.data(); P->dev.gamma = P->kc.gamma.data();
    P->dev.lu29 = P->kc.lu29.data(); P->dev.lu_pre29 = P->kc.lu_pre29.data(); P->dev.row0_29 = P->kc.row0_29.data(); P->dev.sparse29 = P->kc.sparse29.data(); P->dev.gamma29 = P->kc.gamma29.data(); P->dev.mds29 = P->kc.mds29.data(); P->dev.mds_pre29 = P->kc.mds_pre29.data(); P->dev.rc_full29 = P->kc.rc_full29.data();
    P->dev.mds_frag = nullptr; P->dev.mds_pre_frag = nullptr; P->dev.blk8_efrag = nullptr; P->dev.blk8_lfrag = nullptr; P->dev.blk8_unit_frag = nullptr; P->dev.blk8_gfrag = nullptr; P->dev.rc_partial_scaled29 = nullptr;
    P->dev.chain_a = P->kc.chain_a.empty() ? nullptr : P->kc.chain_a.data(); P->dev.chain_g = P->kc.chain_g.empty() ? nullptr : P->kc.chain_g.data(); P->dev.chain_w = P->kc.chain_w.empty() ? nullptr : P->kc.chain_w.data();
}

// One launch of a DS stream on the host: hash_ds_body over every hash of D under P — the body every executor's hash_level and every hc_hash_ds_* export runs.
template <class DS, class Put> static void hash_ds_stream(const HcParams* P, const DS& D, Put put) {
    std::vector<fr_t> st(P->dev.t);
    for (size_t k = 0; k < D.n_out; ++k) { ArrayState s{st.data()}; put(k, hash_ds_body(s, P->dev, D, k)); }
}
// The recording side of the host executors: while a log is open (hc_climb_launches), every hash_level records its launch — which stream, its DS level
// number, its hashes, where they go — and writes zeros where the hashes would go (what is launched depends on the shapes alone).
struct HcLaunch { int kind; uint32_t level; size_t n_out; const fr_t* out; };
enum { kHcBatchPitch = 1, kHcBatchPtrs = 2, kHcBatchPairs = 3, kHcRaggedNodes = 4, kHcRaggedPairs = 5, kHcBatchPairPtrs = 6, kHcRaggedFriPairs = 7 };
static thread_local std::vector<HcLaunch>* g_launch_log = nullptr;
static int ds_kind(const DsBatchStream& D) { return D.in_ptrs ? kHcBatchPtrs : kHcBatchPitch; }
static int ds_kind(const DsBatchPairStream&) { return kHcBatchPairs; }
static int ds_kind(const DsBatchPairPtrStream&) { return kHcBatchPairPtrs; }
static int ds_kind(const DsRaggedStream& D) { return D.mode == 1 ? kHcRaggedPairs : kHcRaggedNodes; }
static int ds_kind(const DsRaggedPairStream&) { return kHcRaggedFriPairs; }
template <class DS> static int32_t hash_ds_stream(const HcParams* P, const DS& D, fr_t* out) {
    if (g_launch_log) { g_launch_log->push_back(HcLaunch{ds_kind(D), fr_to_canonical<PF>(D.level_f).v[0], D.n_out, out}); std::fill(out, out + D.n_out, fr_zero<PF>()); return 0; }
    hash_ds_stream(P, D, [&](size_t k, const fr_t& h) { out[k] = h; }); return 0;
}
static int32_t hash_ds_stream(const HcParams* P, const DsGatherStream& D, fr_t* out) { hash_ds_stream(P, D, [&](size_t k, const fr_t& h) { out[k] = h; }); return 0; }
template <class DS> static int hash_ds_stream(const HcParams* P, const DS& D, uint64_t* out4) { hash_ds_stream(P, D, [&](size_t k, const fr_t& h) { st4(out4 + 4 * k, h); }); return 0; }

extern "C" {

// The byte of every block the host executors allocate from here on (process-wide; 0 = the default).  Returns the previous one; -1: not a byte.
int hc_set_alloc_fill(int byte) { if (byte < 0 || byte > 255) return -1; const int old = g_alloc_fill; g_alloc_fill = byte; return old; }
// Arms the refusal countdown of the host executors: allocation request number n from here on (HostArena::alloc, put and the Merkle executor's level
// blocks) fails with STARK_ERR_OOM, once; n = 0 disarms.  The counters restart either way.  hc_alloc_refusal_stats: requests counted and refusals
// fired since the last call of this function.
int hc_set_alloc_refuse_at(uint64_t n) { g_refuse_at = n; g_alloc_requests = 0; g_alloc_refused = 0; return 0; }
int hc_alloc_refusal_stats(uint64_t* out2) { out2[0] = g_alloc_requests; out2[1] = g_alloc_refused; return 0; }
// A block of `bytes` through the executors' allocation path, copied out: what a driver would read from a slot nothing wrote.
int hc_alloc_probe(size_t bytes, uint8_t* out) { const std::vector<uint64_t> v = hc_block(bytes); memcpy(out, v.data(), bytes); return 0; }

// field: 0 Pallas, 1 BLS12-381.  op: 0 add, 1 sub, 2 mul, 3 inv, 4 from_u64(a[0]), 5 to_canonical, 6 root_of_unity(a[0]), 7 pow_u64(a, b[0]),
// 8 the kernels' S-box fr_pow5_r29 (fr29.hpp: x^5 / 2^20)
int hc_fr_op(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    fr_t x = ld4(a), y = b ? ld4(b) : x, z;
    if (field == 0) {
        switch (op) { case 0: z = fr_add<PallasFr>(x, y); break; case 1: z = fr_sub<PallasFr>(x, y); break; case 2: z = fr_mul<PallasFr>(x, y); break; case 3: z = fr_inv<PallasFr>(x); break;
            case 4: z = fr_from_u64<PallasFr>(a[0]); break; case 5: z = fr_to_canonical<PallasFr>(x); break; case 6: z = fr_root_of_unity<PallasFr>((unsigned)a[0]); break;
            case 7: z = fr_pow_u64<PallasFr>(x, b[0]); break; case 8: z = fr_pow5_r29<PallasFr>(x); break; default: return -1; }
    } else {
        switch (op) { case 0: z = fr_add<Bls12381Fr>(x, y); break; case 1: z = fr_sub<Bls12381Fr>(x, y); break; case 2: z = fr_mul<Bls12381Fr>(x, y); break; case 3: z = fr_inv<Bls12381Fr>(x); break;
            case 4: z = fr_from_u64<Bls12381Fr>(a[0]); break; case 5: z = fr_to_canonical<Bls12381Fr>(x); break; case 6: z = fr_root_of_unity<Bls12381Fr>((unsigned)a[0]); break;
            case 7: z = fr_pow_u64<Bls12381Fr>(x, b[0]); break; case 8: z = fr_pow5_r29<Bls12381Fr>(x); break; default: return -1; }
    }
    st4(out, z); return 0;
}
// sum_i a_i*b_i through the product's dot-product accumulator (DotAcc: radix-2^29 constants, carry pass every 6 terms,
// chunks of 60) and, for comparison, through the radix-2^32 wide accumulator the cooperative kernels use (mode 1)
int hc_wide_dot(const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    DotAcc d; d.init();
    for (size_t i = 0; i < n; ++i) { uint32_t c[9]; fr29_const_from<PF>(ld4(a + 4 * i), c); d.mac(c, ld4(b + 4 * i)); }
    st4(out, d.finish()); return 0;
}
int hc_wide_dot32(const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    if (n > 24) return -1;
    fr_wide w; fr_wide_zero(w);
    for (size_t i = 0; i < n; ++i) fr_wide_mac_f<PF>(w, ld4(a + 4 * i), ld4(b + 4 * i));
    st4(out, fr_wide_reduce<PF>(w)); return 0;
}
}  // extern "C"
// One size-2^log_b sub-NTT exactly as a tile of ntt_dev.hpp computes it (nine-limb lazy decimation-in-time butterflies, the same carry-pass
// schedule, tables carrying the factor 32, the multiply-by-32 epilogue), sequentially on the host.  data: 2^log_b canonical Montgomery values,
// natural order in and out.  Also reports the largest limb / top limb any operand of a product reached (bounds check for the tests).
template <class F> static int hc_ntt29_impl(uint64_t* data, int log_b, int inverse, uint64_t* max_limb, uint64_t* max_top) {
    if (log_b < 1 || log_b > 16) return -1;
    const size_t B = (size_t)1 << log_b;
    fr_t w = fr_root_of_unity<F>((unsigned)log_b); if (inverse) w = fr_inv<F>(w);
    const fr_t k32 = fr_from_u64<F>(32);
    std::vector<fr29_t> tw(B / 2), x(B);
    { fr_t acc = k32; for (size_t i = 0; i < B / 2; ++i) { tw[i] = fr29_unpack(acc); acc = fr_mul<F>(acc, w); } }
    uint32_t D[9]; ntt29_offset<F>(D);
    auto brev = [&](size_t v) { size_t r = 0; for (int i = 0; i < log_b; ++i) r |= ((v >> i) & 1) << (log_b - 1 - i); return r; };
    for (size_t p = 0; p < B; ++p) x[brev(p)] = fr29_unpack(ld4(data + 4 * p));
    uint64_t ml = 0, mt = 0;
    const int head = log_b >= 3 ? 3 : log_b;
    {   // the register head of the kernels: groups of 2^head consecutive (bit-reversed) rows
        const fr29_t w1 = tw[log_b >= 3 ? B >> 3 : 0], w2 = tw[log_b >= 2 ? B >> 2 : 0], w3 = tw[log_b >= 3 ? 3 * (B >> 3) : 0];
        for (size_t g = 0; g < (B >> head); ++g) {
            fr29_t* xs = &x[g << head];
            if (head == 3) ntt29_head<F, 3>(*reinterpret_cast<fr29_t (*)[8]>(xs), w1, w2, w3, D);
            else if (head == 2) ntt29_head<F, 2>(*reinterpret_cast<fr29_t (*)[4]>(xs), w1, w2, w3, D);
            else ntt29_head<F, 1>(*reinterpret_cast<fr29_t (*)[2]>(xs), w1, w2, w3, D);
        }
    }
    for (int s = head + 1; s <= log_b; ++s) {
        const size_t half = (size_t)1 << (s - 1); const bool nrm = ntt29_norm_before(s);
        for (size_t bq = 0; bq < B / 2; ++bq) {
            const size_t j = bq & (half - 1), grp = bq >> (s - 1), i0 = (grp << s) + j, i1 = i0 + half;
            fr29_t a = x[i0], b = x[i1];
            { fr29_t bb = b, aa = a; if (nrm) { fr29_norm(bb); fr29_norm(aa); } for (int k = 0; k < 8; ++k) { ml = std::max<uint64_t>(ml, bb.l[k]); ml = std::max<uint64_t>(ml, aa.l[k]); } mt = std::max<uint64_t>(mt, std::max(bb.l[8], aa.l[8])); }
            ntt29_butterfly<F>(a, b, tw[j << (log_b - s)], D, nrm);
            x[i0] = a; x[i1] = b;
        }
    }
    const bool nrm_out = ntt29_norm_after(log_b);
    fr_t mult = k32; if (inverse) mult = fr_mul<F>(k32, fr_inv<F>(fr_from_u64<F>((uint64_t)B)));
    for (size_t k = 0; k < B; ++k) {
        fr29_t y = x[k];
        for (int i = 0; i < 8; ++i) ml = std::max<uint64_t>(ml, nrm_out ? 0 : y.l[i]);
        if (inverse) {   // an output with a table factor: the product is the reduction
            if (nrm_out) fr29_norm(y);
            mt = std::max<uint64_t>(mt, y.l[8]);
            const fr29_t r = fr29_mul_mont<F>(fr29_unpack(mult), y);
            st4(data + 4 * k, fr29_pack_reduce<F>(r.l));
        } else {         // no factor: reduce without a product
            fr29_partial_reduce<F>(y);
            st4(data + 4 * k, fr29_pack_reduce<F>(y.l));
        }
    }
    if (max_limb) *max_limb = ml; if (max_top) *max_top = mt;
    return 0;
}
extern "C" {
// fr29_partial_reduce on n lazy nine-limb values (9 x u32 each, any limbs below 2^32 with the value below 2^261): in place
int hc_partial_reduce(int field, uint32_t* limbs, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        fr29_t x; for (int k = 0; k < 9; ++k) x.l[k] = limbs[9 * i + k];
        if (field == 0) fr29_partial_reduce<PallasFr>(x); else fr29_partial_reduce<Bls12381Fr>(x);
        for (int k = 0; k < 9; ++k) limbs[9 * i + k] = x.l[k];
    }
    return 0;
}
int hc_ntt29(int field, uint64_t* data, int log_b, int inverse, uint64_t* max_limb, uint64_t* max_top) {
    return field == 0 ? hc_ntt29_impl<PallasFr>(data, log_b, inverse, max_limb, max_top) : hc_ntt29_impl<Bls12381Fr>(data, log_b, inverse, max_limb, max_top);
}
int hc_blake3(const uint8_t* p, size_t n, uint8_t* out32) { host::Blake3::hash(p, n, out32); return 0; }
int hc_chacha12_u64s(const uint8_t* seed32, size_t n, uint64_t* out) { host::ChaCha12Rng r(seed32); for (size_t i = 0; i < n; ++i) out[i] = r.next_u64(); return 0; }
int hc_from_le_bytes_mod_order(const uint8_t* b, size_t n, uint64_t* out) { st4(out, host::h_from_le_bytes_mod_order(b, n)); return 0; }
int hc_to_bytes_le(const uint64_t* a, uint8_t* out32) { host::h_to_bytes_le(ld4(a), out32); return 0; }

// kind 0: consts_for_width(t); 1: transcript; 2: t17 from seed string
void* hc_params_new(int kind, int t, const char* seed) {
    HcParams* P = new HcParams();
    P->ref = kind == 0 ? host::consts_for_width(t) : kind == 1 ? host::consts_transcript() : host::derive_consts(seed, 17, 8, 64);
    bind(P); return P;
}
// a caller's own constants (t*t, rf*t and rp elements, four u64 limbs each as stored), as stark_poseidon_params_upload takes them; check hc_params_ok
void* hc_params_upload(int t, int rf, int rp, const uint64_t* mds, const uint64_t* rc_full, const uint64_t* rc_partial) {
    if (!mds || !rc_full || !rc_partial || t < 2 || rf <= 0 || (rf & 1) || rp <= 0) return nullptr;
    HcParams* P = new HcParams();
    P->ref.t = t; P->ref.rf = rf; P->ref.rp = rp;
    P->ref.mds.resize((size_t)t * t); P->ref.rc_full.resize((size_t)rf * t); P->ref.rc_partial.resize(rp);
    for (size_t i = 0; i < P->ref.mds.size(); ++i) P->ref.mds[i] = ld4(mds + 4 * i);
    for (size_t i = 0; i < P->ref.rc_full.size(); ++i) P->ref.rc_full[i] = ld4(rc_full + 4 * i);
    for (size_t i = 0; i < P->ref.rc_partial.size(); ++i) P->ref.rc_partial[i] = ld4(rc_partial + 4 * i);
    bind(P); return P;
}
int hc_params_ok(void* h) { return ((HcParams*)h)->kc.ok ? 1 : 0; }
void hc_params_free(void* h) { delete (HcParams*)h; }
int hc_params_export(void* h, uint64_t* mds, uint64_t* rc_full, uint64_t* rc_partial) {
    HcParams* P = (HcParams*)h;
    for (size_t i = 0; i < P->ref.mds.size(); ++i) st4(mds + 4 * i, P->ref.mds[i]);
    for (size_t i = 0; i < P->ref.rc_full.size(); ++i) st4(rc_full + 4 * i, P->ref.rc_full[i]);
    for (size_t i = 0; i < P->ref.rc_partial.size(); ++i) st4(rc_partial + 4 * i, P->ref.rc_partial[i]);
    return 0;
}
// One full round's linear layer  y = M * x  (x = S-box outputs) of t = 17 states, two ways on the host: through the in-place L*U rows the VALU
// kernels use (which = 0), and through an emulation of the matrix-core path (which = 1): signed recoding, the int8 RESIDUE FRAGMENT TABLES the
// kernels read (host_util.hpp mfma_frags: lane l of fragment (i, e) holds A[row l & 31][k = 16 (l >> 5) + j]), D[row][col] = sum_k A[row][k] B[k][col]
// for the one 32-row tile, then the kernels' own fold and finishing step (mfma_digits.hpp mfma_cols_of_sums, mfma_finish_cols).
// pre: the B_1 * M matrix.
int hc_full_round_linear(void* h, int which, int pre, uint64_t* states, size_t n) {
    HcParams* P = (HcParams*)h; const int t = P->dev.t;
    if (t != 17 || P->kc.mds_frag.empty()) return -1;
    std::vector<fr_t> st(t), out(t);
    const std::vector<int8_t>& F = pre ? P->kc.mds_pre_frag : P->kc.mds_frag;
    for (size_t s = 0; s < n; ++s) {
        for (int j = 0; j < t; ++j) st[j] = ld4(states + 4 * (s * t + j));
        if (which == 0) { ArrayState a{st.data()}; apply_lu(a, pre ? P->dev.lu_pre29 : P->dev.lu29, t); out = st; }
        else {
            std::vector<fr_t> xd(t); for (int e = 0; e < t; ++e) xd[e] = recode_signed(st[e]);
            for (int i = 0; i < t; ++i) {
                int32_t S[32];
                for (int r = 0; r < 32; ++r) { int64_t acc = 0;
                    for (int e = 0; e < t; ++e) for (int kh = 0; kh < 2; ++kh) { const int8_t* a = &F[((((size_t)i * t + e) * 64) + (r + 32 * kh)) * 16];
                        const int8_t* b = reinterpret_cast<const int8_t*>(xd[e].v) + 16 * kh; for (int j = 0; j < 16; ++j) acc += (int64_t)a[j] * b[j]; }
                    if (acc > 0x7fffffffll || acc < -0x80000000ll) return -2; S[r] = (int32_t)acc; }
                int64_t col[9]; mfma_cols_of_sums(S, col);
                out[i] = mfma_finish_cols(col);
            }
        }
        for (int j = 0; j < t; ++j) st4(states + 4 * (s * t + j), out[j]);
    }
    return 0;
}
// the int8 residue fragment table of a t = 17 parameter set (pre = 0: M, 1: B_1 * M), t*t*64*16 bytes in the layout of host_util.hpp mfma_frags;
// copies at most cap bytes out, returns the table's length
size_t hc_mfma_frag_table(void* h, int pre, int8_t* out, size_t cap) {
    HcParams* P = (HcParams*)h; const std::vector<int8_t>& F = pre ? P->kc.mds_pre_frag : P->kc.mds_frag;
    if (out) memcpy(out, F.data(), std::min(cap, F.size()));
    return F.size();
}
// the finishing step of the matrix-core product alone (mfma_digits.hpp: fold, signed carry pass, product-free reduction): n cases of 32 digit sums
// S_c (any |S_c| < 2^24, row c = digit position) -> the canonical representative of sum_c S_c 256^c mod r; -1 when a sum is outside the domain
int hc_mfma_finish(const int32_t* sums, size_t n, uint64_t* out) {
    for (size_t s = 0; s < n; ++s) {
        const int32_t* S = sums + 32 * s;
        for (int c = 0; c < 32; ++c) if (S[c] >= (1 << 24) || S[c] <= -(1 << 24)) return -1;
        int64_t col[9]; mfma_cols_of_sums(S, col);
        st4(out + 4 * s, mfma_finish_cols(col));
    }
    return 0;
}
// The finishing step stopped at its nine limbs (mfma_finish_limbs: what a fused row hands to the next S-box): n cases of 32 digit sums -> 9 x u32 each,
// W == sum_c S_c 256^c (mod r), 0 < W < 3r, limbs 0..7 below 2^29 and the top limb below 2^24; -1 when a sum is outside the domain
int hc_mfma_finish_limbs(const int32_t* sums, size_t n, uint32_t* out) {
    for (size_t s = 0; s < n; ++s) {
        const int32_t* S = sums + 32 * s;
        for (int c = 0; c < 32; ++c) if (S[c] >= (1 << 24) || S[c] <= -(1 << 24)) return -1;
        int64_t col[9]; mfma_cols_of_sums(S, col);
        mfma_finish_limbs(col, out + 9 * s);
    }
    return 0;
}
// The S-box on lazy limbs (mfma_digits.hpp sbox_lazy29, the kernels' 64-bit columns): n cases of limbs l (9 x u32, below 2^29, top below 2^24) and an
// addend c (9 x u32, below 2^29, top below 2^23) -> the canonical fr_pow5_r29 of (l + c) mod r.  colmax (optional, two u64 per case: low, high): the
// largest column value of the same steps in 128-bit arithmetic.  -1: a limb outside the domain; -2: the 64-bit and the 128-bit columns disagree.
int hc_sbox_lazy29(const uint32_t* l, const uint32_t* c, size_t n, uint64_t* out, uint64_t* colmax) {
    for (size_t s = 0; s < n; ++s) {
        const uint32_t* ls = l + 9 * s; const uint32_t* cs = c + 9 * s;
        for (int i = 0; i < 9; ++i) if (ls[i] >= (i < 8 ? 1u << 29 : 1u << 24) || cs[i] >= (i < 8 ? 1u << 29 : 1u << 23)) return -1;
        const fr_t z = sbox_lazy29(ls, cs);
        Lazy29Wide wide; const fr29_t x5 = wide.pow5(ls, cs);
        const fr_t zw = fr29_pack_reduce<PF>(x5.l);
        if (colmax) { colmax[2 * s] = (uint64_t)wide.max_col; colmax[2 * s + 1] = (uint64_t)(wide.max_col >> 64); }
        if ((wide.max_col >> 64) == 0 && memcmp(&z, &zw, sizeof(fr_t)) != 0) return -2;
        st4(out + 4 * s, z);
    }
    return 0;
}
// ---- the 8-round partial blocks of the t = 17 wave-pair kernels (poseidon_pair.hpp pair_block8) on the host: the kernels' schedule re-enacted with the tables the device gets, the rows' fold and finish their own ----
// One emulated 32-row tile: K K-steps, fragment k (1 KiB, host_util.hpp mfma_frag_of: lane l holds A[row l & 31][16 (l >> 5) + j]) against the recoded
// operand xd[k]; S[row] = sum_k sum_b A_k[row][b] xd_k[b].  -2 when a digit sum leaves the finishing step's domain |S| < 2^24.
static int blk8_tile_sums(const int8_t* const* frag, const fr_t* xd, int K, int32_t* S) {
    for (int r = 0; r < 32; ++r) { int64_t acc = 0;
        for (int k = 0; k < K; ++k) for (int kh = 0; kh < 2; ++kh) { const int8_t* a = frag[k] + (size_t)(r + 32 * kh) * 16;
            const int8_t* b = reinterpret_cast<const int8_t*>(xd[k].v) + 16 * kh; for (int j = 0; j < 16; ++j) acc += (int64_t)a[j] * b[j]; }
        if (acc >= (1 << 24) || acc <= -(1 << 24)) return -2; S[r] = (int32_t)acc; }
    return 0;
}
// a tile's 32 digit sums -> the row's value: the kernels' fold and finish (mfma_digits.hpp), canonical or stopped at the nine limbs
static fr_t blk8_finish_sums(const int32_t* S) { int64_t col[9]; mfma_cols_of_sums(S, col); return mfma_finish_cols(col); }
// to nine limbs as the kernels' mfma_post_limbs does: word columns folded per lane half, exchanged, a constant's words added (c29, or none), one pass
static void blk8_finish_sums_limbs(const int32_t* S, uint32_t* l, const uint32_t* c29 = nullptr) { int64_t col[8]; mfma_word_cols_mad_of_sums(S, col, c29); mfma_finish_words(col, l); }
static int blk8_tile(const int8_t* const* frag, const fr_t* xd, int K, fr_t& out) { int32_t S[32]; const int rc = blk8_tile_sums(frag, xd, K, S); if (rc) return rc; out = blk8_finish_sums(S); return 0; }
// the largest |digit sum| hc_permute_block8 has seen in a row of 16 + 7 K-steps (the longest tile of the block form) since the last reset
static std::atomic<int32_t> g_blk8_row23_max{0};
int32_t hc_blk8_row23_max(int reset) { return reset ? g_blk8_row23_max.exchange(0) : g_blk8_row23_max.load(); }
// A whole t = 17 permutation as pair_permute_fused runs it (poseidon_pair.hpp), stage by stage under the same names, with the tables as uploaded (blk8s_efrag /
// blk8s_gfrag / blk8s_lfrag, rc_partial_scaled29, blk8_unscale29, rc_full29).  The state of one sponge between the stages:
struct HcPair {
    const host::KernelConsts& k;
    fr_t st[17];        // canonical elements (in, and out behind RowEnd::Canonical)
    fr_t xd[17];        // the slots as operands: recoded S-box outputs; lanes 1..16 as digits of their signed residue inside the partial rounds
    uint32_t l0[9];     // kEntrySlot: row 0 of the entry product as its nine finish limbs
    fr29_t u;           // the chain in wave X
};
// pair_sbox_full<17>: st (canonical) -> xd
static void pair_sbox_full(HcPair& s, int r) { for (int j = 0; j < 17; ++j) s.xd[j] = recode_signed(fr_pow5_r29<PF>(fr_add<PF>(s.st[j], s.k.rc_full[(size_t)r * 17 + j]))); }
// pair_mds_sbox_mfma: one fold (the word columns) in front of the three ends.  Canonical: xd -> st; NextSbox: xd -> xd, the recoded S-box outputs of round
// `next`; BlockEntry: rows 1..16 -> xd, the digits of their signed residue (mfma_finish_bytes on the same word columns), row 0 -> l0
static int pair_mds_sbox_mfma(HcPair& s, const std::vector<int8_t>& F, RowEnd end, int next) {
    fr_t o[17] = {};      // BlockEntry forms no o[0]: slot 0 is dead during the blocks (xd[0] is zeroed here; the last block's NextSbox end rewrites it)
    for (int i = 0; i < 17; ++i) {
        const int8_t* fr[17]; for (int e = 0; e < 17; ++e) fr[e] = &F[((size_t)i * 17 + e) * 1024];
        int32_t S[32]; const int rc = blk8_tile_sums(fr, s.xd, 17, S); if (rc) return rc;
        int64_t col[8]; mfma_word_cols_mad_of_sums(S, col);
        if (end == RowEnd::NextSbox) { uint32_t l[9]; mfma_finish_words(col, l); o[i] = sbox_lazy29_recoded(l, &s.k.rc_full29[((size_t)next * 17 + i) * 9]); }
        else if (end == RowEnd::BlockEntry) { if (i == 0) mfma_finish_words(col, s.l0); else o[i] = mfma_finish_bytes(col); }
        else o[i] = mfma_finish_words_canonical(col);      // two conditional subtractions
    }
    for (int i = 0; i < 17; ++i) (end == RowEnd::Canonical ? s.st : s.xd)[i] = o[i];
    return 0;
}
// pair_block8, block b: rounds blk8_round_y / blk8_round_x, then blk8_lane_rows.  Row q = H_q = E_q + sum Gamma y_p as ONE tile of 16 + q K-steps (E fragments
// against the lanes, blk8_gfrag against the recoded yt_0..yt_{q-1}); the SCALED chain as a LAZY residue: no field element inside a block, no a_q y_q product.
static int pair_block8(HcPair& s, int b, LaneEnd end) {
    const host::KernelConsts& k = s.k; const int half = k.rf / 2;
    const int8_t* ef = k.blk8s_efrag.data() + (size_t)b * 8 * 16 * 1024; const int8_t* lf = k.blk8s_lfrag.data() + (size_t)b * 16 * 8 * 1024;
    const int8_t* gf = k.blk8s_gfrag.data() + (size_t)b * 28 * 1024; const int8_t* unit = k.blk8_lfrag.data() + k.blk8_lfrag.size() - 1024;
    fr_t yd[9], kx[23];
    for (int j = 0; j < 16; ++j) kx[j] = s.xd[1 + j];
    for (int q = 0; q < 8; ++q) {
        const int8_t* fr[23]; for (int j = 0; j < 16; ++j) fr[j] = ef + ((size_t)q * 16 + j) * 1024;
        for (int p2 = 0; p2 < q; ++p2) { fr[16 + p2] = gf + ((size_t)q * (q - 1) / 2 + p2) * 1024; kx[16 + p2] = yd[p2]; }
        int32_t S[32]; { const int rc = blk8_tile_sums(fr, kx, 16 + q, S); if (rc) return rc; }
        if (q == 7) { int32_t m = 0; for (int c = 0; c < 32; ++c) m = std::max(m, S[c] < 0 ? -S[c] : S[c]);
                      int32_t seen = g_blk8_row23_max.load(); while (m > seen && !g_blk8_row23_max.compare_exchange_weak(seen, m)) {} }
        // blk8_round_y: the row's finish with the next round's scaled constant in its columns (zero after the last round), posted as the slot's words
        uint32_t l[9]; blk8_finish_sums_limbs(S, l, &k.rc_partial_scaled29[(size_t)9 * (8 * b + q + 1)]);
        const fr_t slot = lazy29_to_slot(l);
        // blk8_round_x: the S-box on the lazy value, yt_q recoded unreduced, the slot's limbs added to x5's
        const fr29_t x5 = pow5_lazy29(s.u);
        yd[q] = recode_lazy29(x5);
        s.u = lazy29_add_slot(x5, slot);
        for (int i = 0; i < 9; ++i) if (s.u.l[i] >= (1u << 30)) return -4;             // pow5_lazy29's contract
    }
    // NextSbox: element 0 of the next full round's S-box from the chain's final value, lambda_rp X_rp (lazy) -> X_rp (below 1.04 r) once per permutation
    if (end == LaneEnd::NextSbox) { const fr29_t x0 = fr29_mul_c29(k.blk8_unscale29.data(), s.u); s.xd[0] = sbox_lazy29_recoded(x0.l, &k.rc_full29[((size_t)half * 17) * 9]); }
    // blk8_lane_rows, the unit fragment as the ninth K-step
    for (int j = 1; j < 17; ++j) {
        const int8_t* fr[9]; for (int p2 = 0; p2 < 8; ++p2) fr[p2] = lf + ((size_t)(j - 1) * 8 + p2) * 1024; fr[8] = unit;
        yd[8] = s.xd[j];
        int32_t S[32]; { const int rc = blk8_tile_sums(fr, yd, 9, S); if (rc) return rc; }
        if (end == LaneEnd::NextSbox) { uint32_t l[9]; blk8_finish_sums_limbs(S, l); s.xd[j] = sbox_lazy29_recoded(l, &k.rc_full29[((size_t)half * 17 + j) * 9]); }      // like a fused product row
        else if (end == LaneEnd::Bytes) { int64_t col[8]; mfma_word_cols_of_sums(S, col); s.xd[j] = mfma_finish_bytes(col); }      // the signed residue's digits, finished in the byte domain
        else { const fr_t z = blk8_finish_sums(S); s.xd[j] = end == LaneEnd::Canonical ? z : recode_signed(z); }
    }
    return 0;
}
static int pair_blocks8(HcPair& s, LaneEnd mid, LaneEnd last) {
    const int nb = s.k.rp / 8;
    for (int b = 0; b < nb; ++b) { const int rc = pair_block8(s, b, b == nb - 1 ? last : mid); if (rc) return rc; }
    return 0;
}
// pair_last_rounds<17, true>, the whole state kept (only0 = false)
static int pair_last_rounds(HcPair& s) {
    for (int r = s.k.rf / 2; r < s.k.rf; ++r) { const bool last = r == s.k.rf - 1; const int rc = pair_mds_sbox_mfma(s, s.k.mds_frag, last ? RowEnd::Canonical : RowEnd::NextSbox, r + 1); if (rc) return rc; }
    return 0;
}
// pair_permute_fused<false>(s, P, false, 0)
static int pair_permute_fused(HcPair& s) {
    const host::KernelConsts& k = s.k; const int half = k.rf / 2;
    pair_sbox_full(s, 0);
    for (int r = 0; r < half; ++r) { const bool pre = r == half - 1; const int rc = pair_mds_sbox_mfma(s, pre ? k.mds_pre_frag : k.mds_frag, pre ? RowEnd::BlockEntry : RowEnd::NextSbox, r + 1); if (rc) return rc; }
    // the chain as a lazy residue: row 0's finish limbs through the mailbox slot's layout, plus lambda_0 c_0 — no canonical value at the entry
    fr29_t zero9; for (int i = 0; i < 9; ++i) zero9.l[i] = 0;
    s.u = lazy29_add_c29(lazy29_add_slot(zero9, lazy29_to_slot(s.l0)).l, &k.rc_partial_scaled29[0]);
    for (int i = 0; i < 9; ++i) if (s.u.l[i] >= (1u << 30)) return -4;
    { const int rc = pair_blocks8(s, LaneEnd::Bytes, LaneEnd::NextSbox); if (rc) return rc; }
    return pair_last_rounds(s);
}
// n states through pair_permute_fused.  -1: the set has no block-8 tables; -2: a digit sum out of range; -4: a chain limb outside pow5_lazy29's contract.
int hc_permute_block8(void* h, uint64_t* states, size_t n) {
    HcParams* P = (HcParams*)h; const host::KernelConsts& k = P->kc;
    if (k.t != 17 || k.blk8s_efrag.empty() || k.blk8s_gfrag.empty() || k.blk8_unscale29.empty() || k.mds_frag.empty()) return -1;
    HcPair s{k};
    for (size_t i = 0; i < n; ++i) {
        for (int j = 0; j < 17; ++j) s.st[j] = ld4(states + 4 * (i * 17 + j));
        const int rc = pair_permute_fused(s); if (rc) return rc;
        for (int j = 0; j < 17; ++j) st4(states + 4 * (i * 17 + j), s.st[j]);
    }
    return 0;
}
// ---- the lazy chain of the 8-round blocks, piece by piece (mfma_digits.hpp) ----
// The finish with a constant in its columns: n cases of 32 digit sums and nine limbs c (below 2^29, top below 2^23) -> the nine limbs of
// W' == sum_c S_c 256^c + c (mod r) and the eight words of its mailbox slot.  -1: a sum or a limb outside the domain.
int hc_mfma_finish_limbs_c(const int32_t* sums, const uint32_t* c, size_t n, uint32_t* limbs, uint32_t* slots) {
    for (size_t s = 0; s < n; ++s) {
        const int32_t* S = sums + 32 * s; const uint32_t* cs = c + 9 * s;
        for (int i = 0; i < 32; ++i) if (S[i] >= (1 << 24) || S[i] <= -(1 << 24)) return -1;
        for (int i = 0; i < 9; ++i) if (cs[i] >= (i < 8 ? 1u << 29 : 1u << 23)) return -1;
        int64_t col[9]; mfma_cols_of_sums(S, col, cs);
        mfma_finish_limbs(col, limbs + 9 * s);
        const fr_t z = lazy29_to_slot(limbs + 9 * s);
        memcpy(slots + 8 * s, z.v, 32);
    }
    return 0;
}
// X's side: n cases of x5 (nine limbs) and a slot (eight words) -> u = lazy29_add_slot(x5, slot), nine limbs
void hc_lazy29_add_slot(const uint32_t* x5, const uint32_t* slots, size_t n, uint32_t* u) {
    for (size_t s = 0; s < n; ++s) { fr29_t a; fr_t z; memcpy(a.l, x5 + 9 * s, 36); memcpy(z.v, slots + 8 * s, 32); const fr29_t r = lazy29_add_slot(a, z); memcpy(u + 9 * s, r.l, 36); }
}
// recode_lazy29: n cases of nine limbs (value below 2^255 - 2^248, so that the top byte stays below 0x7f) -> 32 signed digits each
void hc_recode_lazy29(const uint32_t* x5, size_t n, int8_t* digits) {
    for (size_t s = 0; s < n; ++s) { fr29_t a; memcpy(a.l, x5 + 9 * s, 36); const fr_t d = recode_lazy29(a); memcpy(digits + 32 * s, d.v, 32); }
}
// The census of the chain's S-box: n cases of u (nine limbs below 2^30) -> x2, x4, x5 of pow5_lazy29 (27 limbs per case), the largest 128-bit column of the
// same steps (two u64 per case: low, high) and the top byte of the packed x5.  -1: a limb outside the contract; -2: the 64-bit and the 128-bit columns disagree.
int hc_chain_census(const uint32_t* u, size_t n, uint32_t* x245, uint64_t* colmax, uint8_t* topbyte) {
    static const uint32_t zero9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t s = 0; s < n; ++s) {
        fr29_t a; memcpy(a.l, u + 9 * s, 36);
        for (int i = 0; i < 9; ++i) if (a.l[i] >= (1u << 30)) return -1;
        Lazy29Wide wide; const fr29_t x5w = wide.pow5(a.l, zero9);
        const fr29_t x5 = pow5_lazy29(a);
        colmax[2 * s] = (uint64_t)wide.max_col; colmax[2 * s + 1] = (uint64_t)(wide.max_col >> 64);
        if ((wide.max_col >> 64) == 0 && memcmp(x5.l, x5w.l, 36) != 0) return -2;
        memcpy(x245 + 27 * s, wide.x2.l, 36); memcpy(x245 + 27 * s + 9, wide.x4.l, 36); memcpy(x245 + 27 * s + 18, x5w.l, 36);
        topbyte[s] = (uint8_t)(fr29_pack(x5w.l).v[7] >> 24);
    }
    return 0;
}
// The floor-quotient finish of the lanes between two blocks: n cases of 32 digit sums -> the nine limbs of W = V - floor(V / 2^254) r (the top limb a signed
// word) and the 32 signed digits recode_signed returns on its sign-extended pack.  -1: a sum outside the domain.
int hc_mfma_finish_recoded(const int32_t* sums, size_t n, uint32_t* limbs, int8_t* digits) {
    for (size_t s = 0; s < n; ++s) {
        const int32_t* S = sums + 32 * s;
        for (int i = 0; i < 32; ++i) if (S[i] >= (1 << 24) || S[i] <= -(1 << 24)) return -1;
        int64_t col[9]; mfma_cols_of_sums(S, col); mfma_finish_limbs_floor(col, limbs + 9 * s);
        mfma_cols_of_sums(S, col); const fr_t d = mfma_finish_recoded(col); memcpy(digits + 32 * s, d.v, 32);
    }
    return 0;
}
// The byte-domain finish of the same lanes: n cases of 32 digit sums -> the eight word columns as the lane pair folds them (wide != 0: pairs formed in 64 bits,
// rows of up to 17 K-steps; else the int32 pairs of the 9-K-step lane rows), the quotient estimate, the carry out of word 7 and the 32 signed digits.
// -1: a sum outside the form's domain (|S_c| <= 9 * 32 * 128 * 128, wide: 17 * 32 * 128 * 128).
int hc_mfma_finish_bytes(const int32_t* sums, size_t n, int wide, int64_t* cols, int32_t* qh, int64_t* carry, int8_t* digits) {
    const int32_t lim = (wide ? 17 : 9) * 32 * 128 * 128;
    for (size_t s = 0; s < n; ++s) {
        const int32_t* S = sums + 32 * s;
        for (int i = 0; i < 32; ++i) if (S[i] > lim || S[i] < -lim) return -1;
        int64_t* col = cols + 8 * s;
        if (wide) mfma_word_cols_of_sums<true>(S, col); else mfma_word_cols_of_sums<false>(S, col);
        const fr_t d = mfma_finish_bytes(col, qh + s, carry + s); memcpy(digits + 32 * s, d.v, 32);
    }
    return 0;
}
// The byte-domain finish on word columns folded by the MULTIPLY-ADD chain (mfma_word_cols_mad, then mfma_finish_bytes): what the FUSE kernels' product in front
// of the partial rounds runs for rows 1..16 (pair_mds_sbox_mfma, entry), rows of 17 K-steps.  Outputs as hc_mfma_finish_bytes.  -1: a sum outside
// |S_c| <= 17 * 32 * 128 * 128.
int hc_mfma_finish_bytes_mad(const int32_t* sums, size_t n, int64_t* cols, int32_t* qh, int64_t* carry, int8_t* digits) {
    const int32_t lim = 17 * 32 * 128 * 128;
    for (size_t s = 0; s < n; ++s) {
        const int32_t* S = sums + 32 * s;
        for (int i = 0; i < 32; ++i) if (S[i] > lim || S[i] < -lim) return -1;
        int64_t* col = cols + 8 * s;
        mfma_word_cols_mad_of_sums(S, col);
        const fr_t d = mfma_finish_bytes(col, qh + s, carry + s); memcpy(digits + 32 * s, d.v, 32);
    }
    return 0;
}
// The word-column finish to nine limbs (mfma_word_cols_mad / mfma_finish_words: the fused full-round rows, the H_q rows, the last block's lane rows): n cases
// of 32 digit sums and, with c != nullptr, nine limbs of a stored constant each -> the eight word columns as the lane pair folds them (the constant's words in),
// the quotient estimate, the carry out of word 7, the nine limbs of W == V + c (mod r) and (canon != nullptr) the canonical value by the two conditional
// subtractions of mfma_finish_words_canonical, as the products that end canonical take it.  -1: a sum outside |S_c| <= 23 * 32 * 128 * 128 or a limb of c
// outside a stored value's.
int hc_mfma_finish_words(const int32_t* sums, const uint32_t* c, size_t n, int64_t* cols, int32_t* qh, int64_t* carry, uint32_t* limbs, uint64_t* canon) {
    const int32_t lim = 23 * 32 * 128 * 128;
    for (size_t s = 0; s < n; ++s) {
        const int32_t* S = sums + 32 * s; const uint32_t* cs = c ? c + 9 * s : nullptr;
        for (int i = 0; i < 32; ++i) if (S[i] > lim || S[i] < -lim) return -1;
        if (cs) for (int i = 0; i < 9; ++i) if (cs[i] >= (i < 8 ? 1u << 29 : 1u << 23)) return -1;
        int64_t* col = cols + 8 * s;
        mfma_word_cols_mad_of_sums(S, col, cs);
        mfma_finish_words(col, limbs + 9 * s, qh + s, carry + s);
        if (canon) st4(canon + 4 * s, mfma_finish_words_canonical(col));
    }
    return 0;
}
// the scaled constants as the finishes take them (KernelConsts::rc_partial_scaled29: rp + 1 entries of nine limbs, the last zero); returns the length in words
size_t hc_rc_partial_scaled29_table(void* h, uint32_t* out, size_t cap) {
    const std::vector<uint32_t>& v = ((HcParams*)h)->kc.rc_partial_scaled29;
    if (out && !v.empty()) memcpy(out, v.data(), std::min(cap, v.size()) * 4);
    return v.size();
}
// the block-8 tables of a set: which = 0 blk8_efrag, 1 blk8_lfrag (its last 1 KiB: the unit fragment), 2 gamma8_29 (bytes of the uint32 words), 3 blk8_gfrag;
// the scaled family: 4 blk8s_efrag, 5 blk8s_lfrag (no unit fragment), 6 blk8s_gfrag, 7 rc_partial_scaled (rp stored field elements), 8 blk8_lambda (rp + 1 stored
// field elements) followed by the nine uint32 limbs of blk8_unscale29;
// copies at most cap bytes out, returns the table's length in bytes (0: the set has none)
size_t hc_blk8_table(void* h, int which, void* out, size_t cap) {
    HcParams* P = (HcParams*)h; const host::KernelConsts& k = P->kc;
    if (which >= 4) {
        std::vector<uint8_t> lam;
        if (which == 8 && !k.blk8_lambda.empty()) { lam.resize(k.blk8_lambda.size() * sizeof(fr_t) + k.blk8_unscale29.size() * 4);
            memcpy(lam.data(), k.blk8_lambda.data(), k.blk8_lambda.size() * sizeof(fr_t)); memcpy(lam.data() + k.blk8_lambda.size() * sizeof(fr_t), k.blk8_unscale29.data(), k.blk8_unscale29.size() * 4); }
        const void* src = which == 4 ? (const void*)k.blk8s_efrag.data() : which == 5 ? (const void*)k.blk8s_lfrag.data() : which == 6 ? (const void*)k.blk8s_gfrag.data() : which == 7 ? (const void*)k.rc_partial_scaled.data() : (const void*)lam.data();
        const size_t len = which == 4 ? k.blk8s_efrag.size() : which == 5 ? k.blk8s_lfrag.size() : which == 6 ? k.blk8s_gfrag.size() : which == 7 ? k.rc_partial_scaled.size() * sizeof(fr_t) : which == 8 ? lam.size() : 0;
        if (out && len) memcpy(out, src, std::min(cap, len));
        return len;
    }
    const void* src = which == 0 ? (const void*)k.blk8_efrag.data() : which == 1 ? (const void*)k.blk8_lfrag.data() : which == 3 ? (const void*)k.blk8_gfrag.data() : (const void*)k.gamma8_29.data();
    const size_t len = which == 0 ? k.blk8_efrag.size() : which == 1 ? k.blk8_lfrag.size() : which == 3 ? k.blk8_gfrag.size() : k.gamma8_29.size() * 4;
    if (out && len) memcpy(out, src, std::min(cap, len));
    return len;
}
// the full rounds' constants as the fused rows add them (KernelConsts::rc_full29: rf * t entries of nine 29-bit limbs of the STORED constant); copies at
// most cap words out, returns the table's length in words
size_t hc_rc_full29_table(void* h, uint32_t* out, size_t cap) {
    const std::vector<uint32_t>& v = ((HcParams*)h)->kc.rc_full29;
    if (out && !v.empty()) memcpy(out, v.data(), std::min(cap, v.size()) * 4);
    return v.size();
}
// The lane product's finish with the base lane in the tile: n cases of 32 digit sums S_c (the eight y K-steps) and a canonical base; the unit
// fragment's K-step against the recoded base is added to the sums (as the ninth K-step of pair_block8 does), then fold and finish:
// -> canonical (sum_c S_c 256^c + base) mod r.  -1: a total digit sum outside |S| < 2^24.
int hc_blk8_finish_with_base(void* h, const int32_t* sums, const uint64_t* bases, size_t n, uint64_t* out) {
    HcParams* P = (HcParams*)h; if (P->kc.blk8_lfrag.empty()) return -3;
    const int8_t* unit = P->kc.blk8_lfrag.data() + P->kc.blk8_lfrag.size() - 1024;
    for (size_t s = 0; s < n; ++s) {
        const fr_t bd = recode_signed(ld4(bases + 4 * s)); int32_t U[32], S[32];
        if (blk8_tile_sums(&unit, &bd, 1, U)) return -1;
        for (int c = 0; c < 32; ++c) { const int64_t v = (int64_t)sums[32 * s + c] + U[c]; if (v >= (1 << 24) || v <= -(1 << 24)) return -1; S[c] = (int32_t)v; }
        st4(out + 4 * s, blk8_finish_sums(S));
    }
    return 0;
}
// kernel-form permutation (LU + sparse) of nstates AoS states on the host
int hc_permute_kernel_form(void* h, uint64_t* states, size_t n) {
    HcParams* P = (HcParams*)h; int t = P->dev.t; std::vector<fr_t> st(t);
    for (size_t i = 0; i < n; ++i) { for (int j = 0; j < t; ++j) st[j] = ld4(states + 4 * (i * t + j)); ArrayState s{st.data()}; permute_core(s, P->dev, false); for (int j = 0; j < t; ++j) st4(states + 4 * (i * t + j), st[j]); }
    return 0;
}
// the permutation with its partial rounds UNROLLED over all rp rounds from the chain tables (poseidon_chain.hpp chain_partial_model: the algebra and
// table scaling of the three-wave latency kernel); full rounds dense.  t = 17 only.
int hc_permute_chain_model(void* h, uint64_t* states, size_t n) {
    HcParams* P = (HcParams*)h; const int t = P->ref.t, half = P->ref.rf / 2; if (!P->dev.chain_a) return -1;
    std::vector<fr_t> st(t), o(t);
    auto dense = [&](const std::vector<fr_t>& M) { for (int i = 0; i < t; ++i) { fr_t acc = host::h_zero(); for (int j = 0; j < t; ++j) acc = host::h_add(acc, host::h_mul(M[(size_t)i * t + j], st[j])); o[i] = acc; } st = o; };
    for (size_t i = 0; i < n; ++i) {
        for (int j = 0; j < t; ++j) st[j] = ld4(states + 4 * (i * t + j));
        for (int r = 0; r < half; ++r) { for (int j = 0; j < t; ++j) st[j] = fr_pow5<PallasFr>(host::h_add(st[j], P->ref.rc_full[(size_t)r * t + j])); dense(r == half - 1 ? P->kc.mds_pre : P->kc.mds); }
        chain_partial_model(st.data(), P->dev);
        for (int r = half; r < P->ref.rf; ++r) { for (int j = 0; j < t; ++j) st[j] = fr_pow5<PallasFr>(host::h_add(st[j], P->ref.rc_full[(size_t)r * t + j])); dense(P->kc.mds); }
        for (int j = 0; j < t; ++j) st4(states + 4 * (i * t + j), st[j]);
    }
    return 0;
}
// the constants of the row-form Montgomery step (poseidon_chain.hpp row_consts_host): nine limbs of -r^-1 mod 2^261, five limbs of t = r - 2^254
int hc_row_consts(uint32_t* out14) { const RowConstsHost K = row_consts_host(); for (int i = 0; i < 9; ++i) out14[i] = K.ni[i]; for (int i = 0; i < 5; ++i) out14[9 + i] = K.t[i]; return 0; }
// the chain tables' shapes: chain_a [rp][64], chain_g [rp][9][64], chain_w [rp][t-1][9]; copies one table out (which = 0, 1, 2); returns its length in words
size_t hc_chain_table(void* h, int which, uint32_t* out, size_t cap) {
    HcParams* P = (HcParams*)h; const std::vector<uint32_t>& v = which == 0 ? P->kc.chain_a : which == 1 ? P->kc.chain_g : P->kc.chain_w;
    if (out) for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
    return v.size();
}
// reference-form (dense) permutation on the host, from the same constants
int hc_permute_dense(void* h, uint64_t* states, size_t n) {
    HcParams* P = (HcParams*)h; int t = P->ref.t; std::vector<fr_t> st(t);
    for (size_t i = 0; i < n; ++i) { for (int j = 0; j < t; ++j) st[j] = ld4(states + 4 * (i * t + j)); host::permute_dense(st.data(), P->ref); for (int j = 0; j < t; ++j) st4(states + 4 * (i * t + j), st[j]); }
    return 0;
}
// kernel bodies on the host ---------------------------------------------------------------------------
}  // extern "C"
// the 17-lane template of hash_leaf_pair (LeafConsts::init) where a check needs nothing else of the leaf constants
static void leaf_init(fr_t init[17]) { host::leaf_template(init); }
extern "C" {
// Round 0 of the leaf permutation as k_leaf_pair2<true> runs it (poseidon_pair.hpp pair_leaf_round0_mfma), re-enacted: x4 = fr_pow5_r29(f + rc[4]) and
// x5 = fr_pow5_r29(f_next + rc[5]) (f_next == nullptr: the zero input) recoded, one emulated tile of TWO K-steps per element — fragments (i, 4), (i, 5) of
// mds_frag —, the kernels' fold and finish to nine limbs (word columns, mfma_finish_words), then round 1's S-box on the limbs plus the table entry.  n leaves, one
// f and one f_next each.  Out (each optional): the template (17 stored elements), the table (K_i + rc_full[17 + i]) mod r as 17 x 9 limbs (host_util.hpp
// leaf_round0_consts, what ctx_leaf_init uploads), x4 and x5 as stored (n x 2 elements), the rows' finish limbs (n x 17 x 9) and the canonical S-box outputs of
// round 1 (n x 17 elements).  -1: not a t = 17 set with fragment tables; -2: a digit sum beyond two K-steps' bound.
int hc_leaf_round0(void* tparams, const uint64_t* f, const uint64_t* f_next, size_t n, uint64_t* init_out, uint32_t* table_out, uint64_t* x45_out, uint32_t* limbs_out, uint64_t* sbox_out) {
    HcParams* P = (HcParams*)tparams; const host::KernelConsts& k = P->kc;
    if (k.t != 17 || k.mds_frag.empty() || k.rf < 2) return -1;
    LeafConsts lc; host::leaf_consts(P->ref, lc);      // what ctx_leaf_init uploads
    if (init_out) for (int j = 0; j < 17; ++j) st4(init_out + 4 * j, lc.init[j]);
    if (table_out) memcpy(table_out, lc.krc29, sizeof(lc.krc29));
    for (size_t s = 0; s < n; ++s) {
        fr_t x[2], xd[2];
        x[0] = fr_pow5_r29<PF>(fr_add<PF>(ld4(f + 4 * s), k.rc_full[4]));
        x[1] = fr_pow5_r29<PF>(fr_add<PF>(f_next ? ld4(f_next + 4 * s) : host::h_zero(), k.rc_full[5]));
        for (int e = 0; e < 2; ++e) { xd[e] = recode_signed(x[e]); if (x45_out) st4(x45_out + 4 * (2 * s + e), x[e]); }
        for (int i = 0; i < 17; ++i) {
            const int8_t* fr[2] = {&k.mds_frag[((size_t)i * 17 + 4) * 1024], &k.mds_frag[((size_t)i * 17 + 5) * 1024]};
            int32_t S[32]; if (blk8_tile_sums(fr, xd, 2, S)) return -2;
            for (int c = 0; c < 32; ++c) if (S[c] > 2 * 32 * 128 * 128 || S[c] < -2 * 32 * 128 * 128) return -2;
            uint32_t l[9]; blk8_finish_sums_limbs(S, l);
            if (limbs_out) memcpy(limbs_out + 9 * (17 * s + i), l, sizeof(l));
            if (sbox_out) st4(sbox_out + 4 * (17 * s + i), sbox_lazy29(l, &lc.krc29[9 * i]));
        }
    }
    return 0;
}
// the squeeze round's field row (KernelConsts::row0 = M[0][*], stored elements); copies at most cap elements out, returns the row's length
size_t hc_row0_table(void* h, uint64_t* out, size_t cap) {
    const std::vector<fr_t>& v = ((HcParams*)h)->kc.row0;
    if (out) for (size_t i = 0; i < v.size() && i < cap; ++i) st4(out + 4 * i, v[i]);
    return v.size();
}
// The squeeze row as the t = 17 wave-pair kernels run it (poseidon_pair.hpp pair_squeeze_row_mfma), re-enacted: n states of 17 canonical S-box outputs, recoded,
// one emulated tile of 17 K-steps against fragments (0, e) of mds_frag, the word-column fold and the canonical finish -> element 0 of M x.
// -1: not a t = 17 set with fragment tables; -2: a digit sum out of range.
int hc_squeeze_row(void* h, const uint64_t* states, size_t n, uint64_t* out) {
    HcParams* P = (HcParams*)h; const host::KernelConsts& k = P->kc;
    if (k.t != 17 || k.mds_frag.empty()) return -1;
    const int8_t* fr[17]; for (int e = 0; e < 17; ++e) fr[e] = &k.mds_frag[(size_t)e * 1024];
    for (size_t s = 0; s < n; ++s) {
        fr_t xd[17]; for (int e = 0; e < 17; ++e) xd[e] = recode_signed(ld4(states + 4 * (17 * s + e)));
        int32_t S[32]; if (blk8_tile_sums(fr, xd, 17, S)) return -2;
        int64_t col[8]; mfma_word_cols_mad_of_sums(S, col);
        st4(out + 4 * s, mfma_finish_words_canonical(col));
    }
    return 0;
}
int hc_leaf_pair(void* tparams, const uint64_t* f, const uint64_t* f_next, size_t n, size_t m, uint64_t* hout) {
    HcParams* P = (HcParams*)tparams;
    LeafConsts lc; host::leaf_consts(P->ref, lc);
    std::vector<fr_t> fv(n), nv(f_next ? (n + m - 1) / m : 0);
    for (size_t i = 0; i < fv.size(); ++i) fv[i] = ld4(f + 4 * i);
    for (size_t i = 0; i < nv.size(); ++i) nv[i] = ld4(f_next + 4 * i);
    const LeafStream L{lc.init, fv.data(), f_next ? nv.data() : nullptr, m, n};
    fr_t st[17];
    for (size_t i = 0; i < n; ++i) { ArrayState s{st}; st4(hout + 4 * i, leaf_pair_body(s, P->dev, L, i)); }
    return 0;
}
int hc_hash_ds_level(void* params, int mode, size_t arity, uint32_t level, uint64_t pos0, uint64_t label, const uint64_t* in0, const uint64_t* in1, size_t n_in, uint64_t* out) {
    HcParams* P = (HcParams*)params;
    std::vector<fr_t> a(n_in), b(in1 ? n_in : 0);
    for (size_t i = 0; i < n_in; ++i) { a[i] = ld4(in0 + 4 * i); if (in1) b[i] = ld4(in1 + 4 * i); }
    return hash_ds_stream(P, DsStream::make(mode, arity, level, pos0, label, a.data(), in1 ? b.data() : nullptr, n_in), out);
}
int hc_tr_hash(void* tparams, const char* tag, const uint64_t* fields, size_t k, size_t n, uint64_t* out) {
    HcParams* P = (HcParams*)tparams;
    std::vector<fr_t> fr; const int np = host::tr_hash_frame(tag, fr);
    std::vector<fr_t> fl(n * k); for (size_t i = 0; i < n * k; ++i) fl[i] = ld4(fields + 4 * i);
    const TrStream T = TrStream::equal(fr.data(), np, (int)fr.size() - np, fl.data(), k, n, host::h_tag("FSv1-TRANSCRIPT-INIT"));
    fr_t st[17];
    for (size_t i = 0; i < n; ++i) { ArrayState s{st}; st4(out + 4 * i, tr_hash_body(s, P->dev, T, i)); }
    return 0;
}
// the frame of a tag (host::tr_hash_frame): np elements in front of the fields, ns behind them
int hc_tr_frame_dims(const char* tag, int* np, int* ns) { std::vector<fr_t> fr; *np = host::tr_hash_frame(tag, fr); *ns = (int)fr.size() - *np; return 0; }
// stark_tr_hash_many_dev on the host: tr_hash_body over the Ragged stream that tr_ragged_items builds for the device driver, in its launch order,
// each digest to its item's out slot.  fields: n host pointers (null allowed iff k[i] == 0).  launch_order (optional, n): the caller's index of launch slot j.
int hc_tr_hash_many(void* tparams, size_t n, const char* const* tags, const uint64_t* const* fields, const size_t* k, uint64_t* out, size_t* launch_order) {
    HcParams* P = (HcParams*)tparams;
    std::vector<std::vector<fr_t>> frames(n), fl(n); std::vector<TrFrameRef> fr(n); std::vector<const fr_t*> fp(n, nullptr);
    for (size_t i = 0; i < n; ++i) {
        const int np = host::tr_hash_frame(tags[i], frames[i]); fr[i] = TrFrameRef{frames[i].data(), np, (int)frames[i].size() - np};
        if (!k[i]) continue;
        if (!fields || !fields[i]) return -1;
        fl[i].resize(k[i]); for (size_t q = 0; q < k[i]; ++q) fl[i][q] = ld4(fields[i] + 4 * q);
        fp[i] = fl[i].data();
    }
    const std::vector<TrStream::Item> items = tr_ragged_items(fr.data(), fp.data(), k, n);
    const TrStream T = tr_ragged_stream(items.data(), n, host::h_tag("FSv1-TRANSCRIPT-INIT"));
    fr_t st[17];
    for (size_t j = 0; j < n; ++j) {
        ArrayState s{st}; size_t slot = n; const fr_t d = tr_hash_body<true>(s, P->dev, T, j, &slot);
        if (slot >= n) return -2;
        st4(out + 4 * slot, d); if (launch_order) launch_order[j] = slot;
    }
    return 0;
}
// mixed_prove_groups (fri_plan.hpp): group_of[i] = the group of trace i, order = the traces group by group; returns the number of groups
size_t hc_mixed_prove_groups(size_t B, const size_t* n0, const size_t* schedule, const size_t* sched_off, const size_t* r, size_t* group_of, size_t* order) {
    const std::vector<std::vector<size_t>> G = mixed_prove_groups(B, n0, schedule, sched_off, r);
    size_t pos = 0;
    for (size_t g = 0; g < G.size(); ++g) for (size_t i : G[g]) { group_of[i] = g; order[pos++] = i; }
    return G.size();
}
int hc_hash_stream(void* params, int mode, const uint64_t* a, size_t na, const uint64_t* b, size_t nb, const uint64_t* tag, size_t n, uint64_t* out) {
    HcParams* P = (HcParams*)params;
    std::vector<fr_t> av(n * na), bv(n * nb), st(P->dev.t);
    for (size_t i = 0; i < n * na; ++i) av[i] = ld4(a + 4 * i); for (size_t i = 0; i < n * nb; ++i) bv[i] = ld4(b + 4 * i);
    for (size_t k = 0; k < n; ++k) { ArrayState s{st.data()}; st4(out + 4 * k, hash_stream_body(s, P->dev, mode, av.data(), na, bv.data(), nb, tag ? ld4(tag) : host::h_zero(), k)); }
    return 0;
}

// ---- query plan / assemble (fri_plan.hpp) with the transcript hashes computed on the host -------------------
struct HcHasher : TrHasher {
    void* tp; explicit HcHasher(void* p) : tp(p) {}
    int32_t hash(const char* tag, const fr_t* fields, size_t k, size_t n, fr_t* out) override {
        std::vector<uint64_t> in(4 * k * n), o(4 * n);
        for (size_t i = 0; i < k * n; ++i) st4(in.data() + 4 * i, fields[i]);
        int rc = hc_tr_hash(tp, tag, in.data(), k, n, o.data()); if (rc) return rc;
        for (size_t i = 0; i < n; ++i) out[i] = ld4(o.data() + 4 * i);
        return 0;
    }
};
struct HcPlan { FriPlan plan; void* tp; };
void* hc_fri_plan_create(void* tparams, const uint64_t* roots, size_t n0, const size_t* schedule, size_t L, size_t r) {
    std::vector<fr_t> rt(L + 1); for (size_t l = 0; l <= L; ++l) rt[l] = ld4(roots + 4 * l);
    HcPlan* P = new HcPlan(); P->tp = tparams; P->plan.r = r; std::string err;
    if (!P->plan.shape.make(n0, schedule, L, rt.data(), err)) { delete P; return nullptr; }
    HcHasher H(tparams); if (fri_plan_make(P->plan, H)) { delete P; return nullptr; }
    return P;
}
size_t hc_fri_plan_num_requests(void* p) { return ((HcPlan*)p)->plan.req.size(); }
int hc_fri_plan_requests(void* p, uint32_t* kind, uint32_t* which, uint32_t* level, uint64_t* index) {
    auto& rq = ((HcPlan*)p)->plan.req;
    for (size_t i = 0; i < rq.size(); ++i) { kind[i] = rq[i].kind; which[i] = rq[i].which; level[i] = rq[i].level; index[i] = rq[i].index; }
    return 0;
}
// returns the encoded length (0 on error); writes at most cap bytes
size_t hc_fri_plan_assemble(void* p, const uint64_t* values, size_t n_values, uint8_t* buf, size_t cap, size_t* est) {
    HcPlan* P = (HcPlan*)p; if (n_values != P->plan.req.size()) return 0;
    std::vector<fr_t> v(n_values); for (size_t i = 0; i < n_values; ++i) v[i] = ld4(values + 4 * i);
    ReplaySource src(v.data(), v.size()); HcHasher H(P->tp); std::vector<uint8_t> b; size_t e = 0;
    if (assemble_proof(P->plan.shape, P->plan.r, H, src, b, e) || src.pos != v.size()) return 0;
    if (est) *est = e;
    if (buf && cap >= b.size()) memcpy(buf, b.data(), b.size());
    return b.size();
}
void hc_fri_plan_free(void* p) { delete (HcPlan*)p; }

// ---- verifiers: the batch plans (fri_verify_batch.hpp, merkle_batch.hpp) run step by step as the device runs them, every hash by the host
// instantiation of the kernel bodies.  A single proof is a plan of one item. -------------
// The Merkle parameters per width, derived once per process (t = 129 takes a while on the host)
struct HcParamCache {
    std::map<int, HcParams*> mp;
    ~HcParamCache() { for (auto& kv : mp) delete kv.second; }
    HcParams* params(size_t arity) { int t = host::width_for_arity(arity); auto it = mp.find(t); if (it != mp.end()) return it->second; HcParams* P = new HcParams(); P->ref = host::consts_for_width(t); bind(P); mp[t] = P; return P; }
};
static HcParamCache& hc_param_cache() { static HcParamCache c; return c; }
// One plan: the leaf step (tparams: the transcript parameters; read only when the plan has leaves), then every (width, depth) group of gathered DS
// hashes in depth order, then the per-item root comparisons.
static void run_plan_host(VerifyBatchPlan V, const HcParams* tparams, int32_t* accepted) {
    { std::vector<fr_t> dev = hc_fr_block(V.pool.size()); std::copy(V.pool.begin(), V.pool.begin() + V.n_known, dev.begin()); V.pool.swap(dev); }   // run_verify_batch uploads the known prefix only
    if (V.nl) {
        fr_t init[17]; leaf_init(init);
        const LeafStream LS{init, V.pool.data() + V.leaf_f0, V.pool.data() + V.leaf_f0 + V.nl, 1, V.nl};
        fr_t st[17]; for (size_t j = 0; j < V.nl; ++j) { ArrayState s{st}; V.pool[V.leaf_out0 + j] = leaf_pair_body(s, tparams->dev, LS, j); }
    }
    for (const VerifyBatchPlan::Group& G : V.groups) {
        hash_ds_stream(hc_param_cache().params((size_t)G.t - 1), DsGatherStream{V.hdr.data() + 4 * G.job0, V.off.data() + G.job0, V.idx.data(), V.pool.data(), G.n, G.max_children}, V.pool.data() + G.out0);
    }
    for (size_t b = 0; b < V.batch; ++b) {
        int32_t acc = V.flag[b];
        for (uint32_t j = V.chk_off[b]; j < V.chk_off[b + 1]; ++j) acc &= fr_eq(V.pool[V.chk[2 * j]], V.pool[V.chk[2 * j + 1]]) ? 1 : 0;
        accepted[b] = acc;
    }
}
// deep_fri_verify over `batch` proofs through the batch plan.  accepted[i] = 1 / 0.
int hc_deep_fri_verify_batch(void* tparams, size_t batch, const uint8_t* const* proofs, const size_t* lens, const size_t* schedule, size_t L, size_t r, int32_t* accepted) {
    VerifyBatchPlanner pl; for (size_t b = 0; b < batch; ++b) pl.add(proofs[b], lens[b], schedule, L, r);
    if (!pl.fits_u32()) return -1;
    VerifyBatchPlan V; pl.finish(V);
    run_plan_host(std::move(V), (const HcParams*)tparams, accepted);
    return 0;
}
// 1 accept, 0 reject, negative: internal error
int hc_deep_fri_verify(void* tparams, const uint8_t* bytes, size_t len, const size_t* schedule, size_t L, size_t r) {
    int32_t acc = 0; const int rc = hc_deep_fri_verify_batch(tparams, 1, &bytes, &len, schedule, L, r, &acc);
    return rc ? rc : acc;
}
// the launch steps of the batch plan: (width, depth, hashes) of each DS group, in launch order; returns the number of groups (at most cap written)
size_t hc_verify_batch_groups(size_t batch, const uint8_t* const* proofs, const size_t* lens, const size_t* schedule, size_t L, size_t r, int32_t* t, uint32_t* depth, size_t* n, size_t cap) {
    VerifyBatchPlanner pl; for (size_t b = 0; b < batch; ++b) pl.add(proofs[b], lens[b], schedule, L, r);
    VerifyBatchPlan V; pl.finish(V);
    for (size_t g = 0; g < V.groups.size() && g < cap; ++g) { t[g] = V.groups[g].t; depth[g] = V.groups[g].depth; n[g] = V.groups[g].n; }
    return V.groups.size();
}
// MerkleProver::verify_single / verify_pairs (merkle/src/lib.rs:800-855) over the canonical MerkleProof encoding
int hc_merkle_verify(void* tparams, int pairs, size_t cfg_arity, uint64_t label, const uint64_t* root, const size_t* idx, size_t k, const uint64_t* vals, const uint64_t* cp, const uint8_t* proof, size_t len) {
    (void)tparams;                                                     // a Merkle plan has no leaf step
    const uint64_t none[4] = {0, 0, 0, 0};                             // pairs mode is chosen by a non-null cp: an empty pairs request still goes the pairs way
    MerkleVerifyPlanner pl; pl.add(cfg_arity, label, root, idx, k, vals, pairs ? (cp ? cp : none) : nullptr, proof, len);
    if (!pl.fits_u32()) return -1;
    VerifyBatchPlan V; pl.finish(V);
    int32_t acc = 0; run_plan_host(std::move(V), nullptr, &acc);
    return acc;
}

}  // extern "C"

// ---- the batched sum-check provers (sumcheck_batch.hpp) through the host instantiation of the kernel bodies -------------------------
struct ScHostExec : HostArena {
    HcParams* cp; HcParams* tp;
    ScHostExec(HcParams* c, HcParams* t) : cp(c), tp(t) {}
    template <class DS> int32_t hash_level(const DS& D, fr_t* out) { return hash_ds_stream(cp, D, out); }
    int32_t coeffs(const fr_t* const* ptrs, const fr_t* layers, size_t len, size_t B, fr_t* c01, fr_t* claim, size_t claim_from) {
        for (size_t b = 0; b < B; ++b) {
            const fr_t* l = ptrs ? ptrs[b] : layers + b * len; fr_t c0 = fr_zero<PF>(), c1 = fr_zero<PF>();
            for (size_t j = 0; j < len / 2; ++j) { c0 = fr_add<PF>(c0, l[2 * j]); c1 = fr_add<PF>(c1, fr_sub<PF>(l[2 * j + 1], l[2 * j])); }
            c01[2 * b] = c0; c01[2 * b + 1] = c1; if (claim && b >= claim_from) claim[b] = fr_add<PF>(fr_add<PF>(c0, c0), c1);
        }
        return 0;
    }
    int32_t fold(const fr_t* const* ptrs, const fr_t* layers, size_t len, size_t B, const fr_t* r, fr_t* next) {
        for (size_t b = 0; b < B; ++b) {
            const fr_t* l = ptrs ? ptrs[b] : layers + b * len;
            for (size_t j = 0; j < len / 2; ++j) next[b * (len / 2) + j] = fr_add<PF>(l[2 * j], fr_mul<PF>(r[b], fr_sub<PF>(l[2 * j + 1], l[2 * j])));
        }
        return 0;
    }
    int32_t transcript(const TrBatchStream& T) { fr_t st[17]; for (size_t a = 0; a < T.n_active; ++a) { ArrayState s{st}; tr_batch_body(s, tp->dev, T, a); } return 0; }
    int32_t gather(const fr_t* const* addr, size_t n, fr_t* out) { for (size_t j = 0; j < n; ++j) out[j] = *addr[j]; return 0; }
};
extern "C" {
// One Merkle level of B same-shape trees (DsBatchStream): in = B x n_in contiguous (by_ptrs: read through a pointer per tree), labels[b]
int hc_hash_ds_batch_level(void* params, size_t arity, uint32_t level, uint64_t pos0, const uint64_t* labels, const uint64_t* in, size_t n_in, size_t trees, int by_ptrs, uint64_t* out) {
    HcParams* P = (HcParams*)params;
    std::vector<fr_t> a(n_in * trees); for (size_t i = 0; i < a.size(); ++i) a[i] = ld4(in + 4 * i);
    std::vector<const fr_t*> ptrs(trees); for (size_t b = 0; b < trees; ++b) ptrs[b] = a.data() + b * n_in;
    return hash_ds_stream(P, DsBatchStream::make(arity, level, pos0, labels, by_ptrs ? ptrs.data() : nullptr, by_ptrs ? nullptr : a.data(), n_in, trees), out);
}
// One launch of a TrBatchStream: state (17 per instance) and pos updated in place; out[a * nseg + s] per finished segment.
int hc_tr_batch(void* tparams, uint64_t* state, uint32_t* pos, size_t n_inst, const uint32_t* inst, size_t inst0, size_t n_active, size_t nseg, const uint32_t* el_off,
                const uint32_t* idx, const uint64_t* pool0, size_t n0, const uint64_t* pool1, size_t n1, int reset, int finish_last, uint64_t* out) {
    HcParams* P = (HcParams*)tparams;
    std::vector<fr_t> st(17 * n_inst), p0(n0), p1(n1), o(n_active * nseg, host::h_zero());
    for (size_t i = 0; i < st.size(); ++i) st[i] = ld4(state + 4 * i);
    for (size_t i = 0; i < n0; ++i) p0[i] = ld4(pool0 + 4 * i); for (size_t i = 0; i < n1; ++i) p1[i] = ld4(pool1 + 4 * i);
    TrBatchStream T; T.state = st.data(); T.pos = pos; T.inst = inst; T.inst0 = inst0; T.n_active = n_active; T.nseg = nseg; T.el_off = el_off; T.idx = idx;
    T.pool0 = p0.data(); T.pool1 = p1.data(); T.out = o.data(); T.init_cap = host::h_tag("FSv1-TRANSCRIPT-INIT"); T.reset_from = reset ? 0 : n_active; T.finish_last = finish_last;
    fr_t s17[17]; for (size_t a = 0; a < n_active; ++a) { ArrayState s{s17}; tr_batch_body(s, P->dev, T, a); }
    for (size_t i = 0; i < st.size(); ++i) st4(state + 4 * i, st[i]);
    for (size_t i = 0; i < o.size(); ++i) st4(out + 4 * i, o[i]);
    return 0;
}
// prove_plain (mf = 0) / prove_mf (mf = 1) of B witnesses (host arrays of 2^k elements) through the batched driver.  Writes the proofs back
// to back into buf when cap suffices, their lengths into lens; returns the total length (0 on error).
size_t hc_sumcheck_prove_batch(void* tparams, void* cparams, int mf, size_t B, const uint64_t* const* witnesses, size_t k, const uint64_t* labels, size_t q,
                               uint8_t* buf, size_t cap, size_t* lens) {
    const size_t n = (size_t)1 << k;
    std::vector<std::vector<fr_t>> w(B, std::vector<fr_t>(n)); std::vector<const fr_t*> wp(B);
    for (size_t b = 0; b < B; ++b) { for (size_t i = 0; i < n; ++i) w[b][i] = ld4(witnesses[b] + 4 * i); wp[b] = w[b].data(); }
    ScHostExec X((HcParams*)cparams, (HcParams*)tparams);
    const std::vector<size_t> ks(B, k);
    ScBatch<ScHostExec> S(X, B, wp.data(), ks.data(), labels);
    std::vector<std::vector<uint8_t>> pr;
    if (mf ? S.prove_mf(q, pr) : S.prove_plain(pr)) return 0;
    size_t tot = 0; for (size_t b = 0; b < B; ++b) { lens[b] = pr[b].size(); tot += pr[b].size(); }
    if (buf && cap >= tot) { size_t o = 0; for (auto& p : pr) { memcpy(buf + o, p.data(), p.size()); o += p.size(); } }
    return tot;
}
// The same of witnesses of different sizes: witness b has 2^k[b] elements (k[b] <= 40).  As hc_sumcheck_prove_batch otherwise.
size_t hc_sumcheck_prove_mixed_batch(void* tparams, void* cparams, int mf, size_t B, const uint64_t* const* witnesses, const size_t* k, const uint64_t* labels, size_t q,
                                     uint8_t* buf, size_t cap, size_t* lens) {
    std::vector<std::vector<fr_t>> w(B); std::vector<const fr_t*> wp(B);
    for (size_t b = 0; b < B; ++b) {
        if (k[b] > 40) return 0;
        const size_t n = (size_t)1 << k[b]; w[b].resize(n);
        for (size_t i = 0; i < n; ++i) w[b][i] = ld4(witnesses[b] + 4 * i);
        wp[b] = w[b].data();
    }
    ScHostExec X((HcParams*)cparams, (HcParams*)tparams);
    ScBatch<ScHostExec> S(X, B, wp.data(), k, labels);
    std::vector<std::vector<uint8_t>> pr;
    if (mf ? S.prove_mf(q, pr) : S.prove_plain(pr)) return 0;
    size_t tot = 0; for (size_t b = 0; b < B; ++b) { lens[b] = pr[b].size(); tot += pr[b].size(); }
    if (buf && cap >= tot) { size_t o = 0; for (auto& p : pr) { memcpy(buf + o, p.data(), p.size()); o += p.size(); } }
    return tot;
}
}  // extern "C"

// ---- the batched sum-check verifiers (sumcheck_verify_batch.hpp): the plan run step by step as the device runs it -------------------
static int sc_verify_plan(int mf, size_t batch, const uint8_t* const* proofs, const size_t* lens, const uint64_t* labels, ScVerifyPlan& V) {
    bool fits = false;
    if (sc_verify_plan_some(mf, 0, batch, proofs, lens, labels, (size_t)-1, V, fits) != batch || !fits) return -1;
    return 0;
}
extern "C" {
// The decode body on the element at byte `off` of `blob` (len bytes): 1 and out4 = the stored form, 0 when the value is >= r.
int hc_sc_decode_fr(const uint8_t* blob, size_t len, size_t off, uint64_t* out4) {
    if (off + 32 > len) return -1;
    std::vector<uint32_t> w((len + 3) / 4 + 2, 0u); memcpy(w.data(), blob, len);
    fr_t x; const bool ok = sc_decode_fr(w.data(), (uint32_t)off, 0u, x); st4(out4, x); return ok ? 1 : 0;
}
// One plan run step by step: decode, the transcript streams, the DS groups in depth order (cp: MerkleCommitment's parameters), the checks.
// accepted[i] = 1 / 0 for the V.batch proofs of the plan.
static void run_sc_plan_host(ScVerifyPlan& V, HcParams* tp, HcParams* cp, int32_t* accepted) {
    const int mf = V.mf;
    std::vector<fr_t> pool = hc_fr_block(std::max<size_t>(V.pool_slots, 1));       // run_sc_verify_batch: the pool, the states and the cursors are not uploaded
    for (size_t j = 0; j < V.n_dec; ++j) if (!sc_decode_fr(V.blob.data(), V.dec_off[j], V.dec_proof[j], pool[j])) V.flag[V.dec_proof[j] & ~kScClaim] = 0;
    std::vector<fr_t> state = hc_fr_block(17 * std::max<size_t>(V.n_inst, 1)); std::vector<uint32_t> pos(std::max<size_t>(V.n_inst, 1), 0x01010101u * (uint32_t)g_alloc_fill);
    for (const ScVerifyPlan::Stream& S : V.tr) {
        TrBatchStream T; T.state = state.data(); T.pos = pos.data(); T.inst = nullptr; T.inst0 = S.inst0; T.n_active = S.n; T.nseg = S.nseg; T.el_off = V.tr_off.data() + S.seg0;
        T.idx = V.tr_idx.data(); T.pool0 = pool.data(); T.pool1 = V.consts.data(); T.out = pool.data() + V.n_dec + S.seg0; T.init_cap = host::h_tag("FSv1-TRANSCRIPT-INIT"); T.reset_from = 0; T.finish_last = 1;
        fr_t st[17]; for (size_t a = 0; a < S.n; ++a) { ArrayState s{st}; tr_batch_body(s, tp->dev, T, a); }
    }
    for (const VerifyBatchPlan::Group& G : V.ds.groups) {
        hash_ds_stream(cp, DsGatherStream{V.ds.hdr.data() + 4 * G.job0, V.ds.off.data() + G.job0, V.ds.idx.data(), pool.data(), G.n, G.max_children}, pool.data() + G.out0);
    }
    for (size_t j = 0; j < V.n_rec(); ++j) {
        const uint32_t* r = V.rec.data() + 8 * j;
        if (!(mf ? sc_check_mf(pool.data(), r) : sc_check_plain(pool.data(), r))) V.flag[mf ? r[1] : r[0]] = 0;
    }
    for (size_t b = 0; b < V.batch; ++b) accepted[b] = V.flag[b];
}
// verify_plain (mf = 0; labels may be null) / verify_mf (mf = 1) of `batch` proofs through one batch plan.  accepted[i] = 1 / 0.
int hc_sumcheck_verify_batch(void* tparams, void* cparams, int mf, size_t batch, const uint8_t* const* proofs, const size_t* lens, const uint64_t* labels, int32_t* accepted) {
    ScVerifyPlan V; if (sc_verify_plan(mf, batch, proofs, lens, labels, V)) return -1;
    run_sc_plan_host(V, (HcParams*)tparams, (HcParams*)cparams, accepted);
    return 0;
}
// the same cut into plans of at most max_slots pool slots each (at least one proof a plan), as the device driver cuts a batch under the
// context's "sumcheck_verify_batch_max_slots"
int hc_sumcheck_verify_batch_slots(void* tparams, void* cparams, int mf, size_t batch, const uint8_t* const* proofs, const size_t* lens, const uint64_t* labels, size_t max_slots, int32_t* accepted) {
    size_t b0 = 0;
    while (b0 < batch) {
        ScVerifyPlan V; bool fits = false;
        const size_t b1 = sc_verify_plan_some(mf, b0, batch, proofs, lens, labels, max_slots, V, fits);
        if (!fits) return -1;
        run_sc_plan_host(V, (HcParams*)tparams, (HcParams*)cparams, accepted + b0);
        b0 = b1;
    }
    return 0;
}
// the device steps of the plan as (kind, count) rows in launch order (ScVerifyPlan::steps); returns their number (at most cap written)
size_t hc_sumcheck_verify_batch_steps(int mf, size_t batch, const uint8_t* const* proofs, const size_t* lens, const uint64_t* labels, int32_t* kind, size_t* count, size_t cap) {
    ScVerifyPlan V; if (sc_verify_plan(mf, batch, proofs, lens, labels, V)) return 0;
    const auto st = V.steps();
    for (size_t i = 0; i < st.size() && i < cap; ++i) { kind[i] = st[i].first; count[i] = st[i].second; }
    return st.size();
}
}  // extern "C"

// ---- the batched commit phase (fri_batch.hpp) through the host instantiation of the stream bodies ----------------------------------
struct FriHostExec : HostArena {
    HcParams* tp;
    HcParamCache& mp;
    explicit FriHostExec(HcParams* t) : tp(t), mp(hc_param_cache()) {}
    int32_t zpows(const fr_t& z, size_t m, fr_t* zp) { fr_t acc = fr_one<PF>(); for (size_t t = 0; t < m; ++t) { zp[t] = acc; acc = fr_mul<PF>(acc, z); } return 0; }
    int32_t fold(const fr_t* f, size_t n, const fr_t* zp, size_t m, fr_t* out) {                                   // fri_fold_layer (fri.rs:85-102)
        for (size_t b = 0; b < n / m; ++b) { fr_t acc = fr_zero<PF>(); for (size_t t = 0; t < m; ++t) acc = fr_add<PF>(acc, fr_mul<PF>(f[b * m + t], zp[t])); out[b] = acc; }
        return 0;
    }
    int32_t leaf_pairs(const fr_t* f, const fr_t* f_next, size_t n, size_t m, fr_t* h) {
        fr_t init[17]; leaf_init(init); const LeafStream LS{init, f, f_next, m, n};
        fr_t st[17]; for (size_t i = 0; i < n; ++i) { ArrayState s{st}; h[i] = leaf_pair_body(s, tp->dev, LS, i); }
        return 0;
    }
    template <class DS> int32_t hash_level(size_t arity, const DS& D, fr_t* out) { return hash_ds_stream(mp.params(arity), D, out); }
    int32_t fork() { return 0; }
    void side(bool) {}
    int32_t join() { return 0; }
};
extern "C" {
// The pair leaves of `trees` same-shape unhashed layers (DsBatchPairStream): f = trees x n, cp = trees x (n / cp_div) or null, labels[b]
int hc_hash_ds_batch_pairs_level(void* params, size_t arity, const uint64_t* labels, const uint64_t* f, const uint64_t* cp, size_t n, size_t cp_div, size_t trees, uint64_t* out) {
    HcParams* P = (HcParams*)params;
    if (!cp_div || n % cp_div) return -1;
    std::vector<fr_t> a(n * trees), b(cp ? n / cp_div * trees : 0);
    for (size_t i = 0; i < a.size(); ++i) a[i] = ld4(f + 4 * i);
    for (size_t i = 0; i < b.size(); ++i) b[i] = ld4(cp + 4 * i);
    return hash_ds_stream(P, DsBatchPairStream::make(arity, labels, a.data(), cp ? b.data() : nullptr, n, cp_div, trees), out);
}
// The commit phase of B traces side by side (FriBatchCommit): roots[(b (L + 1) + l) * 4 ..] = root of layer l of trace b.  0 on success.
int hc_fri_commit_batch(void* tparams, size_t B, const uint64_t* const* f0, size_t n0, const size_t* schedule, size_t L, uint64_t seed_z, uint64_t* roots) {
    FriHostExec X((HcParams*)tparams); FriBatchCommit<FriHostExec> C(X);
    std::string err; if (int rc = C.shape(B, n0, schedule, L, err)) return rc;
    HcHasher H(tparams); std::vector<fr_t> z(L);
    for (size_t l = 0; l < L; ++l) {
        const fr_t in[3] = {host::h_u64(seed_z), host::h_u64(l), host::h_u64(C.n[l])}; fr_t fused; if (H.hash("FRI/z/l", in, 3, 1, &fused)) return -3;
        z[l] = fri_z_from_fused(fused, seed_z, l, C.n[l]);
    }
    if (int rc = C.init(z.data())) return rc;
    for (size_t b = 0; b < B; ++b) for (size_t i = 0; i < n0; ++i) C.f[0][b * n0 + i] = ld4(f0[b] + 4 * i);
    if (int rc = C.run()) return rc;
    for (size_t b = 0; b < B; ++b) for (size_t l = 0; l <= L; ++l) st4(roots + 4 * (b * (L + 1) + l), C.roots[l * B + b]);
    return 0;
}
}  // extern "C"

// ---- the pass cutting and the overlap check of stark_ntt_batch_dev / stark_lde_batch_dev: the rules of ntt_mixed_plan.hpp on equal lengths -------------
extern "C" {
// columns per pass into out[0 .. cap); returns the number of passes
size_t hc_ntt_batch_passes(size_t batch, int log_out, size_t max_elems, size_t* out, size_t cap) {
    const std::vector<size_t> lg(batch, (size_t)log_out), p = ntt_mixed_passes(batch, lg.data(), max_elems);
    for (size_t i = 0; i < p.size() && i < cap; ++i) out[i] = p[i];
    return p.size();
}
int hc_ntt_batch_ranges_overlap(const uint64_t* starts, size_t batch, size_t bytes) {
    std::vector<const void*> p(batch); for (size_t i = 0; i < batch; ++i) p[i] = (const void*)(uintptr_t)starts[i];
    const std::vector<size_t> len(batch, bytes);
    return ntt_batch_ranges_overlap(p.data(), batch, len.data()) ? 1 : 0;
}
}  // extern "C"

// ---- stark_ntt_mixed_batch_dev / stark_lde_mixed_batch_dev (ntt_mixed_plan.hpp): tile lookup, pass cutting, overlap check and the launch plan --------
extern "C" {
uint32_t hc_ntt_ragged_locate(const uint32_t* first_tile, uint32_t ncols, uint32_t t) { return ntt_ragged_locate(first_tile, ncols, t); }
size_t hc_ntt_mixed_passes(size_t batch, const size_t* log_out, size_t max_elems, size_t* out, size_t cap) {
    const std::vector<size_t> p = ntt_mixed_passes(batch, log_out, max_elems);
    for (size_t i = 0; i < p.size() && i < cap; ++i) out[i] = p[i];
    return p.size();
}
int hc_ntt_mixed_ranges_overlap(const uint64_t* starts, const size_t* bytes, size_t batch) {
    std::vector<const void*> p(batch); for (size_t i = 0; i < batch; ++i) p[i] = (const void*)(uintptr_t)starts[i];
    return ntt_batch_ranges_overlap(p.data(), batch, bytes) ? 1 : 0;
}
// The plan of one pass as a stream of int64 (returns the words the whole plan takes; only the first `cap` are written):
//   scratch_elems, launches, then per launch  kind, step, strided, pre, ntiles, lds, nshapes, ncols,
//   nshapes x (log_n, P, pass, log_b, log_c, log_m, log_nonzero, tiles),  ncols x (col, shape, first_tile, src.mem, src.off, dst.mem, dst.off, first, head, len).
// lde == 0: in-place transforms (log_blowup unused); lde != 0: extensions (inverse unused; coset: the shift is given and not one).
size_t hc_ntt_mixed_plan(size_t ncols, const size_t* log_n, int lde, int inverse, int coset, size_t log_blowup, int log_tile, int tile_forced, int64_t* out, size_t cap) {
    NttTileOpts o; o.log_tile = log_tile; o.forced = tile_forced != 0;
    const NttMixedPlan plan = lde ? ntt_mixed_lde_plan(log_n, ncols, (int)log_blowup, coset != 0, o) : ntt_mixed_ntt_plan(log_n, ncols, inverse != 0, coset != 0, o);
    std::vector<int64_t> w{(int64_t)plan.scratch_elems, (int64_t)plan.launches.size()};
    for (const NttMixedLaunch& L : plan.launches) {
        w.insert(w.end(), {L.kind, L.step, L.strided, L.pre, (int64_t)L.ntiles, (int64_t)L.lds, (int64_t)L.shapes.size(), (int64_t)L.cols.size()});
        for (const NttMixedShape& s : L.shapes) w.insert(w.end(), {s.log_n, s.P, s.pass, s.log_b, s.log_c, s.log_m, s.log_nonzero, (int64_t)s.tiles});
        for (const NttMixedCol& c : L.cols) w.insert(w.end(), {c.col, c.shape, c.first_tile, c.src.mem, (int64_t)c.src.off, c.dst.mem, (int64_t)c.dst.off, (int64_t)c.first, (int64_t)c.head, (int64_t)c.len});
    }
    for (size_t i = 0; i < w.size() && i < cap; ++i) out[i] = w[i];
    return w.size();
}
// ntt_mixed_one_shape of every launch of the same plan, seven int64 per launch: holds, then (zeros unless it holds) src.mem, src.off, src.pitch, dst.mem,
// dst.off, dst.pitch.  Returns the number of launches; only the first `cap` words are written.
size_t hc_ntt_mixed_one_shape(size_t ncols, const size_t* log_n, int lde, int inverse, int coset, size_t log_blowup, int log_tile, int tile_forced, int64_t* out, size_t cap) {
    NttTileOpts o; o.log_tile = log_tile; o.forced = tile_forced != 0;
    const NttMixedPlan plan = lde ? ntt_mixed_lde_plan(log_n, ncols, (int)log_blowup, coset != 0, o) : ntt_mixed_ntt_plan(log_n, ncols, inverse != 0, coset != 0, o);
    std::vector<int64_t> w;
    for (const NttMixedLaunch& L : plan.launches) {
        NttOneShape S; const bool one = ntt_mixed_one_shape(L, &S);
        if (one) w.insert(w.end(), {1, S.src.mem, (int64_t)S.src.off, (int64_t)S.src.pitch, S.dst.mem, (int64_t)S.dst.off, (int64_t)S.dst.pitch});
        else w.insert(w.end(), {0, 0, 0, 0, 0, 0, 0});
    }
    for (size_t i = 0; i < w.size() && i < cap; ++i) out[i] = w[i];
    return plan.launches.size();
}
}  // extern "C"

// ---- stark_mle_evaluate_batch_dev (mle_dev.hpp): the passes of the driver, every workgroup of k_mle_fold_pass run in lockstep on the host ----------
// One pass: the lane geometry, the lane-local fold and the wave stage are the kernel's own inline pieces; a shuffle is a read of the partner's slot.
template <int C>
static void mle_pass_host(bool contig, size_t B, const fr_t* const* ptrs, const fr_t* layers, uint64_t len, int t, const fr_t* r, size_t k, size_t j0, fr_t* next) {
    const int x = t - C; const uint64_t blocks = ((len >> C) + 255) / 256;
    for (size_t b = 0; b < B; ++b) {
        const fr_t* layer = ptrs ? ptrs[b] : layers + b * len; const fr_t* rr = r + b * k + j0; fr_t* dst = next + b * (len >> t);
        for (uint64_t blk = 0; blk < blocks; ++blk) {
            fr_t v[256], u[256]; MleLane L[256]; bool live[256];
            for (int tid = 0; tid < 256; ++tid) {
                L[tid] = mle_lane(blk * 256 + tid, t, C, contig); live[tid] = L[tid].first < len;
                v[tid] = live[tid] ? mle_fold_local<C>(layer + L[tid].first, L[tid].stride, rr + L[tid].local0) : fr_zero<PF>();
            }
            for (int s = 0; s < 6 && s < x; ++s) {
                for (int tid = 0; tid < 256; ++tid) u[tid] = mle_fold1(v[tid], v[tid ^ (1 << s)], rr[L[tid].cross0 + s]);
                std::copy(u, u + 256, v);
            }
            if (x <= 6) { for (int tid = 0; tid < 256; ++tid) if (live[tid] && (tid & ((1 << x) - 1)) == 0) dst[L[tid].tile] = v[tid]; continue; }
            const fr_t w[4] = {v[0], v[64], v[128], v[192]};
            for (int tid = 0; tid < (4 >> (x - 6)); ++tid) {
                const uint64_t tile = (blk << (kMleLogThreads - x)) + tid;
                if ((tile << t) < len) dst[tile] = mle_fold_waves(w, x, tid, rr[L[tid].cross0 + 6], x == 8 ? rr[L[tid].cross0 + 7] : fr_zero<PF>());
            }
        }
    }
}
extern "C" {
// out[b] = Mle::evaluate of tables[b] (2^k elements) at r[b * k ..], through the driver's passes with tile 2^log_tile (-1: the default) and the lane
// ownership `contig` (-1: the default).  passes (may be null) = the number of launches one evaluation takes.  -1: log_tile out of range.
int hc_mle_evaluate_batch(size_t B, const uint64_t* const* tables, size_t k, const uint64_t* r, int log_tile, int contig, uint64_t* out, size_t* passes) {
    const int T = log_tile < 0 ? kMleDefaultLogTile : log_tile;
    if (T < kMleMinLogTile || T > kMleMaxLogTile || k > 40) return -1;
    const bool cg = (contig < 0 ? kMleDefaultContig : contig) != 0;
    const std::vector<int> rounds = mle_pass_rounds(k, T);
    if (passes) *passes = rounds.size();
    std::vector<std::vector<fr_t>> tab(B, std::vector<fr_t>((size_t)1 << k)); std::vector<const fr_t*> ptrs(B); std::vector<fr_t> rv(B * k);
    for (size_t b = 0; b < B; ++b) { for (size_t i = 0; i < tab[b].size(); ++i) tab[b][i] = ld4(tables[b] + 4 * i); ptrs[b] = tab[b].data(); }
    for (size_t i = 0; i < rv.size(); ++i) rv[i] = ld4(r + 4 * i);
    if (k == 0) { for (size_t b = 0; b < B; ++b) st4(out + 4 * b, tab[b][0]); return 0; }
    std::vector<fr_t> cur, nxt; size_t j0 = 0;
    for (size_t i = 0; i < rounds.size(); ++i) {
        const int t = rounds[i]; const uint64_t len = (uint64_t)1 << (k - j0);
        nxt = hc_fr_block(B * (len >> t));                                                 // a pooled intermediate layer of the device driver
        switch (mle_local_rounds(t)) {
            case 0: mle_pass_host<0>(cg, B, i ? nullptr : ptrs.data(), cur.data(), len, t, rv.data(), k, j0, nxt.data()); break;
            case 1: mle_pass_host<1>(cg, B, i ? nullptr : ptrs.data(), cur.data(), len, t, rv.data(), k, j0, nxt.data()); break;
            case 2: mle_pass_host<2>(cg, B, i ? nullptr : ptrs.data(), cur.data(), len, t, rv.data(), k, j0, nxt.data()); break;
            case 3: mle_pass_host<3>(cg, B, i ? nullptr : ptrs.data(), cur.data(), len, t, rv.data(), k, j0, nxt.data()); break;
            case 4: mle_pass_host<4>(cg, B, i ? nullptr : ptrs.data(), cur.data(), len, t, rv.data(), k, j0, nxt.data()); break;
            default: return -1;
        }
        cur.swap(nxt); j0 += (size_t)t;
    }
    for (size_t b = 0; b < B; ++b) st4(out + 4 * b, cur[b]);
    return 0;
}
}  // extern "C"
extern "C" int hc_mle_default_log_tile() { return kMleDefaultLogTile; }

// ---- stark_lagrange_eval_on_h_batch_dev (lagrange_dev.hpp): the driver itself, every workgroup of k_lagrange_partials run in lockstep on the host ------
// The lane geometry, the weights, the lane dot product and the sums are the kernels' own inline pieces; a shuffle scan is a product over the wave's
// other lanes, LDS a plain array.  Blocks come from the executors' allocation path (hc_set_alloc_fill), as the device driver's come from the pool.
struct LagHostExec : HostArena {
    std::vector<fr_t> lo, hi;
    int32_t pow_table(const fr_t& omega, size_t n, LagPow* out) {
        int bits, lo_bits, hi_bits; lag_pow_split(n, &bits, &lo_bits, &hi_bits);
        lo.assign((size_t)1 << lo_bits, fr_one<PF>()); hi.assign((size_t)1 << hi_bits, fr_one<PF>());
        for (size_t i = 1; i < lo.size(); ++i) lo[i] = fr_mul<PF>(lo[i - 1], omega);
        const fr_t step = fr_pow_u64<PF>(omega, (uint64_t)1 << lo_bits);
        for (size_t i = 1; i < hi.size(); ++i) hi[i] = fr_mul<PF>(hi[i - 1], step);
        *out = LagPow{lo.data(), hi.data(), lo_bits}; return 0;
    }
    int32_t gather(const fr_t* const* cols, size_t ncols, const uint64_t* j, const uint64_t* slot, size_t cnt, fr_t* out) {
        for (size_t q = 0; q < cnt; ++q) for (size_t c = 0; c < ncols; ++c) out[slot[q] * ncols + c] = j[q] == kLagNoRow ? fr_zero<PF>() : cols[c][j[q]];
        return 0;
    }
    // the census of a call: Fermat inversions; weight sets of k_lagrange_partials (workgroup x class evaluations of lag_prefix followed by a peel); products of
    // k_lagrange_totals (workgroup x point evaluations of lag_prefix); member walks of k_lagrange_partials (workgroup x member: what a weight set served)
    uint64_t census[4] = {0, 0, 0, 0};
    // the wave scan of 256 lanes' products: tot[v] = the product of wave v, others[t] = the product of the other lanes of t's wave
    static void scan(const std::vector<fr_t>& run, fr_t (&tot)[4], std::vector<fr_t>& others) {
        for (int v = 0; v < 4; ++v) { tot[v] = fr_one<PF>(); for (int l = 0; l < 64; ++l) tot[v] = fr_mul<PF>(tot[v], run[64 * v + l]); }
        for (int t = 0; t < 256; ++t) {
            const int v = t >> 6, l = t & 63; fr_t before = fr_one<PF>(), after = fr_one<PF>();
            for (int q = 0; q < l; ++q) before = fr_mul<PF>(before, run[64 * v + q]);
            for (int q = l + 1; q < 64; ++q) after = fr_mul<PF>(after, run[64 * v + q]);
            others[t] = fr_mul<PF>(before, after);
        }
    }
    int32_t totals(size_t n, uint64_t j0, const LagPow& wp, const fr_t& w_step, const fr_t* zs, size_t npts, unsigned grid, fr_t* totals) {      // k_lagrange_totals
        const uint32_t T = grid * 256, n32 = (uint32_t)n; fr_t pre[kLagK], t4[4];
        for (size_t p = 0; p < npts; ++p) for (unsigned blk = 0; blk < grid; ++blk) {
            for (int v = 0; v < 4; ++v) t4[v] = fr_one<PF>();
            for (int t = 0; t < 256; ++t) {
                const uint32_t tid = blk * 256 + t; fr_t w = tid < n32 ? lag_pow(wp, j0 + tid) : fr_one<PF>();
                t4[t >> 6] = fr_mul<PF>(t4[t >> 6], lag_prefix(zs[p], w, w_step, tid, T, n32, pre));
            }
            totals[p * grid + blk] = lag_mul4(t4); ++census[2];
        }
        return 0;
    }
    int32_t invert(const fr_t* totals, size_t npts, unsigned grid, fr_t* inv) {                                                                   // k_lagrange_invert
        std::vector<fr_t> run(256), others(256); fr_t tot[4];
        for (size_t p = 0; p < npts; ++p) {
            const fr_t* t = totals + p * grid; fr_t* o = inv + p * grid;
            for (int l = 0; l < 256; ++l) run[l] = lag_chunk_prefix(t, lag_chunk((uint32_t)l, grid), o);
            scan(run, tot, others);
            const fr_t Pinv = fr_inv<PF>(lag_mul4(tot)); ++census[0];
            for (int l = 0; l < 256; ++l) lag_chunk_peel(t, lag_chunk((uint32_t)l, grid), lag_lane_inverse(Pinv, tot, l >> 6, others[l]), o);
        }
        return 0;
    }
    int32_t partials(const fr_t* const* cols, size_t ncols, size_t n, uint64_t j0, const LagPow& wp, const fr_t& w_step, const fr_t& w_step_inv, const fr_t* zs, size_t npts, const LagEntries& E,
                     const fr_t* inv, unsigned groups, unsigned col_groups, size_t group_cols, unsigned grid, fr_t* part) {
        const uint32_t T = grid * 256, n32 = (uint32_t)n;
        std::vector<fr_t> Wv(256 * kLagK), w(256), run(256), lane(256), others(256);
        auto W = [&](int t) -> fr_t (&)[kLagK] { return *reinterpret_cast<fr_t (*)[kLagK]>(&Wv[(size_t)t * kLagK]); };
        for (unsigned cg = 0; cg < col_groups; ++cg) for (unsigned g = 0; g < groups; ++g) for (unsigned blk = 0; blk < grid; ++blk) {      // a workgroup per (tile, point group, column group), as on the device
            const size_t c_lo = (size_t)cg * group_cols, c_hi = std::min(c_lo + group_cols, ncols);
            for (int t = 0; t < 256; ++t) { const uint32_t tid = blk * 256 + t; w[t] = tid < n32 ? lag_pow(wp, j0 + tid) : fr_one<PF>(); }
            for (size_t p = g; p < npts; p += groups) {                                                                                      // the classes of the point group
                const fr_t z = zs[p];
                for (int t = 0; t < 256; ++t) run[t] = lag_prefix(z, w[t], w_step, blk * 256 + (uint32_t)t, T, n32, W(t));
                ++census[1];
                fr_t tot[4]; scan(run, tot, others);
                fr_t Pinv;
                if (inv) Pinv = inv[p * grid + blk]; else { Pinv = fr_inv<PF>(lag_mul4(tot)); ++census[0]; }
                for (int t = 0; t < 256; ++t) lag_peel(z, w[t], w_step_inv, blk * 256 + (uint32_t)t, T, n32, lag_lane_inverse(Pinv, tot, t >> 6, others[t]), W(t));
                const uint32_t m_lo = E.off ? E.off[p] : 0, m_hi = E.off ? E.off[p + 1] : 1;
                for (uint32_t m = m_lo; m < m_hi; ++m) {
                    const size_t q = E.off ? (size_t)E.member[m] : p; const uint32_t shift = E.off ? E.shift[m] : 0;
                    ++census[3];
                    for (size_t c = c_lo; c < c_hi; ++c) {
                        for (int t = 0; t < 256; ++t)
                            lane[t] = E.off ? lag_lane_dot<kLagWideAcc, true>(cols[c], blk * 256 + (uint32_t)t, T, n32, W(t), shift) : lag_lane_dot<kLagWideAcc>(cols[c], blk * 256 + (uint32_t)t, T, n32, W(t));
                        fr_t w4[4];
                        for (int v = 0; v < 4; ++v) { w4[v] = fr_zero<PF>(); for (int l = 0; l < 64; ++l) w4[v] = fr_add<PF>(w4[v], lane[64 * v + l]); }
                        part[(q * ncols + c) * grid + blk] = lag_sum4(w4);
                    }
                }
            }
        }
        return 0;
    }
    int32_t finish(const fr_t* part, unsigned grid, const fr_t* scale, const uint64_t* slot, size_t npts, size_t ncols, fr_t* out) {
        for (size_t b = 0; b < npts * ncols; ++b) {
            const size_t p = b / ncols, c = b % ncols; fr_t lane[256];
            for (int t = 0; t < 256; ++t) { lane[t] = fr_zero<PF>(); for (size_t i = (size_t)t; i < grid; i += 256) lane[t] = fr_add<PF>(lane[t], part[b * grid + i]); }
            fr_t w4[4];
            for (int w = 0; w < 4; ++w) { w4[w] = fr_zero<PF>(); for (int l = 0; l < 64; ++l) w4[w] = fr_add<PF>(w4[w], lane[64 * w + l]); }
            out[slot[p] * ncols + c] = scale ? fr_mul<PF>(lag_sum4(w4), scale[p]) : lag_sum4(w4);
        }
        return 0;
    }
    int32_t combine(const fr_t* partials, size_t nparts, const fr_t* scale, size_t npoints, size_t ncols, fr_t* out) {
        const size_t total = npoints * ncols;
        for (size_t i = 0; i < total; ++i) {
            fr_t acc = partials[i];
            for (size_t q = 1; q < nparts; ++q) acc = fr_add<PF>(acc, partials[q * total + i]);
            out[i] = fr_mul<PF>(acc, scale[i / ncols]);
        }
        return 0;
    }
};
// the domain of an entry point: false when (n, omega) is refused; *w = the caller's generator or the radix-2 one of size n
static bool hc_lag_domain(size_t n, const uint64_t* omega, fr_t* w) {
    if (!n || (n & (n - 1)) || n > ((size_t)1 << kLagMaxLogN)) return false;
    int lg = 0; while (((size_t)1 << lg) < n) ++lg;
    *w = omega ? ld4(omega) : fr_root_of_unity<PF>((unsigned)lg);
    return !lag_check_domain(n, *w);
}
// THE driver on the block B of the columns (cols[c]: B.n_local rows) with the host executor
static int hc_lag_block(size_t ncols, const uint64_t* const* cols, const LagBlock& B, const uint64_t* omega, size_t npoints, const uint64_t* z, size_t max_partials, int col_groups, uint64_t* out,
                        size_t* passes, int shared_inverse = 0, int share_cosets = 0, uint64_t* census4 = nullptr) {
    if (census4) for (int i = 0; i < 4; ++i) census4[i] = 0;
    if (passes) *passes = 0;
    if (!ncols || !npoints) return 0;
    fr_t w; if (!hc_lag_domain(B.n_global, omega, &w)) return -1;
    const size_t n = B.n_local;
    std::vector<std::vector<fr_t>> col(ncols, std::vector<fr_t>(n)); std::vector<const fr_t*> ptrs(ncols); std::vector<fr_t> zs(npoints);
    for (size_t c = 0; c < ncols; ++c) {
        size_t first = c; for (size_t q = 0; q < c; ++q) if (cols[q] == cols[c]) { first = q; break; }      // a repeated pointer stays one column
        if (first == c) for (size_t i = 0; i < n; ++i) col[c][i] = ld4(cols[c] + 4 * i);
        ptrs[c] = col[first].data();
    }
    for (size_t p = 0; p < npoints; ++p) zs[p] = ld4(z + 4 * p);
    std::vector<fr_t> o = hc_fr_block(npoints * ncols);
    LagHostExec X;
    if (int32_t rc = lagrange_eval_batch(X, ncols, ptrs.data(), B, w, npoints, zs.data(), max_partials ? max_partials : kLagDefaultMaxPartials, col_groups, shared_inverse, share_cosets, o.data(), passes))
        return hc_rc(rc);
    if (census4) for (int i = 0; i < 4; ++i) census4[i] = X.census[i];
    for (size_t i = 0; i < o.size(); ++i) st4(out + 4 * i, o[i]);
    return 0;
}
extern "C" {
// out[p * ncols + c] = lagrange_eval_on_h(cols[c] (n elements), z[p], omega) through the driver of stark_lagrange_eval_on_h_batch_dev with passes of at
// most max_partials block partials (0: the default).  omega null: the radix-2 generator of size n.  passes (may be null) = the partial passes taken.
// -1: a refused (n, omega), as the entry point refuses it.
int hc_lagrange_eval_batch(size_t ncols, const uint64_t* const* cols, size_t n, const uint64_t* omega, size_t npoints, const uint64_t* z, size_t max_partials, uint64_t* out, size_t* passes) {
    return hc_lag_block(ncols, cols, lag_whole(n), omega, npoints, z, max_partials, -1, out, passes);
}
// The block form, stark_lagrange_eval_shard_dev: cols[c] = the n_local rows [j0, j0 + n_local) of column c; partials_out[p * ncols + c] = the block's unscaled
// share.  col_groups: the option "lagrange_col_groups" (-1: automatic).  -1: refused as the entry point refuses it.
int hc_lagrange_eval_shard(size_t ncols, const uint64_t* const* cols, size_t n_local, uint64_t j0, size_t n_global, const uint64_t* omega, size_t npoints, const uint64_t* z, size_t max_partials,
                           int col_groups, uint64_t* partials_out, size_t* passes) {
    if (passes) *passes = 0;
    if (!ncols || !npoints) return 0;
    if (!n_local || j0 > n_global || n_local > n_global - j0) return -1;
    return hc_lag_block(ncols, cols, LagBlock{n_local, j0, n_global, false}, omega, npoints, z, max_partials, col_groups, partials_out, passes);
}
// hc_lagrange_eval_batch and hc_lagrange_eval_shard under the options "lagrange_shared_inverse" and "lagrange_share_cosets" (0 | 1), with "lagrange_col_groups"
// for both.  census4 (may be null) = LagHostExec::census of the call: Fermat inversions, weight sets of the partials kernel, products of the totals
// kernel, member walks.
int hc_lagrange_eval_batch_opt(size_t ncols, const uint64_t* const* cols, size_t n, const uint64_t* omega, size_t npoints, const uint64_t* z, size_t max_partials, int col_groups, int shared_inverse,
                               int share_cosets, uint64_t* out, size_t* passes, uint64_t* census4) {
    return hc_lag_block(ncols, cols, lag_whole(n), omega, npoints, z, max_partials, col_groups, out, passes, shared_inverse, share_cosets, census4);
}
int hc_lagrange_eval_shard_opt(size_t ncols, const uint64_t* const* cols, size_t n_local, uint64_t j0, size_t n_global, const uint64_t* omega, size_t npoints, const uint64_t* z, size_t max_partials,
                               int col_groups, int shared_inverse, int share_cosets, uint64_t* partials_out, size_t* passes, uint64_t* census4) {
    if (passes) *passes = 0;
    if (census4) for (int i = 0; i < 4; ++i) census4[i] = 0;
    if (!ncols || !npoints) return 0;
    if (!n_local || j0 > n_global || n_local > n_global - j0) return -1;
    return hc_lag_block(ncols, cols, LagBlock{n_local, j0, n_global, false}, omega, npoints, z, max_partials, col_groups, partials_out, passes, shared_inverse, share_cosets, census4);
}
// stark_lagrange_eval_from_partials_dev: out[p * ncols + c] = scale[p] * the sum of the nparts shares (lagrange_combine)
int hc_lagrange_eval_from_partials(size_t nparts, const uint64_t* partials, size_t ncols, size_t n_global, const uint64_t* omega, size_t npoints, const uint64_t* z, uint64_t* out) {
    if (!ncols || !npoints) return 0;
    fr_t w; if (!nparts || !hc_lag_domain(n_global, omega, &w)) return -1;
    const size_t total = npoints * ncols;
    std::vector<fr_t> part = hc_fr_block(nparts * total), o = hc_fr_block(total), zs(npoints);
    for (size_t i = 0; i < part.size(); ++i) part[i] = ld4(partials + 4 * i);
    for (size_t p = 0; p < npoints; ++p) zs[p] = ld4(z + 4 * p);
    LagHostExec X;
    if (int32_t rc = lagrange_combine(X, nparts, part.data(), ncols, n_global, npoints, zs.data(), o.data())) return hc_rc(rc);
    for (size_t i = 0; i < o.size(); ++i) st4(out + 4 * i, o[i]);
    return 0;
}
// The header of the sharded call's first collective (kLagHdrWords words) and the comparison every rank makes of the W gathered headers with its own
int hc_lagrange_shard_header(size_t n_global, size_t ncols, size_t npoints, const uint64_t* omega, const uint64_t* z, uint64_t* out8) {
    std::vector<fr_t> zs(npoints); for (size_t p = 0; p < npoints; ++p) zs[p] = ld4(z + 4 * p);
    lag_shard_header(n_global, ncols, npoints, ld4(omega), zs.data(), out8); return (int)kLagHdrWords;
}
int hc_lagrange_headers_agree(const uint64_t* all, size_t W, const uint64_t* mine) { return lag_headers_agree(all, W, mine) ? 1 : 0; }
// the column groups the driver launches for a pass of pass_points points of a block of n_local rows (lag_col_groups); *group_cols = the columns of a group
unsigned hc_lagrange_col_groups(int opt, size_t ncols, size_t n_local, size_t pass_points, size_t* group_cols) {
    const LagGeom G = lag_geom(n_local); unsigned cg = 1;
    const size_t per = lag_col_groups(opt, ncols, G.grid, lag_point_groups(pass_points, G.grid), &cg);
    if (group_cols) *group_cols = per;
    return cg;
}
}  // extern "C"

// ---- many Merkle trees in one pass (merkle_batch.hpp) through the host instantiation of the stream bodies -----------------------------------------
struct MerkleHostExec : HostArena {
    HcParams* p;
    explicit MerkleHostExec(HcParams* p_) : p(p_) {}
    int32_t level_block(size_t n_fr, fr_t** out) {                                   // a block that held something before: the fill of hc_set_alloc_fill, and never zeros
        if (hc_alloc_refused()) { *out = nullptr; return kHcOom; }
        mem.emplace_back(4 * n_fr + 1, g_alloc_fill ? 0x0101010101010101ull * (uint64_t)g_alloc_fill : 0xA5A5A5A5A5A5A5A5ull); *out = (fr_t*)mem.back().data(); return 0;
    }
    int32_t tables(const uint64_t* l, const fr_t* const* leaves, const fr_t* const* cp, size_t B, const uint64_t** lx, const fr_t* const** vx, const fr_t* const** cx) {
        uint64_t* dl = nullptr; const fr_t** dv = nullptr; const fr_t** dc = nullptr;
        if (int32_t rc = put(std::vector<uint64_t>(l, l + B), &dl)) return rc;
        if (int32_t rc = put(std::vector<const fr_t*>(leaves, leaves + B), &dv)) return rc;
        if (cp) if (int32_t rc = put(std::vector<const fr_t*>(cp, cp + B), &dc)) return rc;
        *lx = dl; *vx = dv; *cx = dc; return 0;
    }
    int32_t copy_rows(const fr_t* const* src, size_t n, size_t B, fr_t* dst) { for (size_t b = 0; b < B; ++b) for (size_t i = 0; i < n; ++i) dst[b * n + i] = src[b][i]; return 0; }
    template <class DS> int32_t hash_level(const DS& D, fr_t* out) { return hash_ds_stream(p, D, out); }
    // merkle_build_mixed_batch
    int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** x) { DsRaggedStream::Seg* d = nullptr; if (int32_t rc = put(h, &d)) return rc; *x = d; return 0; }
    int32_t copy_ragged(const DsRaggedStream& D, fr_t* dst) { for (size_t i = 0; i < D.n_out; ++i) { const DsRaggedStream::Seg& S = D.segs[D.seg(i)]; dst[i] = S.in0[i - S.first]; } return 0; }
};
struct MerkleOpenHostExec { int32_t gather(const MerkleGatherList& G, fr_t* out) { for (size_t i = 0; i < G.size(); ++i) out[G.row_of(i)] = G.base[G.src[i]][G.index[i]]; return 0; } };
static std::vector<size_t> total_lens(const std::vector<size_t>& lens, size_t B) { std::vector<size_t> o(lens.size() + 1, 0); for (size_t v = 0; v < lens.size(); ++v) o[v + 1] = o[v] + B * lens[v]; return o; }
extern "C" {
// MerkleTree::new / new_pairs of B trees of n leaves through the batch driver.  leaves / cp: B host columns (cp null iff !pairs; a null entry = zeros).
// out (cap_fr elements) receives the level blocks back to back: level v at element offset sum_{u<v} B lens[u], tree b's slice at b lens[v] inside it.
// Returns the number of levels (lens_out: their lengths, at most 64), or -1 on a refused shape.
int hc_merkle_build_batch(void* params, size_t arity, size_t B, const uint64_t* labels, const uint64_t* const* leaves, size_t n, int pairs, const uint64_t* const* cp,
                          uint64_t* out, size_t cap_fr, size_t* lens_out) {
    HcParams* P = (HcParams*)params;
    if (!B || !n || !arity || host::width_for_arity(arity) != P->dev.t || (arity == 1 && n > 1) || (pairs && !cp)) return -1;
    std::vector<std::vector<fr_t>> col(B, std::vector<fr_t>(n)), cc(B); std::vector<const fr_t*> lp(B), cpp(B, nullptr);
    for (size_t b = 0; b < B; ++b) {
        for (size_t i = 0; i < n; ++i) col[b][i] = ld4(leaves[b] + 4 * i);
        lp[b] = col[b].data();
        if (pairs && cp[b]) { cc[b].resize(n); for (size_t i = 0; i < n; ++i) cc[b][i] = ld4(cp[b] + 4 * i); cpp[b] = cc[b].data(); }
    }
    MerkleHostExec X(P); std::vector<size_t> lens; std::vector<fr_t*> base;
    if (int32_t rc = merkle_build_batch(X, arity, B, labels, lp.data(), n, pairs, pairs ? cpp.data() : nullptr, lens, base)) return hc_rc(rc);
    const std::vector<size_t> at = total_lens(lens, B);
    if (lens.size() > 64 || at.back() > cap_fr) return -1;
    for (size_t v = 0; v < lens.size(); ++v) { lens_out[v] = lens[v]; for (size_t i = 0; i < B * lens[v]; ++i) st4(out + 4 * (at[v] + i), base[v][i]); }
    return (int)lens.size();
}
// One launch of a DsRaggedStream (mode 0 node level / 1 pair leaf): segment s reads in0[s] (in1[s], pair leaves; a null table or entry = zeros), n_in[s]
// elements under labels[s]; out receives the segments' hashes back to back.  Returns the number of hashes, or -1 on an empty segment.
long hc_hash_ds_ragged_level(void* params, int mode, size_t arity, uint32_t level, uint64_t pos0, size_t n_seg, const uint64_t* labels, const uint64_t* const* in0,
                             const uint64_t* const* in1, const size_t* n_in, uint64_t* out) {
    HcParams* P = (HcParams*)params;
    std::vector<std::vector<fr_t>> a(n_seg), b(n_seg); DsRaggedTable T;
    for (size_t s = 0; s < n_seg; ++s) {
        if (!n_in[s]) return -1;
        a[s].resize(n_in[s]); for (size_t i = 0; i < n_in[s]; ++i) a[s][i] = ld4(in0[s] + 4 * i);
        if (mode == 1 && in1 && in1[s]) { b[s].resize(n_in[s]); for (size_t i = 0; i < n_in[s]; ++i) b[s][i] = ld4(in1[s] + 4 * i); }
        T.add(mode, arity, a[s].data(), b[s].empty() ? nullptr : b[s].data(), n_in[s], labels[s]);
    }
    hash_ds_stream(P, DsRaggedStream::make(mode, arity, level, pos0, T.segs.data(), n_seg, T.n_out), out);
    return (long)T.n_out;
}
// MerkleTree::new / new_pairs of B trees of n[b] leaves through the mixed-size driver.  out (cap_fr elements) receives the level blocks back to back,
// level v the slices of the trees with more than v levels in tree order.  nlev_out[b]: the levels of tree b, lens_out[64 b + v] their lengths.
// Returns the number of level blocks, or -1 on a refused shape.
int hc_merkle_build_mixed_batch(void* params, size_t arity, size_t B, const uint64_t* labels, const uint64_t* const* leaves, const size_t* n, int pairs, const uint64_t* const* cp,
                                uint64_t* out, size_t cap_fr, size_t* nlev_out, size_t* lens_out) {
    HcParams* P = (HcParams*)params;
    if (!B || !arity || host::width_for_arity(arity) != P->dev.t || (pairs && !cp)) return -1;
    for (size_t b = 0; b < B; ++b) if (!n[b] || !leaves[b] || (arity == 1 && n[b] > 1)) return -1;
    std::vector<std::vector<fr_t>> col(B), cc(B); std::vector<const fr_t*> lp(B), cpp(B, nullptr);
    for (size_t b = 0; b < B; ++b) {
        col[b].resize(n[b]); for (size_t i = 0; i < n[b]; ++i) col[b][i] = ld4(leaves[b] + 4 * i);
        lp[b] = col[b].data();
        if (pairs && cp[b]) { cc[b].resize(n[b]); for (size_t i = 0; i < n[b]; ++i) cc[b][i] = ld4(cp[b] + 4 * i); cpp[b] = cc[b].data(); }
    }
    MerkleHostExec X(P); std::vector<std::vector<size_t>> lens, at; std::vector<fr_t*> base;
    if (int32_t rc = merkle_build_mixed_batch(X, arity, B, labels, lp.data(), n, pairs, pairs ? cpp.data() : nullptr, lens, at, base)) return hc_rc(rc);
    std::vector<size_t> block(base.size(), 0);
    for (size_t b = 0; b < B; ++b) {
        if (lens[b].size() > 64) return -1;
        nlev_out[b] = lens[b].size();
        for (size_t v = 0; v < lens[b].size(); ++v) { lens_out[64 * b + v] = lens[b][v]; block[v] += lens[b][v]; }
    }
    size_t o = 0;
    for (size_t v = 0; v < base.size(); ++v) {
        if (o + block[v] > cap_fr) return -1;
        for (size_t i = 0; i < block[v]; ++i) st4(out + 4 * (o + i), base[v][i]);
        o += block[v];
    }
    return (int)base.size();
}
// open_union_of_paths of B trees through the batch driver.  Tree b: arity[b], nlev[b] levels; the levels of all trees are listed tree by tree in
// levels / lens.  Tree b opens idx[idx_off[b] .. idx_off[b + 1]).  The proofs are written back to back into buf when cap suffices, their lengths
// into out_lens; returns the total length, or -1 on refused arguments.
long hc_merkle_open_batch(size_t B, const size_t* arity, const size_t* nlev, const uint64_t* const* levels, const size_t* lens, const size_t* idx, const size_t* idx_off,
                          uint8_t* buf, size_t cap, size_t* out_lens) {
    std::vector<std::vector<std::vector<fr_t>>> lv(B); std::vector<std::vector<const fr_t*>> lp(B); std::vector<std::vector<size_t>> ll(B); std::vector<MerkleTreeView> views(B);
    for (size_t b = 0, q = 0; b < B; ++b) {
        for (size_t v = 0; v < nlev[b]; ++v, ++q) {
            lv[b].emplace_back(lens[q]); for (size_t i = 0; i < lens[q]; ++i) lv[b][v][i] = ld4(levels[q] + 4 * i);
            ll[b].push_back(lens[q]);
        }
        for (auto& l : lv[b]) lp[b].push_back(l.data());
        views[b] = MerkleTreeView{arity[b], &ll[b], lp[b].data()};
    }
    MerkleOpenHostExec X; std::vector<std::vector<uint8_t>> pr;
    if (merkle_open_batch(X, views.data(), B, idx, idx_off, pr)) return -1;
    size_t tot = 0; for (size_t b = 0; b < B; ++b) { out_lens[b] = pr[b].size(); tot += pr[b].size(); }
    if (buf && cap >= tot) { size_t o = 0; for (auto& p : pr) { memcpy(buf + o, p.data(), p.size()); o += p.size(); } }
    return (long)tot;
}
// verify_many_ds of `batch` openings through the batch planner, run step by step as the device runs it (max_slots: the pool slots of one plan;
// 0 = the library's 2^25); roots and values go to the driver as they come, at any 8-byte alignment.  accepted[i] = 1 / 0.  Returns 0, or -1 on an unsupported cfg_arity.
int hc_merkle_verify_batch(size_t cfg_arity, size_t batch, const uint64_t* labels, const uint64_t* roots, const size_t* indices, const size_t* idx_off, const uint64_t* values,
                           const uint8_t* const* proofs, const size_t* lens, size_t max_slots, int32_t* accepted) {
    if (host::width_for_arity(cfg_arity) < 0 || cfg_arity == 0) return -1;
    auto run = [](const VerifyBatchPlan& V, int32_t* acc) { run_plan_host(V, nullptr, acc); return 0; };
    return merkle_verify_batch(run, cfg_arity, batch, labels, roots, indices, idx_off, values, proofs, lens, max_slots ? max_slots : (size_t)1 << 25, accepted);
}
}  // extern "C"

// ---- the climbs of merkle_batch.hpp on their own: the ragged plan as data, and the launches of each call site -------------------------------------
extern "C" {
// merkle_ragged_plan of B trees of n[b] leaves.  Per tree: nlev[b], lens[64 b + v], at[64 b + v]; per level v < depth (at most 64): block[v], t0[v],
// n_seg[v], n_out[v]; per segment of the one table (at most cap written): first, n_in, label, tree.  *depth_out = depth; returns the number of
// segments, or -1 on refused arguments (no tree, an empty tree, arity 0 or arity 1 with more than one leaf) or a tree of more than 64 levels.
long hc_merkle_ragged_plan(size_t arity, size_t B, const size_t* n, const uint64_t* labels, int leaf_table, size_t* depth_out, size_t* nlev, size_t* lens, size_t* at,
                           size_t* block, size_t* t0, size_t* n_seg, size_t* n_out, uint64_t* seg_first, uint64_t* seg_n_in, uint64_t* seg_label, uint32_t* seg_tree, size_t cap) {
    if (!B || !arity) return -1;
    for (size_t b = 0; b < B; ++b) if (!n[b] || (arity == 1 && n[b] > 1)) return -1;
    const MerkleRaggedPlan P = merkle_ragged_plan(arity, B, n, labels, leaf_table != 0);
    if (P.depth > 64) return -1;
    *depth_out = P.depth;
    for (size_t b = 0; b < B; ++b) { nlev[b] = P.lens[b].size(); for (size_t v = 0; v < P.lens[b].size(); ++v) { lens[64 * b + v] = P.lens[b][v]; at[64 * b + v] = P.at[b][v]; } }
    for (size_t v = 0; v < P.depth; ++v) { block[v] = P.block[v]; t0[v] = P.t0[v]; n_seg[v] = P.n_seg[v]; n_out[v] = P.n_out[v]; }
    for (size_t s = 0; s < P.segs.size() && s < cap; ++s) { seg_first[s] = P.segs[s].first; seg_n_in[s] = P.segs[s].n_in; seg_label[s] = P.segs[s].label; seg_tree[s] = P.tree[s]; }
    return (long)P.segs.size();
}
// The DS launches of one call site of the climbs over zero-valued inputs of the given shapes, in launch order: out[4 i ..] = (stream kind: 1 DsBatchStream
// at a pitch, 2 behind a pointer table, 3 DsBatchPairStream, 4 DsRaggedStream node level, 5 pair leaves, 6 DsBatchPairPtrStream; DS level number; hashes; 1 when they go into
// the caller's top slots, else 0).  Returns their number (at most cap written), or -1 on a refused shape.
//   site 0  merkle_build_batch: B trees of n[0] leaves, flag = pairs                  site 1  merkle_build_mixed_batch: tree b of n[b] leaves, flag = pairs
//   site 2  FriBatchCommit::run: B traces of n[0] rows under schedule[0 .. L); the top slots are the (L + 1) x B roots
//   site 3  ScBatch::commit_layers: B layers of n[0] elements, flag = behind a pointer table; the top slots are B roots
//   site 4  ScBatch::commit_witnesses: witness b of n[b] = 2^k elements; the top slots are B roots
long hc_climb_launches(int site, size_t arity, size_t B, const size_t* n, int flag, const size_t* schedule, size_t L, int64_t* out, size_t cap) {
    if (!B || !arity) return -1;
    const size_t nb = site == 1 || site == 4 ? B : 1;
    for (size_t b = 0; b < nb; ++b) if (!n[b] || (arity == 1 && n[b] > 1)) return -1;
    std::vector<std::vector<fr_t>> col(B); std::vector<const fr_t*> cp(B); std::vector<uint64_t> labels(B); std::vector<size_t> k(B, 0);
    for (size_t b = 0; b < B; ++b) { const size_t nn = n[nb == 1 ? 0 : b]; col[b].assign(nn, fr_zero<PF>()); cp[b] = col[b].data(); labels[b] = 100 + b; while (((size_t)1 << k[b]) < nn) ++k[b]; }
    std::vector<HcLaunch> log; const fr_t* top = nullptr; size_t n_top = 0; int32_t rc = 0;
    struct Open { Open(std::vector<HcLaunch>* l) { g_launch_log = l; } ~Open() { g_launch_log = nullptr; } };
    // the executors (and with them the top slots) live until the log is classified
    HcParams* P = hc_param_cache().params(site >= 3 ? 16 : arity);
    MerkleHostExec XM(P); FriHostExec XF(P); FriBatchCommit<FriHostExec> C(XF); ScHostExec XS(P, P); ScBatch<ScHostExec> S(XS, B, cp.data(), k.data(), labels.data());
    if (site == 0) {
        std::vector<size_t> lens; std::vector<fr_t*> base; Open o(&log);
        rc = merkle_build_batch(XM, arity, B, labels.data(), cp.data(), n[0], flag, flag ? cp.data() : nullptr, lens, base);
    } else if (site == 1) {
        std::vector<std::vector<size_t>> lens, at; std::vector<fr_t*> base; Open o(&log);
        rc = merkle_build_mixed_batch(XM, arity, B, labels.data(), cp.data(), n, flag, flag ? cp.data() : nullptr, lens, at, base);
    } else if (site == 2) {
        std::string err; if (C.shape(B, n[0], schedule, L, err)) return -1;
        const std::vector<fr_t> z(L, host::h_u64(3)); if (C.init(z.data())) return -1;
        for (size_t i = 0; i < B * n[0]; ++i) C.f[0][i] = fr_zero<PF>();
        Open o(&log); rc = C.run(); top = C.roots; n_top = (L + 1) * B;
    } else if (site == 3 || site == 4) {
        if (site == 4) for (size_t b = 0; b < B; ++b) if (n[b] != (size_t)1 << k[b]) return -1;
        if (S.setup()) return -1;
        fr_t* roots = nullptr; if (S.alloc_fr(B, &roots)) return -1;
        std::vector<ScBatch<ScHostExec>::Tree> T; Open o(&log);
        if (site == 4) rc = S.commit_witnesses(roots, T);
        else if (flag) rc = S.commit_layers(S.wit_x, S.wit_s.data(), nullptr, n[0], B, roots, T);
        else { fr_t* layers = nullptr; if (S.alloc_fr(B * n[0], &layers)) return -1; for (size_t i = 0; i < B * n[0]; ++i) layers[i] = fr_zero<PF>(); rc = S.commit_layers(nullptr, nullptr, layers, n[0], B, roots, T); }
        top = roots; n_top = B;
    } else return -1;
    if (rc) return -1;
    for (size_t i = 0; i < log.size() && i < cap; ++i) {
        out[4 * i] = log[i].kind; out[4 * i + 1] = log[i].level; out[4 * i + 2] = (int64_t)log[i].n_out; out[4 * i + 3] = top && log[i].out >= top && log[i].out < top + n_top ? 1 : 0;
    }
    return (long)log.size();
}
}  // extern "C"

// ---- the ragged commit phase (fri_mixed.hpp) through the host instantiation of the stream bodies -------------------------------------------------------
// FriHostExec plus the ragged steps, counting what the driver asks for by kind (the census of hc_fri_commit_mixed_steps).  dry: count only — nothing is
// folded or hashed (what the driver launches depends on the shapes alone).
struct FriMixedHostExec : FriHostExec {
    bool dry = false; size_t n_fold = 0, n_leaf_pairs = 0, n_pair_streams = 0, n_levels = 0, n_blocks = 0, n_zpows = 0, n_gathers = 0;
    using FriHostExec::FriHostExec;
    int32_t alloc(size_t bytes, void** out) { ++n_blocks; return HostArena::alloc(bytes, out); }
    template <class T> int32_t put(const std::vector<T>& h, T** out) { ++n_blocks; return HostArena::put(h, out); }
    int32_t zpows_many(const ZpowJob* jobs, size_t n_jobs, size_t, fr_t* zp) {
        ++n_zpows; if (dry) return 0;
        for (size_t s = 0; s < n_jobs; ++s) FriHostExec::zpows(jobs[s].z, jobs[s].m, zp + jobs[s].off);
        return 0;
    }
    int32_t fold(const fr_t* f, size_t n, const fr_t* zp, size_t m, fr_t* out) { ++n_fold; return dry ? 0 : FriHostExec::fold(f, n, zp, m, out); }
    int32_t fold_ragged(const fr_t* f, size_t n, const FoldSeg* segs, size_t n_seg, const fr_t* zp, size_t m, fr_t* out) { ++n_fold; if (!dry) fri_fold_ragged_host(f, n, segs, n_seg, zp, m, out); return 0; }
    int32_t leaf_pairs(const fr_t* f, const fr_t* f_next, size_t n, size_t m, fr_t* h) { ++n_leaf_pairs; return dry ? 0 : FriHostExec::leaf_pairs(f, f_next, n, m, h); }
    int32_t hash_level(size_t arity, const DsRaggedPairStream& D, fr_t* out) { ++n_pair_streams; return dry ? 0 : hash_ds_stream(mp.params(arity), D, out); }
    int32_t hash_level(size_t arity, const DsRaggedStream& D, fr_t* out) { ++n_levels; return dry ? 0 : hash_ds_stream(mp.params(arity), D, out); }
    int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** x) { DsRaggedStream::Seg* d = nullptr; if (int32_t rc = put(h, &d)) return rc; *x = d; return 0; }
    int32_t gather(const MerkleGatherList& G, fr_t* out) { ++n_gathers; if (!dry) for (size_t i = 0; i < G.size(); ++i) out[G.row_of(i)] = G.base[G.src[i]][G.index[i]]; return 0; }
};
extern "C" {
// The commit phase of B traces of one schedule and any n0[b] through FriMixedCommit: roots[(b (L + 1) + l) * 4 ..] = root of layer l of trace b.  All
// "FRI/z/l" hashes of the pass are one hash call.  0 on success, the driver's refusal (-1, -2, -3) or the out-of-memory code otherwise.
int hc_fri_commit_mixed(void* tparams, size_t B, const uint64_t* const* f0, const size_t* n0, const size_t* schedule, size_t L, uint64_t seed_z, uint64_t* roots) {
    FriMixedHostExec X((HcParams*)tparams); FriMixedCommit<FriMixedHostExec> C(X);
    std::string err; if (int rc = C.shape(B, n0, schedule, L, err)) return rc;
    const size_t K = C.zkeys.size(); std::vector<fr_t> in(3 * K), fused(K), z(K);
    for (size_t k = 0; k < K; ++k) { in[3 * k] = host::h_u64(seed_z); in[3 * k + 1] = host::h_u64(C.zkeys[k].l); in[3 * k + 2] = host::h_u64(C.zkeys[k].n); }
    HcHasher H(tparams); if (K && H.hash("FRI/z/l", in.data(), 3, K, fused.data())) return -4;
    for (size_t k = 0; k < K; ++k) z[k] = fri_z_from_fused(fused[k], seed_z, C.zkeys[k].l, C.zkeys[k].n);
    if (int32_t rc = C.init(z.data())) return hc_rc(rc);
    for (size_t b = 0; b < B; ++b) for (size_t i = 0; i < n0[b]; ++i) C.f[0][C.at[0][b] + i] = ld4(f0[b] + 4 * i);
    if (int32_t rc = C.run()) return hc_rc(rc);
    for (size_t i = 0; i < B * (L + 1); ++i) st4(roots + 4 * i, C.roots[i]);
    return 0;
}
// The driver's census over shapes alone: out7 = (folds, leaf-pair launches, pair-stream launches, level launches, blocks, z-power launches, gathers).
int hc_fri_commit_mixed_steps(size_t B, const size_t* n0, const size_t* schedule, size_t L, size_t* out7) {
    FriMixedHostExec X(nullptr); X.dry = true; FriMixedCommit<FriMixedHostExec> C(X);
    std::string err; if (int rc = C.shape(B, n0, schedule, L, err)) return rc;
    const std::vector<fr_t> z(C.zkeys.size(), host::h_u64(3));
    if (int32_t rc = C.init(z.data())) return hc_rc(rc);
    if (int32_t rc = C.run()) return hc_rc(rc);
    out7[0] = X.n_fold; out7[1] = X.n_leaf_pairs; out7[2] = X.n_pair_streams; out7[3] = X.n_levels; out7[4] = X.n_blocks; out7[5] = X.n_zpows; out7[6] = X.n_gathers;
    return 0;
}
// One launch of a DsRaggedPairStream: segment s reads in0[s] (n_in[s] elements) under labels[s]; in1 (n_in1 elements, or null: zero partners) is the ONE
// partner array of the launch, read at (hash index) / cp_div.  out receives the segments' hashes back to back.  Returns their number, or -1 on an empty
// segment or a partner index out of range.
long hc_hash_ds_ragged_pairs_level(void* params, size_t arity, size_t n_seg, const uint64_t* labels, const uint64_t* const* in0, const size_t* n_in, const uint64_t* in1, size_t n_in1,
                                   size_t cp_div, uint64_t* out) {
    HcParams* P = (HcParams*)params;
    std::vector<std::vector<fr_t>> a(n_seg); std::vector<fr_t> b(in1 ? n_in1 : 0); DsRaggedTable T;
    for (size_t s = 0; s < n_seg; ++s) {
        if (!n_in[s]) return -1;
        a[s].resize(n_in[s]); for (size_t i = 0; i < n_in[s]; ++i) a[s][i] = ld4(in0[s] + 4 * i);
        T.add(1, arity, a[s].data(), nullptr, n_in[s], labels[s]);
    }
    for (size_t i = 0; i < b.size(); ++i) b[i] = ld4(in1 + 4 * i);
    if (!cp_div || (in1 && T.n_out && (T.n_out - 1) / cp_div >= n_in1)) return -1;
    hash_ds_stream(P, DsRaggedPairStream::make(arity, T.segs.data(), n_seg, T.n_out, in1 ? b.data() : nullptr, cp_div), out);
    return (long)T.n_out;
}
// The ragged fold's host restatement (fri_fold_ragged_host): n inputs, runs (first_out[s], zp_off[s]) over a table of n_zp elements.  -1: refused arguments.
int hc_fri_fold_ragged(const uint64_t* f, size_t n, const uint64_t* first_out, const uint64_t* zp_off, size_t n_seg, const uint64_t* zp, size_t n_zp, size_t m, uint64_t* out) {
    if (m < 2 || n % m || !n_seg || first_out[0] != 0) return -1;
    std::vector<FoldSeg> segs(n_seg);
    for (size_t s = 0; s < n_seg; ++s) { if ((s && first_out[s] <= first_out[s - 1]) || zp_off[s] + m > n_zp) return -1; segs[s] = FoldSeg{first_out[s], zp_off[s]}; }
    std::vector<fr_t> fv(n), zv(n_zp), o(n / m);
    for (size_t i = 0; i < n; ++i) fv[i] = ld4(f + 4 * i);
    for (size_t i = 0; i < n_zp; ++i) zv[i] = ld4(zp + 4 * i);
    fri_fold_ragged_host(fv.data(), n, segs.data(), n_seg, zv.data(), m, o.data());
    for (size_t i = 0; i < o.size(); ++i) st4(out + 4 * i, o[i]);
    return 0;
}
// mixed_prove_classes (fri_plan.hpp): class_of[i] = the class of trace i, order = the traces class by class; returns the number of classes
size_t hc_mixed_prove_classes(size_t B, const size_t* schedule, const size_t* sched_off, size_t* class_of, size_t* order) {
    const std::vector<std::vector<size_t>> G = mixed_prove_classes(B, schedule, sched_off);
    size_t pos = 0;
    for (size_t g = 0; g < G.size(); ++g) for (size_t i : G[g]) { class_of[i] = g; order[pos++] = i; }
    return G.size();
}
// mixed_prove_passes (fri_plan.hpp): the traces per pass into out[0 .. cap); returns the number of passes
size_t hc_mixed_prove_passes(size_t B, const size_t* n0, size_t max_rows, size_t max_traces, size_t* out, size_t cap) {
    const std::vector<size_t> p = mixed_prove_passes(B, n0, max_rows, max_traces);
    for (size_t i = 0; i < p.size() && i < cap; ++i) out[i] = p[i];
    return p.size();
}
}  // extern "C"
