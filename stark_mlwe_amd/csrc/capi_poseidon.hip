// stark_mlwe_amd/csrc/capi_poseidon.hip — the Poseidon kernels, the selector of their forms and every launcher of them (poseidon_launch.hpp);
// the Poseidon, leaf-hash, tr_hash and Merkle entry points of the C-ABI (include/stark_mlwe.h).  The only translation unit that includes the
// kernel headers: each Poseidon kernel is in one code object of the library.  No CPU compute fallback anywhere in this file: every bulk
// operation is a kernel launch.
#include <algorithm>
#include <cstring>
#include <type_traits>
#include "poseidon_launch.hpp"
#include "poseidon_dev.hpp"
#include "poseidon_pair.hpp"
#include "poseidon_coop.hpp"
#include "poseidon_chain.hpp"
#include "poseidon_wave.hpp"
#include "poseidon_transcript.hpp"
#include "fri_dev.hpp"
#include "merkle_batch.hpp"

using namespace stark;

static const size_t kMaxLds = 160 * 1024;
static inline int poseidon_block(int t) { return (size_t)t * 32 * 64 <= kMaxLds ? 64 : 32; }
static inline size_t poseidon_lds(int t, int block) { return (size_t)t * 32 * block; }
// ---- which kernel form runs a Poseidon operation of n sponges ---------------------------------------------------------------------------------
//   Lane      one lane per sponge, state in LDS (poseidon_dev.hpp): any width; the option "poseidon_lane_only" forces it (diagnostic)
//   WavePair  two waves per 64 sponges (poseidon_pair.hpp): the throughput form of the hot widths t = 9, 17
//   OneWave   one wave per sponge (poseidon_coop.hpp): few or long sponges, t = 9, 17
//   FiveWave  five waves per sponge (poseidon_chain.hpp), one workgroup resident per CU: the latency form, t = 17 with the chain tables
//   Wide      one wave per sponge for t = 33, 65, 129 (poseidon_wave.hpp)
// Small batches of t = 17 sponges take the five-wave form: Merkle levels of up to 256 nodes (two permutations: 155 us against 290 us on one wave each;
// equal from 512 nodes on), leaf layers of up to 2048 leaves (one permutation: 80 us per 256 leaves against the 0.77 ms a launch of the wave-pair
// throughput kernel takes whatever its size), transcript hashes of up to 512 sponges (up to two resident workgroups per CU; 72 us per permutation
// against 142 us on one wave).  Above that one wave per node / leaf / sponge up to 4096, then the wave pair (Merkle levels, leaf layers) or a lane per
// sponge (transcript hashes).  The Merkle and leaf crossovers were measured by tools/latency_timing.py; the option "sponge_one_wave" keeps the small
// batches on the one-wave / wave-pair kernels (comparison).
// The mapping is kept exactly as measured, including where operations differ: under "sponge_one_wave" a Merkle level of <= 4096 nodes runs one wave per
// node but a leaf layer of <= 4096 leaves the wave pair, and the column sponges ignore "poseidon_lane_only".
// RaggedSponges (stark_tr_hash_many_dev: items of any tag and length in one launch) selects as the column sponges do, whatever the count — a
// ragged launch is for chains — except that it honours "poseidon_lane_only", so that the lane form of the layout can be run.
enum class PoseidonForm { Lane, WavePair, OneWave, FiveWave, Wide };
enum class PoseidonOp { MerkleLevel, LeafLayer, TrHash, ColumnSponges, RaggedSponges, DeviceTranscript };
constexpr size_t kChainMaxNodes = 256, kChainMaxLeaves = 2048, kChainMaxSponges = 512, kCoopMaxNodes = 4096, kCoopMaxLeaves = 4096, kCoopMaxSponges = 4096;
static PoseidonForm poseidon_form(const stark_ctx* ctx, const stark_params* p, PoseidonOp op, size_t n) {
    const PoseidonDev& d = p->dev;
    const bool lane_only = ctx->opt.poseidon_lane_only, one_wave = ctx->opt.sponge_one_wave;
    const bool chain = !lane_only && !one_wave && d.t == 17 && d.rf == 8 && d.rp == 64 && d.chain_a;
    switch (op) {
    case PoseidonOp::MerkleLevel:
        if ((ctx->side_commit || ctx->opt.merkle_wave_pair) && !lane_only && (d.t == 9 || d.t == 17)) return PoseidonForm::WavePair;
        if (chain && n <= kChainMaxNodes) return PoseidonForm::FiveWave;
        if (!lane_only && (d.t == 9 || d.t == 17)) return n <= kCoopMaxNodes ? PoseidonForm::OneWave : PoseidonForm::WavePair;
        if (!lane_only && (d.t == 33 || d.t == 65 || d.t == 129) && n <= 0x7fffffffu) return PoseidonForm::Wide;     // one block per node
        return PoseidonForm::Lane;
    case PoseidonOp::LeafLayer:
        if (ctx->side_commit && !lane_only) return PoseidonForm::WavePair;
        if (chain && n <= kChainMaxLeaves) return PoseidonForm::FiveWave;
        if (!lane_only && !one_wave && n <= kCoopMaxLeaves) return PoseidonForm::OneWave;
        return lane_only ? PoseidonForm::Lane : PoseidonForm::WavePair;
    case PoseidonOp::TrHash:
        if (chain && n <= kChainMaxSponges) return PoseidonForm::FiveWave;
        return !lane_only && n <= kCoopMaxSponges ? PoseidonForm::OneWave : PoseidonForm::Lane;
    case PoseidonOp::RaggedSponges:
        if (lane_only) return PoseidonForm::Lane;
        [[fallthrough]];
    case PoseidonOp::ColumnSponges:
        return d.chain_a && !one_wave ? PoseidonForm::FiveWave : PoseidonForm::OneWave;
    case PoseidonOp::DeviceTranscript:                                  // n instances advanced by one launch; up to two resident five-wave workgroups per CU, as for TrHash
        return chain && n <= kChainMaxSponges ? PoseidonForm::FiveWave : PoseidonForm::OneWave;
    }
    return PoseidonForm::Lane;
}
static inline row::Consts row_consts_of(const stark_ctx* ctx) {
    const RowConstsHost h = row_consts_host(); row::Consts RK; for (int i = 0; i < 9; ++i) RK.ni[i] = h.ni[i]; for (int i = 0; i < 5; ++i) RK.t[i] = h.t[i]; RK.dbg = (uint32_t)ctx->opt.sponge_debug; return RK;
}

// the leaf constants of hash_leaf_pair (fri.rs:38-44) on the device: the template and round 0 in closed form (LeafConsts)
static int32_t ctx_leaf_init(stark_ctx* ctx, const LeafConsts** out) {
    if (!ctx->leaf_init) {
        stark_params* tp = nullptr; STARK_TRY(ctx_transcript_params(ctx, &tp));
        LeafConsts lc; host::leaf_consts(tp->ref, lc);
        DevMem d; STARK_TRY(d.fill_sync(ctx, &lc, sizeof lc));
        ctx->leaf_init = std::move(d);
    }
    *out = ctx->leaf_init.as<LeafConsts>(); return STARK_OK;
}

namespace stark {

// The device copy of host::tr_hash_frame(tag), cached per tag: frame = prefix || suffix, np + ns elements.
static int32_t tr_frame(stark_ctx* ctx, const char* tag, fr_t** dev, int* np, int* ns) {
    const std::string key(tag);
    auto it = ctx->tr_frames.find(key);
    if (it == ctx->tr_frames.end()) {
        std::vector<fr_t> fr; const int p = host::tr_hash_frame(tag, fr);
        DevMem d; STARK_TRY(d.fill_sync(ctx, fr.data(), fr.size() * sizeof(fr_t)));
        it = ctx->tr_frames.emplace(key, std::move(d)).first; ctx->tr_frame_dims[key] = {p, (int)fr.size() - p};
    }
    *dev = it->second.fr(); *np = ctx->tr_frame_dims[key].first; *ns = ctx->tr_frame_dims[key].second; return STARK_OK;
}
static int32_t launch_tr_hash(stark_ctx* ctx, stark_params* tp, PoseidonForm form, const TrStream& T, fr_t* out_dev) {
    const bool ragged = T.layout == TrStream::Ragged;
    switch (form) {
    case PoseidonForm::FiveWave:
        if (ragged) hipLaunchKernelGGL(k_tr_hash_chain_ragged, dim3((unsigned)T.n), dim3(320), chain_lds_bytes(), ctx->stream, tp->dev, T, row_consts_of(ctx), out_dev);
        else hipLaunchKernelGGL(k_tr_hash_chain, dim3((unsigned)T.n), dim3(320), chain_lds_bytes(), ctx->stream, tp->dev, T, row_consts_of(ctx), out_dev);
        break;
    case PoseidonForm::OneWave:
        if (ragged) hipLaunchKernelGGL((k_tr_hash_coop<true, true>), dim3((unsigned)T.n), dim3(64), coop_lds_bytes(17), ctx->stream, tp->dev, T, out_dev);
        else if (T.layout == TrStream::Equal) hipLaunchKernelGGL(k_tr_hash_coop<false>, dim3((unsigned)T.n), dim3(64), coop_lds_bytes(17), ctx->stream, tp->dev, T, out_dev);
        else hipLaunchKernelGGL(k_tr_hash_coop<true>, dim3((unsigned)T.n), dim3(64), coop_lds_bytes(17), ctx->stream, tp->dev, T, out_dev);
        break;
    default: {
        const int block = 64;
        if (ragged) hipLaunchKernelGGL(k_tr_hash_ragged, dim3((unsigned)((T.n + block - 1) / block)), dim3(block), poseidon_lds(17, block), ctx->stream, tp->dev, T, out_dev);
        else hipLaunchKernelGGL(k_tr_hash, dim3((unsigned)((T.n + block - 1) / block)), dim3(block), poseidon_lds(17, block), ctx->stream, tp->dev, T, out_dev);
    } }
    STARK_HIP(ctx, hipGetLastError());
    return STARK_OK;
}
int32_t tr_hash_dev(stark_ctx* ctx, const char* tag, const fr_t* fields_dev, size_t k, size_t n, fr_t* out_dev) {
    stark_params* tp = nullptr; STARK_TRY(ctx_transcript_params(ctx, &tp));
    fr_t* frame = nullptr; int np = 0, ns = 0; STARK_TRY(tr_frame(ctx, tag, &frame, &np, &ns));
    if (n == 0) return STARK_OK;
    const TrStream T = TrStream::equal(frame, np, ns, fields_dev, k, n, host::h_tag("FSv1-TRANSCRIPT-INIT"));
    return launch_tr_hash(ctx, tp, poseidon_form(ctx, tp, PoseidonOp::TrHash, n), T, out_dev);
}
// The serial column sponges of DeepAliRealBuilder::build_f0 (fri.rs:551-554), one block each: the four columns of one trace (ptrs_dev == nullptr) or
// of B independent traces (ptrs_dev[4 * p + c] = column c of trace p, a device array of device pointers).
static int32_t tr_hash_columns(stark_ctx* ctx, const char* const tags[4], const fr_t* const cols[4], const fr_t* const* ptrs_dev, size_t nblocks, size_t n0, fr_t* out_dev) {
    stark_params* tp = nullptr; STARK_TRY(ctx_transcript_params(ctx, &tp));
    TrStream T{}; T.layout = ptrs_dev ? TrStream::BatchColumns : TrStream::Columns; T.n = nblocks; T.batch = ptrs_dev; T.cap = host::h_tag("FSv1-TRANSCRIPT-INIT");
    for (int c = 0; c < 4; ++c) {
        fr_t* frame = nullptr; int np = 0, ns = 0; STARK_TRY(tr_frame(ctx, tags[c], &frame, &np, &ns));
        T.prefix[c] = frame; T.np[c] = np; T.suffix[c] = frame + np; T.ns[c] = ns; T.fields[c] = cols ? cols[c] : nullptr; T.k[c] = n0;
    }
    return launch_tr_hash(ctx, tp, poseidon_form(ctx, tp, PoseidonOp::ColumnSponges, nblocks), T, out_dev);
}
int32_t tr_hash_columns4_dev(stark_ctx* ctx, const char* const tags[4], const fr_t* const cols[4], size_t n0, fr_t* out4_dev) {
    return tr_hash_columns(ctx, tags, cols, nullptr, 4, n0, out4_dev);
}
int32_t tr_hash_columns_batch_dev(stark_ctx* ctx, const char* const tags[4], const fr_t* const* ptrs_dev, size_t batch, size_t n0, fr_t* out_dev) {
    return tr_hash_columns(ctx, tags, nullptr, ptrs_dev, 4 * batch, n0, out_dev);
}
// n sponges of any tags and lengths in ONE launch (the Ragged layout of TrStream): out_dev[i] = tr_hash_fields_tagged(tags[i], fields[i][0 .. k[i])),
// fields a host table of device pointers (an entry with k[i] == 0 is not read and may be null).  The frames come from the per-tag cache (the first
// use of a tag uploads its frame and synchronises, as everywhere); the items go up staged, so nothing else synchronises.  column_sponges: select the
// kernel form as the column sponges of build_f0 do (the mixed-size prover); otherwise as PoseidonOp::RaggedSponges.
int32_t tr_hash_many_dev(stark_ctx* ctx, size_t n, const char* const* tags, const fr_t* const* fields, const size_t* k, fr_t* out_dev, bool column_sponges) {
    stark_params* tp = nullptr; STARK_TRY(ctx_transcript_params(ctx, &tp));
    std::vector<TrFrameRef> fr(n);
    for (size_t i = 0; i < n; ++i) { fr_t* frame = nullptr; STARK_TRY(tr_frame(ctx, tags[i], &frame, &fr[i].np, &fr[i].ns)); fr[i].frame = frame; }
    if (n == 0) return STARK_OK;
    if (n > 0x7fffffffu) return ctx->fail(STARK_ERR_UNSUPPORTED, "tr_hash_many: more than 2^31 - 1 items in one call");
    const std::vector<TrStream::Item> items = tr_ragged_items(fr.data(), fields, k, n);
    DevBuf d; STARK_HIP(ctx, d.alloc(ctx, n * sizeof(TrStream::Item))); STARK_TRY(ctx_upload_staged(ctx, d.p, items.data(), n * sizeof(TrStream::Item)));
    const TrStream T = tr_ragged_stream((const TrStream::Item*)d.p, n, host::h_tag("FSv1-TRANSCRIPT-INIT"));
    return launch_tr_hash(ctx, tp, poseidon_form(ctx, tp, column_sponges ? PoseidonOp::ColumnSponges : PoseidonOp::RaggedSponges, n), T, out_dev);
}
int32_t tr_hash_host1(stark_ctx* ctx, const char* tag, const std::vector<fr_t>& fields, fr_t* out) {
    DevBuf in, o; STARK_HIP(ctx, in.alloc(ctx, fields.size() * sizeof(fr_t))); STARK_HIP(ctx, o.alloc(ctx, sizeof(fr_t)));
    STARK_TRY(ctx_upload_staged(ctx, in.p, fields.data(), fields.size() * sizeof(fr_t)));
    STARK_TRY(tr_hash_dev(ctx, tag, in.fr(), fields.size(), 1, o.fr()));
    STARK_HIP(ctx, o.download_sync(out, sizeof(fr_t)));
    return STARK_OK;
}
// The streaming transcripts (poseidon_transcript.hpp): one instance, or the active instances of a batch, on five waves or on one
int32_t tr_stream_on(stark_ctx* ctx, stark_params* tp, fr_t* state, uint32_t* pos, const fr_t* fields, size_t n, bool finish, fr_t* out) {
    if (poseidon_form(ctx, tp, PoseidonOp::DeviceTranscript, 1) == PoseidonForm::FiveWave)
        hipLaunchKernelGGL(k_tr_stream_chain, dim3(1), dim3(320), chain_lds_bytes(), ctx->stream, tp->dev, row_consts_of(ctx), state, pos, fields, (uint64_t)n, finish ? 1 : 0, finish ? out : (fr_t*)nullptr);
    else
        hipLaunchKernelGGL(k_tr_stream, dim3(1), dim3(64), coop_lds_bytes(17), ctx->stream, tp->dev, state, pos, fields, (uint64_t)n, finish ? 1 : 0, finish ? out : (fr_t*)nullptr);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
int32_t tr_batch_on(stark_ctx* ctx, stark_params* tp, const TrBatchStream& T, size_t n_for_form) {
    if (!T.n_active) return STARK_OK;
    if (poseidon_form(ctx, tp, PoseidonOp::DeviceTranscript, n_for_form) == PoseidonForm::FiveWave)
        for (uint32_t sg = 0; sg < (uint32_t)T.nseg; ++sg)
            hipLaunchKernelGGL(k_tr_batch_chain, dim3((unsigned)T.n_active), dim3(320), chain_lds_bytes(), ctx->stream, tp->dev, row_consts_of(ctx), T, sg);
    else
        hipLaunchKernelGGL(k_tr_batch, dim3((unsigned)T.n_active), dim3(64), coop_lds_bytes(17), ctx->stream, tp->dev, T);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}

}  // namespace stark

extern "C" {

// ---- Poseidon ----------------------------------------------------------------------------------------
int32_t stark_poseidon_permute_batch_dev(stark_ctx_t* ctx, stark_params_t* p, uint64_t* states, size_t n) {
    if (!ctx || !p || (!states && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (!n) return STARK_OK;
    const int block = poseidon_block(p->dev.t);
    hipLaunchKernelGGL(k_permute_batch, dim3((unsigned)((n + block - 1) / block)), dim3(block), poseidon_lds(p->dev.t, block), ctx->stream, p->dev, as_fr(states), n);
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
int32_t stark_poseidon_permute_batch(stark_ctx_t* ctx, stark_params_t* p, uint64_t* states, size_t n) {
    if (!ctx || !p || (!states && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    size_t bytes = n * p->dev.t * sizeof(fr_t); DevBuf d; CallerUploads up(ctx); STARK_HIP(ctx, up.up(d, states, bytes));
    STARK_TRY(stark_poseidon_permute_batch_dev(ctx, p, (uint64_t*)d.p, n));
    STARK_HIP(ctx, up.download_sync(states, d.p, bytes));
    return STARK_OK;
}
static int32_t hash_stream(stark_ctx_t* ctx, stark_params_t* p, int mode, const uint64_t* a, size_t na, const uint64_t* b, size_t nb, const fr_t& tag, size_t n, uint64_t* out) {
    DevBuf da, db, dout; CallerUploads up(ctx);
    STARK_HIP(ctx, up.up(da, a, n * na * sizeof(fr_t))); STARK_HIP(ctx, up.up(db, b, n * nb * sizeof(fr_t))); STARK_HIP(ctx, dout.alloc(ctx, n * sizeof(fr_t)));
    const int block = poseidon_block(p->dev.t);
    hipLaunchKernelGGL(k_hash_stream, dim3((unsigned)((n + block - 1) / block)), dim3(block), poseidon_lds(p->dev.t, block), ctx->stream, p->dev, mode, da.fr(), na, db.fr(), nb, tag, n, dout.fr());
    STARK_HIP(ctx, hipGetLastError());
    STARK_HIP(ctx, up.download_sync(out, dout.p, n * sizeof(fr_t)));
    return STARK_OK;
}
int32_t stark_poseidon_hash_with_ds_dynamic(stark_ctx_t* ctx, stark_params_t* p, const uint64_t* ds, size_t nds, const uint64_t* in, size_t cnt, size_t n, uint64_t* out) {
    if (!ctx || !p || !out || (!ds && nds) || (!in && cnt)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (!n) return STARK_OK;
    return hash_stream(ctx, p, 0, ds, nds, in, cnt, host::h_zero(), n, out);
}
int32_t stark_poseidon_hash_with_ds(stark_ctx_t* ctx, stark_params_t* p, const uint64_t* in, size_t cnt, const uint64_t* ds_tag, uint64_t* out) {
    if (!ctx || !p || !out || !ds_tag || (!in && cnt)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (p->dev.t != 17) return ctx->fail(STARK_ERR_INVALID_ARG, "hash_with_ds is the fixed t=17 sponge");
    return hash_stream(ctx, p, 1, nullptr, 0, in, cnt, load_fr(ds_tag), 1, out);
}
}  // extern "C"
// The 8-round partial blocks of the t = 17 wave-pair kernels: option poseidon_block8 (default 1) and a parameter set with rp % 8 == 0.  Such a set
// without its tables on the device is an error, never a quiet return to blocks of 4.
static int32_t pair_block8_form(stark_ctx* ctx, const stark_params* p, bool* on) {
    *on = ctx->opt.poseidon_block8 && p->dev.t == 17 && p->dev.rp % 8 == 0 && p->dev.rf >= 2;      // rf >= 2: the fused kernels enter the blocks from the product of round rf / 2 - 1
    if (*on && (!p->dev.blk8_efrag || !p->dev.blk8_lfrag || !p->dev.blk8_unit_frag || !p->dev.blk8_gfrag || !p->dev.rc_partial_scaled29)) return ctx->fail(STARK_ERR_UNSUPPORTED, "poseidon_block8: the parameter set has no block-8 tables");
    return STARK_OK;
}
// One launch of hash_with_ds_dynamic over the hashes of a DS stream (hash_ds_on), in the form poseidon_form picks for a Merkle level of that many nodes.
template <class DS>
static int32_t launch_ds(stark_ctx_t* ctx, hipStream_t st, stark_params_t* p, const DS& D, fr_t* out) {
    if (!D.n_out) return STARK_OK;
    const int t = p->dev.t; const unsigned nodes = (unsigned)D.n_out, pairs = (unsigned)((D.n_out + 63) / 64);
    bool b8 = false; STARK_TRY(pair_block8_form(ctx, p, &b8));
    switch (poseidon_form(ctx, p, PoseidonOp::MerkleLevel, D.n_out)) {
    case PoseidonForm::FiveWave: hipLaunchKernelGGL(k_hash_ds_chain<DS>, dim3(nodes), dim3(320), chain_lds_bytes(), st, p->dev, D, row_consts_of(ctx), out); break;
    case PoseidonForm::OneWave:
        if (t == 17) hipLaunchKernelGGL((k_hash_ds_coop<17, DS>), dim3(nodes), dim3(64), coop_lds_bytes(17), st, p->dev, D, out);
        else hipLaunchKernelGGL((k_hash_ds_coop<9, DS>), dim3(nodes), dim3(64), coop_lds_bytes(9), st, p->dev, D, out);
        break;
    case PoseidonForm::WavePair:
        if constexpr (std::is_same<DS, DsStream>::value) {
            // a node level whose every node has 16 children (no ragged last node): the fixed two-permutation kernel
            if (t == 17 && ctx->opt.merkle_node16_pair && D.mode == 0 && D.arity == 16 && D.n_in == 16 * D.n_out) {
                if (b8) hipLaunchKernelGGL(k_node16_pair<true>, dim3(pairs), dim3(128), pair_lds_bytes(17), st, p->dev, D.arity_f, D.level_f, D.label_f, D.pos0, D.in0, D.n_out, out);
                else hipLaunchKernelGGL(k_node16_pair<false>, dim3(pairs), dim3(128), pair_lds_bytes(17), st, p->dev, D.arity_f, D.level_f, D.label_f, D.pos0, D.in0, D.n_out, out);
                break;
            }
        }
        if (t == 17 && b8) hipLaunchKernelGGL((k_hash_ds2<17, DS, true>), dim3(pairs), dim3(128), pair_lds_bytes(17), st, p->dev, D, out);
        else if (t == 17) hipLaunchKernelGGL((k_hash_ds2<17, DS>), dim3(pairs), dim3(128), pair_lds_bytes(17), st, p->dev, D, out);
        else hipLaunchKernelGGL((k_hash_ds2<9, DS>), dim3(pairs), dim3(128), pair_lds_bytes(9), st, p->dev, D, out);
        break;
    case PoseidonForm::Wide:
        if (t == 33) hipLaunchKernelGGL((k_hash_ds_wave<33, DS>), dim3(nodes), dim3(64), wave_lds_bytes(t), st, p->dev, D, out);
        else if (t == 65) hipLaunchKernelGGL((k_hash_ds_wave<65, DS>), dim3(nodes), dim3(64), wave_lds_bytes(t), st, p->dev, D, out);
        else hipLaunchKernelGGL((k_hash_ds_wave<129, DS>), dim3(nodes), dim3(64), wave_lds_bytes(t), st, p->dev, D, out);
        break;
    case PoseidonForm::Lane: {
        const int block = poseidon_block(t);
        hipLaunchKernelGGL(k_hash_ds<DS>, dim3((unsigned)((D.n_out + block - 1) / block)), dim3(block), poseidon_lds(t, block), st, p->dev, D, out);
    } }
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
int32_t stark::hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsStream& D, fr_t* out) { return launch_ds(ctx, st, p, D, out); }
int32_t stark::hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsGatherStream& D, fr_t* out) { return launch_ds(ctx, st, p, D, out); }
int32_t stark::hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsBatchStream& D, fr_t* out) { return launch_ds(ctx, st, p, D, out); }
int32_t stark::hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsBatchPairStream& D, fr_t* out) { return launch_ds(ctx, st, p, D, out); }
int32_t stark::hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsBatchPairPtrStream& D, fr_t* out) { return launch_ds(ctx, st, p, D, out); }
int32_t stark::hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsRaggedStream& D, fr_t* out) { return launch_ds(ctx, st, p, D, out); }
int32_t stark::hash_ds_on(stark_ctx* ctx, hipStream_t st, stark_params* p, const DsRaggedPairStream& D, fr_t* out) { return launch_ds(ctx, st, p, D, out); }
// The full 160 KiB of LDS per workgroup for the kernels that stage through it: every instantiation the launchers of this file can reach (a DS
// kernel: once per stream type hash_ds_on takes).  Not listed: the one-wave and wide kernels (k_*_coop, k_hash_ds_wave, k_tr_stream, k_tr_batch), whose
// coop_lds_bytes / wave_lds_bytes stay below the 64 KiB a kernel may use without the attribute.
static void lds_attr(const void* kernel) { (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds); }
template <class DS>
static void ds_attrs() {
    lds_attr((const void*)k_hash_ds<DS>); lds_attr((const void*)k_hash_ds2<17, DS>); lds_attr((const void*)k_hash_ds2<17, DS, true>); lds_attr((const void*)k_hash_ds2<9, DS>); lds_attr((const void*)k_hash_ds_chain<DS>);
}
void stark::poseidon_set_attrs() {
    ds_attrs<DsStream>(); ds_attrs<DsGatherStream>(); ds_attrs<DsBatchStream>(); ds_attrs<DsBatchPairStream>(); ds_attrs<DsBatchPairPtrStream>(); ds_attrs<DsRaggedStream>(); ds_attrs<DsRaggedPairStream>();
    for (const void* k : {(const void*)k_leaf_pair, (const void*)k_permute_batch, (const void*)k_tr_hash, (const void*)k_hash_stream, (const void*)k_leaf_pair2<false>, (const void*)k_leaf_pair2<true>, (const void*)k_node16_pair<false>, (const void*)k_node16_pair<true>,
                          (const void*)k_tr_hash_chain, (const void*)k_tr_hash_chain_ragged, (const void*)k_tr_hash_ragged, (const void*)k_leaf_pair_chain, (const void*)k_tr_stream_chain, (const void*)k_tr_batch_chain})
        lds_attr(k);
}
extern "C" {
int32_t stark_poseidon_hash_ds_batch_dev(stark_ctx_t* ctx, stark_params_t* p, size_t arity, uint32_t level, uint64_t pos0, uint64_t label, const uint64_t* in, size_t n_in, uint64_t* out) {
    if (!ctx || !p || !in || !out || arity == 0) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (host::width_for_arity(arity) != p->dev.t) return ctx->fail(STARK_ERR_INVALID_ARG, "arity incompatible with Poseidon width");
    STARK_TRY(ctx_enter(ctx));
    return hash_ds_on(ctx, ctx->stream, p, DsStream::make(0, arity, level, pos0, label, as_fr(in), nullptr, n_in), as_fr(out));
}
int32_t stark_poseidon_hash_ds_batch(stark_ctx_t* ctx, stark_params_t* p, size_t arity, uint32_t level, uint64_t pos0, uint64_t label, const uint64_t* in, size_t n_in, uint64_t* out) {
    if (!ctx || !p || !in || !out || arity == 0) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    size_t n_out = (n_in + arity - 1) / arity; DevBuf di, dout; CallerUploads up(ctx); STARK_HIP(ctx, up.up(di, in, n_in * sizeof(fr_t))); STARK_HIP(ctx, dout.alloc(ctx, n_out * sizeof(fr_t)));
    STARK_TRY(stark_poseidon_hash_ds_batch_dev(ctx, p, arity, level, pos0, label, (const uint64_t*)di.p, n_in, (uint64_t*)dout.p));
    STARK_HIP(ctx, up.download_sync(out, dout.p, n_out * sizeof(fr_t)));
    return STARK_OK;
}
}  // extern "C"
namespace stark {
// hash_leaf_pair is the FIXED transcript permutation (fri.rs:39: transcript::default_params()): a caller's handle must hold
// those very constants, anything else would silently mix two parameter sets (round 0 is folded into the context's template).
static bool same_consts(const host::PoseidonConsts& a, const host::PoseidonConsts& b) {
    if (a.t != b.t || a.rf != b.rf || a.rp != b.rp || a.mds.size() != b.mds.size() || a.rc_full.size() != b.rc_full.size() || a.rc_partial.size() != b.rc_partial.size()) return false;
    for (size_t i = 0; i < a.mds.size(); ++i) if (!fr_eq(a.mds[i], b.mds[i])) return false;
    for (size_t i = 0; i < a.rc_full.size(); ++i) if (!fr_eq(a.rc_full[i], b.rc_full[i])) return false;
    for (size_t i = 0; i < a.rc_partial.size(); ++i) if (!fr_eq(a.rc_partial[i], b.rc_partial[i])) return false;
    return true;
}
int32_t leaf_pair_hash_on(stark_ctx* ctx, hipStream_t st, const fr_t* f, const fr_t* f_next, size_t n, size_t m, fr_t* h) {
    if (!n) return STARK_OK;
    stark_params* tp = nullptr; STARK_TRY(ctx_transcript_params(ctx, &tp));
    const LeafConsts* lc = nullptr; STARK_TRY(ctx_leaf_init(ctx, &lc));
    const LeafStream L{reinterpret_cast<const fr_t*>(reinterpret_cast<const char*>(lc) + offsetof(LeafConsts, init)), f, f_next, m, n};      // LeafConsts::init on the device
    bool b8 = false; STARK_TRY(pair_block8_form(ctx, tp, &b8));
    if (tp->ref.rf < 4) b8 = false;      // k_leaf_pair2<true> hands round 0's rows to round 1's S-box: a full-round product must follow (the transcript set has rf = 8)
    switch (poseidon_form(ctx, tp, PoseidonOp::LeafLayer, n)) {
    case PoseidonForm::FiveWave: hipLaunchKernelGGL(k_leaf_pair_chain, dim3((unsigned)n), dim3(320), chain_lds_bytes(), st, tp->dev, row_consts_of(ctx), L, h); break;
    case PoseidonForm::OneWave: hipLaunchKernelGGL(k_leaf_pair_coop, dim3((unsigned)n), dim3(64), coop_lds_bytes(17), st, tp->dev, L, h); break;
    case PoseidonForm::WavePair:
        if (b8) hipLaunchKernelGGL(k_leaf_pair2<true>, dim3((unsigned)((n + 63) / 64)), dim3(128), pair_lds_bytes(17), st, tp->dev, lc, f, f_next, n, m, h);
        else hipLaunchKernelGGL(k_leaf_pair2<false>, dim3((unsigned)((n + 63) / 64)), dim3(128), pair_lds_bytes(17), st, tp->dev, lc, f, f_next, n, m, h);
        break;
    default: hipLaunchKernelGGL(k_leaf_pair, dim3((unsigned)((n + 63) / 64)), dim3(64), poseidon_lds(17, 64), st, tp->dev, L, h);
    }
    STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
}
}  // namespace stark
extern "C" {
int32_t stark_leaf_pair_hash_dev(stark_ctx_t* ctx, stark_params_t* tp, const uint64_t* f, const uint64_t* f_next, size_t n, size_t m, uint64_t* h) {
    if (!ctx || (!f && n) || (!h && n) || m == 0) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (tp) {    // NULL = the transcript parameters (the only valid choice); a handle is accepted when it holds the same constants
        if (tp->dev.t != 17) return ctx->fail(STARK_ERR_INVALID_ARG, "leaf hash uses the t=17 transcript permutation");
        stark_params* mine = nullptr; STARK_TRY(ctx_transcript_params(ctx, &mine));
        if (tp != mine && !same_consts(tp->ref, mine->ref)) return ctx->fail(STARK_ERR_INVALID_ARG, "hash_leaf_pair is defined over transcript::default_params(); the handle holds other constants");
    }
    return leaf_pair_hash_on(ctx, ctx->stream, as_fr(f), as_fr(f_next), n, m, as_fr(h));
}
int32_t stark_leaf_pair_hash(stark_ctx_t* ctx, stark_params_t* tp, const uint64_t* f, const uint64_t* f_next, size_t n, size_t m, uint64_t* h) {
    if (!ctx || (!f && n) || (!h && n) || m == 0) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    size_t nn = f_next ? (n + m - 1) / m : 0; DevBuf df, dn, dh; CallerUploads up(ctx);
    STARK_HIP(ctx, up.up(df, f, n * sizeof(fr_t))); STARK_HIP(ctx, up.up(dn, f_next, nn * sizeof(fr_t))); STARK_HIP(ctx, dh.alloc(ctx, n * sizeof(fr_t)));
    STARK_TRY(stark_leaf_pair_hash_dev(ctx, tp, (const uint64_t*)df.p, f_next ? (const uint64_t*)dn.p : nullptr, n, m, (uint64_t*)dh.p));
    STARK_HIP(ctx, up.download_sync(h, dh.p, n * sizeof(fr_t))); return STARK_OK;
}
int32_t stark_tr_hash_fields_tagged_dev(stark_ctx_t* ctx, stark_params_t* tp, const char* tag, const uint64_t* fields, size_t k, size_t n, uint64_t* out) {
    if (!ctx || !tag || (!fields && k && n) || (!out && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    (void)tp;   // the transcript permutation is fixed (transcript/src/lib.rs:44-46); the handle is accepted for API symmetry
    return tr_hash_dev(ctx, tag, as_fr(fields), k, n, as_fr(out));
}
int32_t stark_tr_hash_fields_tagged(stark_ctx_t* ctx, stark_params_t* tp, const char* tag, const uint64_t* fields, size_t k, size_t n, uint64_t* out) {
    if (!ctx || !tag || (!fields && k && n) || (!out && n)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    DevBuf di, dout; CallerUploads up(ctx); STARK_HIP(ctx, up.up(di, fields, n * k * sizeof(fr_t))); STARK_HIP(ctx, dout.alloc(ctx, n * sizeof(fr_t)));
    STARK_TRY(stark_tr_hash_fields_tagged_dev(ctx, tp, tag, (const uint64_t*)di.p, k, n, (uint64_t*)dout.p));
    STARK_HIP(ctx, up.download_sync(out, dout.p, n * sizeof(fr_t))); return STARK_OK;
}
int32_t stark_tr_hash_many_dev(stark_ctx_t* ctx, size_t n, const char* const* tags, const uint64_t* const* fields, const size_t* k, uint64_t* out) {
    if (!ctx) return STARK_ERR_INVALID_ARG;
    if (!n) return STARK_OK;
    if (!tags || !k || !out) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + n * sizeof(fr_t);
    for (size_t i = 0; i < n; ++i) {
        if (!tags[i]) return ctx->fail(STARK_ERR_INVALID_ARG, "tr_hash_many: null tag " + std::to_string(i));
        if (!k[i]) continue;
        if (!fields || !fields[i]) return ctx->fail(STARK_ERR_INVALID_ARG, "tr_hash_many: null fields with k > 0, item " + std::to_string(i));
        const uintptr_t f0 = (uintptr_t)fields[i];
        if (f0 < o1 && o0 < f0 + k[i] * sizeof(fr_t)) return ctx->fail(STARK_ERR_INVALID_ARG, "tr_hash_many: out overlaps the fields of item " + std::to_string(i));
    }
    return tr_hash_many_dev(ctx, n, tags, reinterpret_cast<const fr_t* const*>(fields), k, as_fr(out), false);
}

// ---- Merkle ------------------------------------------------------------------------------------------
}  // extern "C"
namespace stark {
// MerkleTree::new / new_pairs on `st`.  pairs: leaves are (f_i, cp[i / cp_div]) pairs (cp == nullptr: zeros).  level0: a pooled block that already
// holds the n leaves is MOVED into the tree as level 0 (no copy; `leaves` is not read); an empty one: level 0 is a copy of `leaves`.  On a failure
// the block is released once, by whoever holds it then: the caller's owner before the move, the tree that dies here after it.
int32_t merkle_build_on(stark_ctx* ctx, hipStream_t st, stark_params* p, size_t arity, uint64_t label, const fr_t* leaves, size_t n, int pairs, const fr_t* cp, size_t cp_div,
                        uint64_t first_pos, uint32_t level0, size_t stop_at_len, DevBuf&& level0_block, std::unique_ptr<stark_tree>& out) {
    if (n == 0) return ctx->fail(STARK_ERR_INVALID_ARG, "no leaves");                                                 // merkle/src/lib.rs:148
    if (host::width_for_arity(arity) != p->dev.t) return ctx->fail(STARK_ERR_INVALID_ARG, "arity incompatible with Poseidon width");   // :155-161
    if (arity == 1 && n > 1) return ctx->fail(STARK_ERR_UNSUPPORTED, "arity 1 with more than one leaf never terminates in the reference");
    std::unique_ptr<stark_tree> T(new stark_tree(ctx, p, arity, label));
    auto add_level = [&](DevBuf&& b, size_t len) { T->levels.push_back(b.fr()); T->lens.push_back(len); T->blocks.push_back(std::move(b)); };
    const bool moved_in = level0_block.p && !pairs;
    { DevBuf l0; if (moved_in) l0 = std::move(level0_block); else STARK_TRY(l0.take(ctx, n * sizeof(fr_t))); add_level(std::move(l0), n); }
    if (pairs) STARK_TRY(hash_ds_on(ctx, st, p, DsStream::make(1, arity, 0xFFFFFFFFu, first_pos, label, leaves, cp, n, cp_div), T->levels[0]));
    else if (!moved_in && hipMemcpyAsync(T->levels[0], leaves, n * sizeof(fr_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return ctx->fail(STARK_ERR_HIP, "copy leaves");
    uint32_t level = level0; uint64_t pos = first_pos; size_t stop = stop_at_len > 0 ? stop_at_len : 1;
    while (T->lens.back() > stop) {
        size_t len = T->lens.back(), nn = (len + arity - 1) / arity;
        if (pos % arity) return ctx->fail(STARK_ERR_INVALID_ARG, "shard offset not aligned to the arity");
        pos /= arity;
        { DevBuf nx; STARK_TRY(nx.take(ctx, nn * sizeof(fr_t))); add_level(std::move(nx), nn); }
        STARK_TRY(hash_ds_on(ctx, st, p, DsStream::make(0, arity, level, pos, label, T->levels[T->levels.size() - 2], nullptr, len), T->levels.back()));
        level += 1;
    }
    out = std::move(T); return STARK_OK;
}
}  // namespace stark
extern "C" {
int32_t stark_merkle_build_dev(stark_ctx_t* ctx, stark_params_t* p, size_t arity, uint64_t label, const uint64_t* leaves, size_t n, int32_t pairs, const uint64_t* cp,
                               uint64_t first_pos, uint32_t level0, int32_t stop_at_len, stark_tree_t** out) {
    if (!ctx || !p || !leaves || !out || arity == 0 || (pairs && !cp)) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad merkle args") : STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    std::unique_ptr<stark_tree> T;
    STARK_TRY(merkle_build_on(ctx, ctx->stream, p, arity, label, as_fr(leaves), n, pairs, as_fr(cp), 1, first_pos, level0, stop_at_len > 0 ? (size_t)stop_at_len : 0, DevBuf(), T));
    *out = T.release(); return STARK_OK;
}
int32_t stark_merkle_build(stark_ctx_t* ctx, stark_params_t* p, size_t arity, uint64_t label, const uint64_t* leaves, size_t n, int32_t pairs, const uint64_t* cp, stark_tree_t** out) {
    if (!ctx || !p || !leaves || !out || (pairs && !cp)) return STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    if (n == 0) return ctx->fail(STARK_ERR_INVALID_ARG, "no leaves");
    DevBuf dl, dc; CallerUploads up(ctx); STARK_HIP(ctx, up.up(dl, leaves, n * sizeof(fr_t)));
    if (pairs) STARK_HIP(ctx, up.up(dc, cp, n * sizeof(fr_t)));
    STARK_TRY(stark_merkle_build_dev(ctx, p, arity, label, (const uint64_t*)dl.p, n, pairs, pairs ? (const uint64_t*)dc.p : nullptr, 0, 0, 0, out));
    STARK_HIP(ctx, up.sync()); return STARK_OK;
}
int32_t stark_merkle_num_levels(stark_tree_t* t) { return t ? (int32_t)t->levels.size() : STARK_ERR_INVALID_ARG; }
size_t stark_merkle_level_len(stark_tree_t* t, int32_t lvl) { return (t && lvl >= 0 && (size_t)lvl < t->lens.size()) ? t->lens[lvl] : 0; }
const uint64_t* stark_merkle_level_dev(stark_tree_t* t, int32_t lvl) { return (t && lvl >= 0 && (size_t)lvl < t->levels.size()) ? (const uint64_t*)t->levels[lvl] : nullptr; }
int32_t stark_merkle_level(stark_tree_t* t, int32_t lvl, uint64_t* out) {
    if (!t || !out || lvl < 0 || (size_t)lvl >= t->levels.size()) return STARK_ERR_INVALID_ARG;
    stark_ctx* ctx = t->ctx; STARK_TRY(ctx_enter(ctx));
    STARK_HIP(ctx, hipMemcpyAsync(out, t->levels[lvl], t->lens[lvl] * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream)); return STARK_OK;
}
int32_t stark_merkle_root(stark_tree_t* t, uint64_t* out4) {
    if (!t || !out4) return STARK_ERR_INVALID_ARG;
    if (t->lens.back() != 1) return t->ctx->fail(STARK_ERR_INVALID_ARG, "partial (sharded) tree has no root");
    return stark_merkle_level(t, (int32_t)t->levels.size() - 1, out4);
}
int32_t stark_merkle_gather(stark_tree_t* t, int32_t lvl, const size_t* idx, size_t k, uint64_t* out) {
    if (!t || (!idx && k) || (!out && k) || lvl < 0 || (size_t)lvl >= t->levels.size()) return STARK_ERR_INVALID_ARG;
    stark_ctx* ctx = t->ctx; if (!k) return STARK_OK;
    STARK_TRY(ctx_enter(ctx));
    for (size_t i = 0; i < k; ++i) if (idx[i] >= t->lens[lvl]) return ctx->fail(STARK_ERR_INVALID_ARG, "gather index out of range");
    MerkleGatherList G; G.level(t->levels[lvl], std::vector<size_t>(idx, idx + k));
    return gather_rows(ctx, G, nullptr, out);
}
int32_t stark_merkle_free(stark_tree_t* t) { if (!t) return STARK_ERR_INVALID_ARG; delete t; return STARK_OK; }   // levels go back to the context's pool (stream-ordered reuse: no device sync)

}  // extern "C"

// ---- many trees in one pass (merkle_batch.hpp) ----------------------------------------------------------------------------------------------------
namespace stark {
// The device executor of merkle_build_batch: every step is one launch on the context's stream (a few, for more than 65535 trees in the copy), the
// level blocks are pooled and owned by the holder the batch's trees share, and the labels and pointer tables go up as ONE staged upload.
struct MerkleBatchDevExec {
    stark_ctx* ctx; stark_params* p; std::shared_ptr<TreeBlocks> blocks; DevArena mem;
    MerkleBatchDevExec(stark_ctx* c, stark_params* p_) : ctx(c), p(p_), blocks(std::make_shared<TreeBlocks>()), mem(c) {}
    int32_t level_block(size_t n_fr, fr_t** out) {
        DevBuf b; STARK_TRY(b.take(ctx, n_fr * sizeof(fr_t))); *out = b.fr(); blocks->blocks.push_back(std::move(b)); return STARK_OK;
    }
    int32_t tables(const uint64_t* labels, const fr_t* const* leaves, const fr_t* const* cp, size_t B, const uint64_t** labels_x, const fr_t* const** leaves_x, const fr_t* const** cp_x) {
        std::vector<uint64_t> h((cp ? 3 : 2) * B);                       // [labels | leaves | cp], eight bytes each
        for (size_t b = 0; b < B; ++b) { h[b] = labels[b]; h[B + b] = (uint64_t)(uintptr_t)leaves[b]; if (cp) h[2 * B + b] = (uint64_t)(uintptr_t)cp[b]; }
        uint64_t* d = nullptr; STARK_TRY(mem.put(h, &d));
        *labels_x = d; *leaves_x = (const fr_t* const*)(d + B); *cp_x = cp ? (const fr_t* const*)(d + 2 * B) : nullptr; return STARK_OK;
    }
    int32_t copy_rows(const fr_t* const* src_x, size_t n, size_t B, fr_t* dst) {
        for (size_t b0 = 0; b0 < B; b0 += 65535)
            hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)((n + 255) / 256), (unsigned)std::min<size_t>(65535, B - b0)), dim3(256), 0, ctx->stream, src_x + b0, (uint64_t)n, dst + b0 * n);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
    template <class DS> int32_t hash_level(const DS& D, fr_t* out) { return hash_ds_on(ctx, ctx->stream, p, D, out); }
};
int32_t merkle_build_batch_on(stark_ctx* ctx, stark_params* p, size_t arity, size_t batch, const uint64_t* labels, const uint64_t* const* leaves, size_t n, int pairs,
                              const uint64_t* const* cp, stark_tree** out) {
    for (size_t b = 0; b < batch; ++b) out[b] = nullptr;
    if (n == 0) return ctx->fail(STARK_ERR_INVALID_ARG, "no leaves");                                                 // merkle/src/lib.rs:148
    if (arity == 0 || host::width_for_arity(arity) != p->dev.t) return ctx->fail(STARK_ERR_INVALID_ARG, "arity incompatible with Poseidon width");   // :155-161
    if (arity == 1 && n > 1) return ctx->fail(STARK_ERR_UNSUPPORTED, "arity 1 with more than one leaf never terminates in the reference");
    for (size_t b = 0; b < batch; ++b) if (!leaves[b]) return ctx->fail(STARK_ERR_INVALID_ARG, "null leaves entry");
    if (n > 0x7fffffffu / batch) return ctx->fail(STARK_ERR_INVALID_ARG, "batch x n exceeds 2^31 - 1 leaves: one level of the batch is one launch");
    MerkleBatchDevExec X(ctx, p);
    std::vector<size_t> lens; std::vector<fr_t*> base;
    STARK_TRY(merkle_build_batch(X, arity, batch, labels, reinterpret_cast<const fr_t* const*>(leaves), n, pairs, reinterpret_cast<const fr_t* const*>(cp), lens, base));
    std::vector<std::unique_ptr<stark_tree>> trees(batch);
    for (size_t b = 0; b < batch; ++b) {
        trees[b].reset(new stark_tree(ctx, p, arity, labels[b])); trees[b]->shared = X.blocks;
        for (size_t v = 0; v < lens.size(); ++v) { trees[b]->levels.push_back(base[v] + b * lens[v]); trees[b]->lens.push_back(lens[v]); }
    }
    for (size_t b = 0; b < batch; ++b) out[b] = trees[b].release();                      // the single success point
    return STARK_OK;
}
// The device executor of merkle_build_mixed_batch: the batch executor's blocks and arena, one staged upload for every segment table of the call.
struct MerkleMixedDevExec : MerkleBatchDevExec {
    using MerkleBatchDevExec::MerkleBatchDevExec;
    int32_t segments(const std::vector<DsRaggedStream::Seg>& h, const DsRaggedStream::Seg** x) { DsRaggedStream::Seg* d = nullptr; STARK_TRY(mem.put(h, &d)); *x = d; return STARK_OK; }
    int32_t copy_ragged(const DsRaggedStream& D, fr_t* dst) {
        hipLaunchKernelGGL(k_copy_ragged, dim3((unsigned)((D.n_out + 255) / 256)), dim3(256), 0, ctx->stream, D, dst);
        STARK_HIP(ctx, hipGetLastError()); return STARK_OK;
    }
};
int32_t merkle_build_mixed_batch_on(stark_ctx* ctx, stark_params* p, size_t arity, size_t batch, const uint64_t* labels, const uint64_t* const* leaves, const size_t* n, int pairs,
                                    const uint64_t* const* cp, stark_tree** out) {
    for (size_t b = 0; b < batch; ++b) out[b] = nullptr;
    if (arity == 0 || host::width_for_arity(arity) != p->dev.t) return ctx->fail(STARK_ERR_INVALID_ARG, "arity incompatible with Poseidon width");   // :155-161
    size_t sum = 0;
    for (size_t b = 0; b < batch; ++b) {
        if (!leaves[b]) return ctx->fail(STARK_ERR_INVALID_ARG, "null leaves entry");
        if (n[b] == 0) return ctx->fail(STARK_ERR_INVALID_ARG, "no leaves");                                          // merkle/src/lib.rs:148
        if (n[b] > 0x7fffffffu - sum) return ctx->fail(STARK_ERR_INVALID_ARG, "the sum of n exceeds 2^31 - 1 leaves: one level of the batch is one launch");
        sum += n[b];
    }
    if (arity == 1 && sum > batch) return ctx->fail(STARK_ERR_UNSUPPORTED, "arity 1 with more than one leaf never terminates in the reference");
    MerkleMixedDevExec X(ctx, p);
    std::vector<std::vector<size_t>> lens, at; std::vector<fr_t*> base;
    STARK_TRY(merkle_build_mixed_batch(X, arity, batch, labels, reinterpret_cast<const fr_t* const*>(leaves), n, pairs, reinterpret_cast<const fr_t* const*>(cp), lens, at, base));
    std::vector<std::unique_ptr<stark_tree>> trees(batch);
    for (size_t b = 0; b < batch; ++b) {
        trees[b].reset(new stark_tree(ctx, p, arity, labels[b])); trees[b]->shared = X.blocks;
        for (size_t v = 0; v < lens[b].size(); ++v) { trees[b]->levels.push_back(base[v] + at[b][v]); trees[b]->lens.push_back(lens[b][v]); }
    }
    for (size_t b = 0; b < batch; ++b) out[b] = trees[b].release();                      // the single success point
    return STARK_OK;
}
// THE row gather (declared in ctx.hpp): stark_merkle_gather, stark_merkle_roots_batch, every Merkle open and every DEEP-FRI query phase end here.
int32_t gather_rows(stark_ctx* ctx, const MerkleGatherList& G, fr_t* out_dev, void* out_host) {
    const size_t k = G.size(), nb = G.base.size();
    if (!k) return STARK_OK;
    std::vector<uint64_t> h(nb + 2 * k + (k + 1) / 2);                   // [base | index | row | src (u32)]
    for (size_t i = 0; i < nb; ++i) h[i] = (uint64_t)(uintptr_t)G.base[i];
    for (size_t i = 0; i < k; ++i) { h[nb + i] = G.index[i]; h[nb + k + i] = G.row_of(i); }
    memcpy(h.data() + nb + 2 * k, G.src.data(), k * 4);
    DevBuf d, o; STARK_HIP(ctx, d.alloc(ctx, h.size() * 8));
    if (!out_dev) { STARK_HIP(ctx, o.alloc(ctx, k * sizeof(fr_t))); out_dev = o.fr(); }
    STARK_TRY(ctx_upload_staged(ctx, d.p, h.data(), h.size() * 8));
    const uint64_t* t = (const uint64_t*)d.p;
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, ctx->stream, (const fr_t* const*)t, (const uint32_t*)(t + nb + 2 * k), t + nb, t + nb + k, (uint64_t)k, out_dev);
    STARK_HIP(ctx, hipGetLastError());
    if (!out_host) return STARK_OK;
    STARK_HIP(ctx, hipMemcpyAsync(out_host, out_dev, k * sizeof(fr_t), hipMemcpyDeviceToHost, ctx->stream)); STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return STARK_OK;
}
// merkle_open_batch's executor: every sibling of every tree and level of a call through that one gather
struct MerkleOpenDevExec { stark_ctx* ctx; int32_t gather(const MerkleGatherList& G, fr_t* out_host) { return gather_rows(ctx, G, nullptr, out_host); } };
// the trees of one call: all non-null, complete and of one context
static int32_t same_ctx_trees(stark_tree* const* trees, size_t batch, stark_ctx** ctx) {
    for (size_t b = 0; b < batch; ++b) if (!trees[b]) return STARK_ERR_INVALID_ARG;
    stark_ctx* c = trees[0]->ctx;
    for (size_t b = 1; b < batch; ++b) if (trees[b]->ctx != c) return c->fail(STARK_ERR_INVALID_ARG, "the trees of a batch must share one context");
    for (size_t b = 0; b < batch; ++b) if (trees[b]->lens.back() != 1) return c->fail(STARK_ERR_INVALID_ARG, "partial (sharded) tree in a batch");
    *ctx = c; return STARK_OK;
}
}  // namespace stark

extern "C" {
int32_t stark_merkle_build_batch_dev(stark_ctx_t* ctx, stark_params_t* p, size_t arity, size_t batch, const uint64_t* tree_labels, const uint64_t* const* leaves, size_t n, int32_t pairs,
                                     const uint64_t* const* cp, stark_tree_t** out) {
    if (!batch) return STARK_OK;
    if (!out) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad merkle batch args") : STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) out[b] = nullptr;
    if (!ctx || !p || !tree_labels || !leaves || (pairs && !cp)) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad merkle batch args") : STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return merkle_build_batch_on(ctx, p, arity, batch, tree_labels, leaves, n, pairs, pairs ? cp : nullptr, out);
}
int32_t stark_merkle_build_mixed_batch_dev(stark_ctx_t* ctx, stark_params_t* p, size_t arity, size_t batch, const uint64_t* tree_labels, const uint64_t* const* leaves, const size_t* n,
                                           int32_t pairs, const uint64_t* const* cp, stark_tree_t** out) {
    if (!batch) return STARK_OK;
    if (!out) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad merkle batch args") : STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) out[b] = nullptr;
    if (!ctx || !p || !tree_labels || !leaves || !n || (pairs && !cp)) return ctx ? ctx->fail(STARK_ERR_INVALID_ARG, "bad merkle batch args") : STARK_ERR_INVALID_ARG;
    STARK_TRY(ctx_enter(ctx));
    return merkle_build_mixed_batch_on(ctx, p, arity, batch, tree_labels, leaves, n, pairs, pairs ? cp : nullptr, out);
}
int32_t stark_merkle_roots_batch(stark_tree_t* const* trees, size_t batch, uint64_t* roots) {
    if (!batch) return STARK_OK;
    if (!trees || !roots) return STARK_ERR_INVALID_ARG;
    stark_ctx* ctx = nullptr; STARK_TRY(same_ctx_trees(trees, batch, &ctx));
    STARK_TRY(ctx_enter(ctx));
    MerkleGatherList G;
    for (size_t b = 0; b < batch; ++b) G.level(trees[b]->levels.back(), std::vector<size_t>(1, 0));
    return gather_rows(ctx, G, nullptr, roots);
}
int32_t stark_merkle_open_batch(stark_tree_t* const* trees, size_t batch, const size_t* idx, const size_t* idx_off, stark_proof_t** out) {
    if (!batch) return STARK_OK;
    if (!out) return STARK_ERR_INVALID_ARG;
    for (size_t b = 0; b < batch; ++b) out[b] = nullptr;
    if (!trees || !idx || !idx_off) return STARK_ERR_INVALID_ARG;
    stark_ctx* ctx = nullptr; STARK_TRY(same_ctx_trees(trees, batch, &ctx));
    STARK_TRY(ctx_enter(ctx));
    std::vector<MerkleTreeView> views(batch);
    for (size_t b = 0; b < batch; ++b) views[b] = MerkleTreeView{trees[b]->arity, &trees[b]->lens, trees[b]->levels.data()};
    MerkleOpenDevExec X{ctx}; std::vector<std::vector<uint8_t>> proofs;
    const int32_t rc = merkle_open_batch(X, views.data(), batch, idx, idx_off, proofs);
    if (rc == -1) return ctx->fail(STARK_ERR_INVALID_ARG, "open batch: idx_off not increasing, an empty index list or a leaf index out of range");
    if (rc) return rc;
    std::vector<std::unique_ptr<stark_proof>> pf(batch);
    for (size_t b = 0; b < batch; ++b) { pf[b].reset(new stark_proof()); pf[b]->bytes = std::move(proofs[b]); }
    hand_out(pf, out); return STARK_OK;
}
// open_union_of_paths (merkle/src/lib.rs:246-315) of one tree: merkle_open_batch over one view.  The three refusals keep their own wording (they run
// first, so the batch driver's one message for all of them never surfaces here).
int32_t stark_merkle_open(stark_tree_t* t, const size_t* idx, size_t k, uint8_t* buf, size_t cap, size_t* len) {
    if (!t || !len || (!idx && k)) return STARK_ERR_INVALID_ARG;
    stark_ctx* ctx = t->ctx;
    if (!k) return ctx->fail(STARK_ERR_INVALID_ARG, "open_many: empty indices");                                        // :247
    if (t->lens.back() != 1) return ctx->fail(STARK_ERR_INVALID_ARG, "cannot open a partial tree");
    for (size_t i = 0; i < k; ++i) if (idx[i] >= t->lens[0]) return ctx->fail(STARK_ERR_INVALID_ARG, "leaf index out of range");
    STARK_TRY(ctx_enter(ctx));
    const MerkleTreeView view{t->arity, &t->lens, t->levels.data()}; const size_t off[2] = {0, k};
    MerkleOpenDevExec X{ctx}; std::vector<std::vector<uint8_t>> proofs;
    STARK_TRY(merkle_open_batch(X, &view, 1, idx, off, proofs));
    const std::vector<uint8_t>& b = proofs[0];
    *len = b.size();
    if (buf) { if (cap < b.size()) return ctx->fail(STARK_ERR_INVALID_ARG, "buffer too small"); memcpy(buf, b.data(), b.size()); }
    return STARK_OK;
}
}  // extern "C"
