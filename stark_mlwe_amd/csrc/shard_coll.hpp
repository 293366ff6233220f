// stark_mlwe_amd/csrc/shard_coll.hpp — the collectives of the sharded operations: the LDE (capi_ntt.hip) and the FRI commit and prove
// (fri_shard_impl.hpp).  One object serves all the LOCAL ranks of a driver.  A real instance has one, the communicator's rank (rank 0 of 1
// without a communicator: every collective is then nothing or a device copy).  An emulated instance has W virtual ranks 0..W-1 on one GPU and
// does every collective as device copies, which is how the tests reach the W > 1 index arithmetic without a second GPU.
// Every buffer argument holds one entry per local rank.
#pragma once
#include <vector>
#include "ctx.hpp"
#include "fri_dev.hpp"

namespace stark {

struct ShardColl {
    stark_ctx* ctx; int W; bool emulated;
    int rank0, nlocal;                                    // the local ranks: rank0 .. rank0 + nlocal - 1
    static ShardColl real(stark_ctx* ctx) { return ctx->comm ? ShardColl{ctx, stark_comm_size(ctx), false, stark_comm_rank(ctx), 1} : ShardColl{ctx, 1, false, 0, 1}; }
    static ShardColl emulate(stark_ctx* ctx, int W) { return ShardColl{ctx, W, true, 0, W}; }
    int rank(size_t i) const { return rank0 + (int)i; }
    size_t local() const { return (size_t)nlocal; }      // read only once W is checked
    // The block of a caller's array that local rank i works on: a real caller passes its own block, an emulated one the whole array.
    size_t block(size_t i) const { return emulated ? (size_t)rank(i) : 0; }
    bool local_copy() const { return !emulated && W == 1 && !ctx->comm; }

    // send[i]: W chunks of `bytes`, chunk q for rank q; recv[i]: chunk p is what rank p sent to local rank i.  send != recv.
    int32_t all_to_all(const std::vector<const void*>& send, const std::vector<void*>& recv, size_t bytes) const {
        if (!bytes) return STARK_OK;
        if (local_copy()) { STARK_HIP(ctx, hipMemcpyAsync(recv[0], send[0], bytes, hipMemcpyDeviceToDevice, ctx->stream)); return STARK_OK; }
        if (!emulated) return stark_comm_all_to_all_dev(ctx, send[0], recv[0], bytes);
        for (int p = 0; p < W; ++p) for (int q = 0; q < W; ++q)
            STARK_HIP(ctx, hipMemcpyAsync((char*)recv[q] + (size_t)p * bytes, (const char*)send[p] + (size_t)q * bytes, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return STARK_OK;
    }
    // in place: buf[i] holds W chunks of `bytes`; local rank i's own chunk is at rank(i) * bytes
    int32_t all_gather(const std::vector<void*>& buf, size_t bytes) const {
        if (!bytes || local_copy()) return STARK_OK;
        if (!emulated) return stark_comm_all_gather_dev(ctx, (const char*)buf[0] + (size_t)rank0 * bytes, buf[0], bytes);
        for (int p = 0; p < W; ++p) for (int q = 0; q < W; ++q) if (p != q)
            STARK_HIP(ctx, hipMemcpyAsync((char*)buf[q] + (size_t)p * bytes, (const char*)buf[p] + (size_t)p * bytes, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return STARK_OK;
    }
    // SUM of `count` uint64 words, in place
    int32_t all_reduce(const std::vector<void*>& buf, size_t count) const {
        if (!count || local_copy()) return STARK_OK;
        if (!emulated) return stark_comm_all_reduce_u64_dev(ctx, buf[0], buf[0], count);
        for (int q = 1; q < W; ++q) { hipLaunchKernelGGL(k_add_u64, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, (uint64_t*)buf[0], (const uint64_t*)buf[q], (uint64_t)count); STARK_HIP(ctx, hipGetLastError()); }
        for (int q = 1; q < W; ++q) STARK_HIP(ctx, hipMemcpyAsync(buf[q], buf[0], count * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return STARK_OK;
    }
    // send[i] (`bytes`) to rank `root`; recv: the root's buffer of W chunks, or null when the root is not local
    int32_t gather(const std::vector<const void*>& send, void* recv, size_t bytes, int root) const {
        if (!bytes) return STARK_OK;
        if (local_copy()) { STARK_HIP(ctx, hipMemcpyAsync(recv, send[0], bytes, hipMemcpyDeviceToDevice, ctx->stream)); return STARK_OK; }
        if (!emulated) return stark_comm_gather_dev(ctx, send[0], rank0 == root ? recv : nullptr, bytes, root);
        for (int p = 0; p < W; ++p) STARK_HIP(ctx, hipMemcpyAsync((char*)recv + (size_t)p * bytes, send[p], bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return STARK_OK;
    }
};

}  // namespace stark
