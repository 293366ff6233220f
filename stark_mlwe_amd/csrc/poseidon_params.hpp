// stark_mlwe_amd/csrc/poseidon_params.hpp — device view of the Poseidon constants (kernel form).
#pragma once
#include <cstddef>
#include <type_traits>
#include "fr.hpp"
namespace stark {
struct PoseidonDev {           // device pointers to kernel-form constants (see host_util.hpp KernelConsts)
    int t, rf, rp;
    const fr_t* rc_full;       // rf*t
    const fr_t* rc_partial;    // rp
    const fr_t* lu;            // t*t  LU(M)
    const fr_t* lu_pre;        // t*t  LU(B_1*M)
    const fr_t* row0;          // t    M[0][*]
    const fr_t* sparse;        // rp*(2t-1)
    const fr_t* mds;           // t*t  reference form
    const fr_t* mds_pre;       // t*t  dense B_1*M
    const fr_t* gamma;         // (rp/4)*6  cross terms of the 4-round partial blocks
    // the same multiplier tables in radix 2^29, R' = 2^261 domain, 9 words per entry (fr29.hpp): what the dot products read
    const uint32_t* lu29; const uint32_t* lu_pre29; const uint32_t* row0_29; const uint32_t* sparse29; const uint32_t* gamma29;
    const uint32_t* mds29; const uint32_t* mds_pre29;   // dense M and B_1*M (one-wave kernel)
    const void* mds_frag; const void* mds_pre_frag;     // t = 17: the same two matrices as int8 MFMA fragments (host_util.hpp mfma_frags); nullptr otherwise
    // t = 17: the partial rounds unrolled over all rp rounds for the five-wave latency kernel (host_util.hpp chain_*, poseidon_chain.hpp); nullptr otherwise
    const uint32_t* chain_a; const uint32_t* chain_g; const uint32_t* chain_w;
    // t = 17, rp % 8 == 0: the 8-round partial blocks of the wave-pair kernels (host_util.hpp blk8_*, poseidon_pair.hpp pair_block8); nullptr otherwise
    // The device holds the SCALED family (KernelConsts blk8s_*: the chain carries lambda_q X_q), the unit fragment and rc_partial_scaled29: the rp scaled round
    // constants lambda_q c_q as nine 29-bit limbs of their stored value and a zero entry for "no round follows" (they enter the finish of the row their round
    // consumes), and right behind them the nine limbs of the multiplier 1 / lambda_rp that brings the chain value back after the last block
    // (blk8_unscale29 below: one pointer for both, the wave-pair kernels have no scalar register to spare).  The unscaled family stays on the host.
    const void* blk8_efrag; const void* blk8_lfrag; const void* blk8_unit_frag; const void* blk8_gfrag;
    const uint32_t* rc_partial_scaled29;       // (rp + 1) * 9, then blk8_unscale29
    FR_HD const uint32_t* blk8_unscale29() const { return rc_partial_scaled29 + (size_t)(rp + 1) * 9; }
    // the full rounds' constants again as nine 29-bit limbs of their STORED value (fr29_unpack; not the R' domain of the multiplier tables), 9 words per entry:
    // added limb by limb to a product row that stays in limbs up to its S-box (poseidon_pair.hpp sbox_lazy29)
    const uint32_t* rc_full29;
};

// The leaf constants of hash_leaf_pair on the device (capi_poseidon.hip ctx_leaf_init fills it): the 17-lane template, of which lanes 4, 5 = (f, s) are the only
// inputs, and round 0 in closed form for the wave-pair kernels (host_util.hpp leaf_round0_consts): the MDS output is K_i + M[i][4] x4 + M[i][5] x5.
struct LeafConsts {
    fr_t init[17];                              // the template (every leaf kernel; LeafStream::init)
    fr_t K[17];                                 // K_i = sum_{j != 4, 5} M[i][j] (init_j + rc0_j)^5
    fr_t m4[17], m5[17];                        // columns 4 and 5 of M
    alignas(16) uint32_t m45_29[2 * 17 * 9];    // the two columns times 2^20 as multiplier-table entries in radix 2^29, m4 then m5 (k_leaf_pair2<false>)
    alignas(16) uint32_t krc29[17 * 9];         // (K_i + round 1's constant) mod r as nine limbs of the stored value (k_leaf_pair2<true>, pair_leaf_round0_mfma)
};
static_assert(std::is_trivially_copyable<LeafConsts>::value, "uploaded byte for byte");
static_assert(offsetof(LeafConsts, m45_29) % 16 == 0 && offsetof(LeafConsts, krc29) % 16 == 0, "the 32-bit tables start at 16 bytes, as the field elements in front of them do");

}  // namespace stark
