// stark_mlwe_amd/csrc/sumcheck_impl.hpp — the host-only part of the sum-check consumer (the device part: capi_sumcheck.hip)
// the provers' transcript labels and the batched round loops / verification plans that hostcheck.cpp runs on the host as well.
#pragma once
#include "fri_verify.hpp"

// The provers' transcript labels, the reference's strings verbatim (channel/src/lib.rs).  The round loops of sumcheck_batch.hpp lay out
// their absorbs with these, as the verification plans of sumcheck_verify_batch.hpp do, and the host-check library includes this file for them.
namespace stark { namespace sc_lab {
constexpr const char *digest = "CHAN/SEND/DIGEST", *open = "CHAN/SEND/OPEN", *arity = "PROOF/ARITY", *group_sizes = "PROOF/GROUP_SIZES",
                     *siblings = "PROOF/SIBLINGS";                                                                          // :22-56
constexpr const char *plain = "E2E/PLAIN", *root = "commit/root", *claim = "SUMCHECK/CLAIM", *round = "SUMCHECK/ROUND", *c0 = "COEFF/c0",
                     *c1 = "COEFF/c1", *r = "sumcheck/r";                                                                   // :175, :442-472, :1064
constexpr const char *mf = "E2E/MF", *mf_round_chal = "SUMCHECK-MF/ROUND-CHAL", *mf_r = "SUMCHECK/MF/R", *r_i = "r_i", *mf_root0 = "sumcheck-mf/root/0",
                     *mf_claim = "SUMCHECK/MF/CLAIM", *mf_round = "SUMCHECK/MF/ROUND", *mf_root_next = "sumcheck-mf/root/next", *mf_q = "sumcheck-mf/q";   // :593-735
// finalize_eval absorbs "SUMCHECK/FINAL/EVAL" / "SUMCHECK/MF/FINAL/EVAL" and the final value last (:474-484, :732-738); nothing is drawn
// after it, so no launch would ever run that absorb and the provers leave it out.
} }
#include "sumcheck_batch.hpp"
#include "sumcheck_verify_batch.hpp"
