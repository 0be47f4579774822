// Launch sequence of the block verifier's kernels (verify_kernels.hpp) from k_verify_front through k_verify_affine, and
// the filling of a device key: one place for both, shared by verify_dev.hip (verify_block, capgpu_plonk_vk_upload) and by
// the direct driver of these kernels (tests/hip/verifycheck.hip), so that the driver runs each kernel in the order and
// geometry the verifier gives it and builds its keys with the verifier's code.  Host side only; nothing here waits.
#pragma once
#include <string.h>

#include "launch.hpp"
#include "msm.hpp"
#include "verify_kernels.hpp"
#include "verify_terms.hpp"

namespace cap {
namespace vf {

// Fills a DevVk from the ABI's key: the coset constants, the 18 commitments and the generator, n with n_mont and omega,
// and the transcript prefix.  domain_size (a power of two in [4, 2^28]) and num_inputs are the caller's to check.
// Returns -1, or the first field that is not canonical / not a point of the curve: 0..4 for k[i], 5 + i for commitment i
// (13 selectors, then 5 sigmas); `out` is then unfinished.
inline int dev_vk_fill(const capgpu_verifying_key* vk, DevVk* out) {
  DevVk& k = *out;
  memset(&k, 0, sizeof k);
  for (int i = 0; i < 5; i++) {
    memcpy(&k.k[i], vk->k[i], 32);
    if (Fr::geq_mod(k.k[i])) return i;
  }
  for (int i = 0; i < 18; i++) {
    k.pts[i] = g1_from_abi(i < 13 ? vk->selector_comms[i] : vk->sigma_comms[i - 13]);
    if (!g1_abi_on_curve(k.pts[i])) return 5 + i;
  }
  k.pts[18].x = Fq::one();
  k.pts[18].y = Fq::dbl(Fq::one());
  const uint64_t n = vk->domain_size;
  k.n = n;
  k.num_inputs = (uint32_t)vk->num_inputs;
  fe nw = Fr::zero();
  nw.v[0] = (uint32_t)n;
  nw.v[1] = (uint32_t)(n >> 32);
  k.n_mont = Fr::to_mont(nw);
  k.omega = domain_generator(n);
  prefix_bytes(k, k.prefix);
  return -1;
}

}  // namespace vf

namespace CAP_VK_NS {

// the device buffers of one block between its proofs and its two sums
struct FoldArgs {
  FrontArgs front;             // the proofs, rows, keys, messages and what the front end writes (front.count proofs)
  uint32_t nkeys;
  uint8_t* seed;               // 32 bytes: S
  fe* w;                       // count weights
  g1_affine* mpts;             // vf::kOwnTerms * count + vf::kKeyTerms * nkeys points of the two MSMs
  fe* msc;                     // and their scalars
  const MsmVarDesc* desc;      // device: A over [0, 2 count), B over the rest
  g1_jac* sums;                // 2
  void* msm_ws;                // msm_var_plan(msm_pts - 2 count, msm_pts, 2).workspace_bytes
  size_t msm_ws_bytes;
  g1_affine* ab;               // A and -B
};

// Enqueues k_verify_front, k_verify_seed, k_verify_weights, k_verify_gather, k_verify_fold, the two one-shot MSMs and
// k_verify_affine on s.  Returns msm_var_run's code (0: fine).  A launch that failed is left in launch_error() for the
// caller to take, and nothing is enqueued behind it.
inline int fold_launch(const FoldArgs& a, hipStream_t s) {
  const uint32_t n = a.front.count;
  const size_t msm_pts = (size_t)vf::kOwnTerms * n + (size_t)vf::kKeyTerms * a.nkeys;
  const size_t nb = msm_pts - (size_t)vf::kATerms * n;
  const uint8_t* d_proofs = a.front.proofs;
  const vf::DevVk* const* d_keys = a.front.keys;
  const uint32_t* d_meta = a.front.meta;
  int* d_valid = a.front.valid;
  fe* d_sc = a.front.sc;
  launch("k_verify_front", k_verify_front, dim3(n), dim3(64), 0, s, a.front);
  launch("k_verify_seed", k_verify_seed, dim3(1), dim3(64), 0, s, (const uint8_t*)a.front.ubytes, n, a.seed);
  launch("k_verify_weights", k_verify_weights, dim3(n), dim3(64), 0, s, (const uint8_t*)a.seed, n, a.w);
  launch("k_verify_gather", k_verify_gather, dim3((n * vf::kOwnTerms + 63) / 64), dim3(64), 0, s, d_proofs,
         (const fe*)d_sc, (const fe*)a.w, (const int*)d_valid, n, a.mpts, a.msc);
  launch("k_verify_fold", k_verify_fold, dim3((unsigned)a.nkeys, vf::kKeyTerms), dim3(64), 0, s, d_keys, d_meta,
         (const fe*)d_sc, (const fe*)a.w, (const int*)d_valid, n, a.mpts, a.msc);
  if (launch_error().code != hipSuccess) return 0;
  const int rc = msm_var_run(a.mpts, msm_pts, a.msc, 0, a.desc, nb, 2, 1, a.sums, a.msm_ws, a.msm_ws_bytes, s);
  if (rc) return rc;
  launch("k_verify_affine", k_verify_affine, dim3(1), dim3(64), 0, s, (const g1_jac*)a.sums, a.ab, a.ab + 1);
  return 0;
}

}  // namespace CAP_VK_NS
}  // namespace cap
