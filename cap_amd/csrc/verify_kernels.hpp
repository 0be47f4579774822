// The block verifier's kernels from the proofs' bytes to the two sums in affine form (K13 of DESIGN.md §4): the front end,
// the seed and the weights, the gather and the fold of the two MSMs' inputs, and the sums to affine form.  They sit in a
// named namespace so that two translation units compile the same text with the same flags: verify_dev.hip, which runs
// them for capgpu_plonk_verify_block_*, and tests/hip/verifycheck.hip, which runs them on chosen inputs and dumps every
// intermediate value (tests/test_gpu_verifycheck.py compares the dump with Python integers).  verify_launch.hpp has the
// launch sequence both use; verify_front.hpp the term order and the weight rule.
// The includer sets CAP_FL_SCHED and CAP_TD_NO_KERNELS as verify_dev.hip does.
//
// CAP_VK_NS names the namespace (vk unless set).  A program that compiles these kernels beside the library sets a name of
// its own: a kernel's handle is an exported symbol, two of one name in a process resolve to one handle, and the code
// object registered first under it - the library's - would be what both launch.
#pragma once
#include "verify_front.hpp"

#ifndef CAP_VK_NS
#define CAP_VK_NS vk
#endif

namespace cap {
namespace CAP_VK_NS {

struct FrontArgs {
  const uint8_t* proofs;          // count x capgpu_proof
  const fe* pubs;                 // count rows of pub_stride
  const vf::DevVk* const* keys;   // the call's keys
  const uint32_t* meta;           // per proof: key index, message offset, message length, 0
  const uint8_t* msgs;
  uint8_t *state, *pre, *app, *ubytes;  // per proof: 64, pre_stride, vf::kAppBytes, 32 bytes
  int* valid;
  fe* sc;                         // count x vf::kTerms
  uint32_t pub_stride, pre_stride, count;
};

// proof p's point of own term t (< vf::kOwnTerms): the 13 points of a capgpu_proof are contiguous
__device__ __forceinline__ uint32_t own_point_offset(uint32_t t) {
  if (t == vf::kTermWzeta || t == vf::kTermBWzeta) return td::kPrOpen;
  if (t == vf::kTermWzetaW || t == vf::kTermBWzetaW) return td::kPrShifted;
  return 64 * (t - vf::kTermWires);  // wires, z, quotient parts in the struct's order
}

// One wavefront per proof: verify.hip's verifier_terms, in its order.  Lanes 0..12 check and compress the proof's points,
// lanes 13..22 its evaluations, all lanes stride over the public inputs, the message and the key's prefix; the wavefront
// draws the seven challenges; the lanes stride over PI(zeta); lane 0 derives the scalars.
__global__ __launch_bounds__(64) void k_verify_front(FrontArgs a) {
  __shared__ fe sh[64];
  const uint32_t p = blockIdx.x, t = threadIdx.x;
  if (p >= a.count) return;
  const uint8_t* pr = a.proofs + (size_t)p * td::kPrBytes;
  const uint32_t moff = a.meta[4 * p + 1], mlen = a.meta[4 * p + 2];
  const vf::DevVk* vk = a.keys[a.meta[4 * p]];
  const uint32_t nin = vk->num_inputs;
  const fe* pubs = a.pubs + (size_t)p * a.pub_stride;
  uint8_t* pre = a.pre + (size_t)p * a.pre_stride;
  uint8_t* app = a.app + (size_t)p * vf::kAppBytes;
  uint8_t* st = a.state + (size_t)p * 64;
  fe* sc = a.sc + (size_t)p * vf::kTerms;
  bool ok = true;
  if (t < 13) {
    const g1_affine pt = *(const g1_affine*)(pr + 64 * t);
    ok = vf::g1_valid(pt);
    td::compress_g1(pt, app + (t < 11 ? 32 * t : 32 * (t + 10)));  // the two openings follow the ten evaluations
  } else if (t < 23) {
    const fe e = *(const fe*)(pr + td::kPrWireEvals + 32 * (t - 13));
    ok = !Fr::geq_mod(e);
    td::serialize_fr(e, app + td::kAppEvals + 32 * (t - 13));
  }
  for (uint32_t j = t; j < nin; j += 64) {
    const fe v = pubs[j];
    ok = ok && !Fr::geq_mod(v);
    td::serialize_fr(v, pre + mlen + vf::kPrefixBytes + 32 * j);
  }
  for (uint32_t k = t; k < mlen; k += 64) pre[k] = a.msgs[moff + k];
  for (uint32_t k = t; k < vf::kPrefixBytes; k += 64) pre[mlen + k] = vk->prefix[k];
  st[t] = 0;
  bool valid = __syncthreads_and(ok) != 0;
  fe beta, gamma, alpha, zeta, v, u, zh;
  if (valid) {
    td::KeccakTabs<td::LaneDev> tabs;
    tabs.init();
    const uint32_t lpre = mlen + vf::kPrefixBytes + 32 * nin;
    auto draw = [&](uint32_t lapp) {
      td::transcript_challenge<td::LaneDev>(st, pre, lpre, app, lapp, tabs);
      return td::reduce48(st);
    };
    (void)draw(td::kAppZ);  // plookup's tau
    beta = draw(td::kAppZ);
    gamma = draw(td::kAppZ);
    alpha = draw(td::kAppQuot);
    zeta = draw(td::kAppEvals);
    v = draw(vf::kAppOpen);
    u = draw(vf::kAppBytes);
    valid = vf::vanishing(zeta, vk->n, &zh);
  }
  if (!valid) {  // uniform: every lane saw the same flags and challenges
    for (uint32_t k = t; k < vf::kTerms; k += 64) sc[k] = Fr::zero();
    if (t < 32) a.ubytes[(size_t)p * 32 + t] = 0;
    if (t == 0) a.valid[p] = 0;
    return;
  }
  sh[t] = vf::pi_partial(pubs, nin, t, 64, zeta, zh, vk->omega, vk->n_mont);
  __syncthreads();
  if (t == 0) {
    fe pi = sh[0];
#pragma unroll 1
    for (int i = 1; i < 64; i++) pi = Fr::add(pi, sh[i]);
    const vf::FrontIn in{(const fe*)(pr + td::kPrWireEvals), vk->k, beta, gamma, alpha, zeta, v, u, vk->omega, vk->n_mont,
                         zh, pi, vk->n};
    vf::front_scalars(in, sc);
    td::serialize_fr(u, a.ubytes + (size_t)p * 32);
    a.valid[p] = 1;
  }
}

// S = Keccak-256 of the block's u bytes: one wavefront
__global__ __launch_bounds__(64) void k_verify_seed(const uint8_t* __restrict__ ubytes, uint32_t count, uint8_t* __restrict__ S) {
  td::KeccakTabs<td::LaneDev> tabs;
  tabs.init();
  vf::weight_seed<td::LaneDev>(ubytes, count, tabs, S);
}
// r_i, one wavefront per proof
__global__ __launch_bounds__(64) void k_verify_weights(const uint8_t* __restrict__ S, uint32_t count, fe* __restrict__ w) {
  __shared__ uint8_t idx8[8], dig[32];
  const uint32_t i = blockIdx.x;
  if (i >= count) return;
  td::KeccakTabs<td::LaneDev> tabs;
  tabs.init();
  const fe r = vf::weight<td::LaneDev>(S, i, tabs, idx8, dig);
  if (threadIdx.x == 0) w[i] = r;
}

// The points and weighted scalars of the two MSMs: A over [0, 2 count), B's own terms over the next 13 count.  One thread
// per (proof, own term).  An invalid proof contributes points at infinity and zero scalars.
__global__ __launch_bounds__(64) void k_verify_gather(const uint8_t* __restrict__ proofs, const fe* __restrict__ sc,
                                                      const fe* __restrict__ w, const int* __restrict__ valid,
                                                      uint32_t count, g1_affine* __restrict__ pts, fe* __restrict__ out) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if (g >= count * vf::kOwnTerms) return;
  const uint32_t i = g / vf::kOwnTerms, t = g % vf::kOwnTerms;
  const uint32_t at = t < vf::kATerms ? vf::kATerms * i + t
                                      : vf::kATerms * count + (vf::kOwnTerms - vf::kATerms) * i + (t - vf::kATerms);
  g1_affine pt;
  fe s = Fr::zero();
  pt.x = Fq::zero();
  pt.y = Fq::zero();
  if (valid[i]) {
    pt = *(const g1_affine*)(proofs + (size_t)i * td::kPrBytes + own_point_offset(t));
    s = Fr::mul(w[i], sc[(size_t)i * vf::kTerms + t]);
  }
  pts[at] = pt;
  out[at] = s;
}
// Block (k, j): sum over the valid proofs i of key k of r_i s_ij for key term j, lanes striding over the proofs; written
// with the key's point behind the own terms of B
__global__ __launch_bounds__(64) void k_verify_fold(const vf::DevVk* const* __restrict__ keys,
                                                    const uint32_t* __restrict__ meta, const fe* __restrict__ sc,
                                                    const fe* __restrict__ w, const int* __restrict__ valid,
                                                    uint32_t count, g1_affine* __restrict__ pts, fe* __restrict__ out) {
  __shared__ fe sh[64];
  const uint32_t k = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
  fe acc = Fr::zero();
  for (uint32_t i = t; i < count; i += 64)
    if (meta[4 * i] == k && valid[i]) acc = Fr::add(acc, Fr::mul(w[i], sc[(size_t)i * vf::kTerms + vf::kOwnTerms + j]));
  sh[t] = acc;
  __syncthreads();
  for (uint32_t s = 32; s >= 1; s >>= 1) {
    if (t < s) sh[t] = Fr::add(sh[t], sh[t + s]);
    __syncthreads();
  }
  if (t == 0) {
    const uint32_t at = vf::kOwnTerms * count + vf::kKeyTerms * k + j;
    pts[at] = keys[k]->pts[j];
    out[at] = sh[0];
  }
}
// the two sums to affine form, B negated: what the check takes
__global__ __launch_bounds__(64) void k_verify_affine(const g1_jac* __restrict__ sums, g1_affine* __restrict__ a_out,
                                                      g1_affine* __restrict__ negb_out) {
  if (blockIdx.x || threadIdx.x) return;
  const g1_jac in[2] = {sums[0], sums[1]};
  g1_affine o[2];
  td::to_affine(in, 2, o);
  if (!G1::is_inf(o[1])) o[1].y = Fq::neg(o[1].y);
  a_out[0] = o[0];
  negb_out[0] = o[1];
}

}  // namespace CAP_VK_NS
}  // namespace cap
