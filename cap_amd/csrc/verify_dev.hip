// Per-proof PLONK verification on the device: one verdict per proof for a whole batch (capgpu_plonk_verify_each_dev), and
// the pairing check it ends in on its own (capgpu_pairing_check_pairs_dev).
//
// capgpu_plonk_batch_verify[_dev] answers yes or no for a whole block (txn_batch_verify, src/lib.rs:455-529); when a
// block fails, the reference finds the bad notes with TransferNote::verify (src/transfer.rs:345-363), one at a time.
// Here the transcripts and scalars stay on the host (verify.hip: batch_terms_each, the host threads of the batch
// verifier) and the group arithmetic of every proof runs on the device:
//   k_verify_terms    one workgroup of 64 per proof, one lane per (proof, term) pair: [s] P by 2-bit windows in XYZZ
//                     (curve29.hpp), the per-proof sums A = sum a-terms, B = sum b-terms by a tree through LDS, then
//                     A and -B in affine form (one Fermat inversion each, lanes 0 and 1).
//   k_pairing_check2  one check per lane: e(P_i, Q1) e(R_i, Q2) == 1 over the prepared lines of Q1 and Q2 (host-made,
//                     pairing29.hpp: prepare_lines), shared squarings, final exponentiation, one verdict.
//   k_pairing_check2_wave  the same contract, one check per group of six lanes (pairing_wave.hpp), ten checks per
//                     wavefront.  One lane's check takes ~22 ms however few there are; a group's chain
//                     is about a quarter as long by operation count and needs no stack (not timed yet).  capgpu_pairing_set_form chooses between the two
//                     (CAPGPU_PAIRING_LANE, the default, or CAPGPU_PAIRING_WAVE); capgpu_plonk_verify_dev - one proof,
//                     the device's counterpart of capgpu_plonk_verify - always takes the wave form.
// A proof holds iff e(A, [tau]H) e(-B, H) == 1 (the predicate of capgpu_plonk_verify): Q1 = beta_h, Q2 = h.
#define CAP_FL_SCHED 0
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "context.hpp"
#include "curve29.hpp"
#include "launch.hpp"
#include "pairing29.hpp"
#include "pairing_wave.hpp"
#include "verify_terms.hpp"

namespace cap {
namespace {

using F = Fq29;
using T = p29::Tower<CAP_FL_SCHED>;
using W = pw::Wave<pw::GroupDev, CAP_FL_SCHED>;
constexpr int kTermLanes = 64;

// [k] P, one out-of-line copy per kernel (curve29.hpp: G1LT::term_mul; tests/hip runs the same function)
__device__ __noinline__ g1x term_mul(const g1a& b, const fe& k) { return G1L::term_mul(b, k); }

__device__ __forceinline__ g1a load_abi(const g1_affine& m) {  // arkworks Montgomery -> internal form; (0, 0) stays
  g1a r;
  r.x = F::from_ext(m.x);
  r.y = F::from_ext(m.y);
  return r;
}

// Block i: the terms [first[i], first[i + 1]) of proof i, the first na[i] of them a-terms.  Lane t takes terms t, t + 64,
// ...; a tree through LDS sums the 64 partial A and B.  Writes A_i and -B_i (arkworks affine form, (0, 0) = infinity).
__global__ __launch_bounds__(kTermLanes) void k_verify_terms(const g1_affine* __restrict__ pts,
                                                             const fe* __restrict__ scalars,
                                                             const uint32_t* __restrict__ first,
                                                             const uint32_t* __restrict__ na,
                                                             g1_affine* __restrict__ a_out,
                                                             g1_affine* __restrict__ negb_out) {
  __shared__ g1x sh[2][kTermLanes];
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  const uint32_t lo = first[i], hi = first[i + 1], split = lo + na[i];
  g1x acc_a = G1L::inf(), acc_b = G1L::inf();
  for (uint32_t k = lo + t; k < hi; k += kTermLanes) {
    const g1x v = term_mul(load_abi(pts[k]), scalars[k]);
    if (k < split) acc_a = G1L::add(acc_a, v);
    else acc_b = G1L::add(acc_b, v);
  }
  sh[0][t] = acc_a;
  sh[1][t] = acc_b;
  __syncthreads();
  for (uint32_t s = kTermLanes / 2; s >= 1; s >>= 1) {
    if (t < s) {
      sh[0][t] = G1L::add(sh[0][t], sh[0][t + s]);
      sh[1][t] = G1L::add(sh[1][t], sh[1][t + s]);
    }
    __syncthreads();
  }
  if (t < 2) {
    const g1x sum = sh[t][0];
    g1_affine o;
    if (G1L::is_inf(sum)) {
      memset(&o, 0, sizeof o);
    } else {
      g1a q = G1L::to_affine(sum);
      if (t == 1) q.y = F::neg(q.y);
      o.x = F::to_ext(q.x);
      o.y = F::to_ext(q.y);
    }
    (t == 0 ? a_out : negb_out)[i] = o;
  }
}

// ok[i] = (e(p[i], Q1) e(r[i], Q2) == 1); p, r in arkworks affine form, (0, 0) = infinity (a factor of 1); a null line
// table stands for Q at infinity (every pair with it is a factor of 1)
__global__ __launch_bounds__(64) void k_pairing_check2(const g1_affine* __restrict__ p, const g1_affine* __restrict__ r,
                                                       uint32_t count, const p29::line_coeffs* __restrict__ l1,
                                                       const p29::line_coeffs* __restrict__ l2, int* __restrict__ ok) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const g1a a = load_abi(p[i]), b = load_abi(r[i]);
  const T::g1_eval e1 = T::eval_point(a.x, a.y, !l1 || G1L::is_inf(a));
  const T::g1_eval e2 = T::eval_point(b.x, b.y, !l2 || G1L::is_inf(b));
  ok[i] = T::check2(l1 ? l1 : l2, e1, l2 ? l2 : l1, e2) ? 1 : 0;
}

// The same verdicts, one check per group of pw::kGroup lanes: group g of block b decides check b * 10 + g.  Groups past
// `count` (and lanes 60..63, which belong to no group) run the same instructions on a pair of points at infinity - the
// loop then multiplies nothing - and write nothing, so every exchange inside a group finds its six lanes active.
__global__ __launch_bounds__(64) void k_pairing_check2_wave(const g1_affine* __restrict__ p,
                                                            const g1_affine* __restrict__ r, uint32_t count,
                                                            const p29::line_coeffs* __restrict__ l1,
                                                            const p29::line_coeffs* __restrict__ l2,
                                                            int* __restrict__ ok) {
  const uint32_t lane = threadIdx.x, g = lane / pw::kGroup;
  const uint32_t i = blockIdx.x * pw::kGroupsPerWave + g;
  const bool live = g < pw::kGroupsPerWave && i < count;
  const uint32_t at = live ? i : 0;  // count >= 1: a valid element for the idle lanes to read
  const g1a a = load_abi(p[at]), b = load_abi(r[at]);
  const T::g1_eval e1 = T::eval_point(a.x, a.y, !live || !l1 || G1L::is_inf(a));
  const T::g1_eval e2 = T::eval_point(b.x, b.y, !live || !l2 || G1L::is_inf(b));
  const bool yes = W::check2(l1 ? l1 : l2, e1, l2 ? l2 : l1, e2);
  if (live && lane == g * pw::kGroup) ok[i] = yes ? 1 : 0;
}

// ---- which kernel decides: process-wide, settable before capgpu_init ---------------------------------------------------
std::atomic<int> g_form{-1};  // -1: not read from the environment yet
std::atomic<uint64_t> g_lane_checks{0}, g_wave_checks{0};
int current_form() {
  int f = g_form.load(std::memory_order_acquire);
  if (f >= 0) return f;
  const char* e = getenv("CAPGPU_PAIRING");
  const int init = (e && !strcmp(e, "wave")) ? CAPGPU_PAIRING_WAVE : CAPGPU_PAIRING_LANE;
  int expect = -1;
  g_form.compare_exchange_strong(expect, init, std::memory_order_acq_rel);
  return g_form.load(std::memory_order_acquire);
}

// the two line tables on the device (null for a point at infinity)
struct Lines {
  DevTmp<p29::line_coeffs> d1, d2;
};
int upload_lines(const pairing::g2_affine& q1, const pairing::g2_affine& q2, Lines* L, hipStream_t s) {
  std::vector<p29::line_coeffs> h(2 * p29::kLines);
  const pairing::g2_affine* qs[2] = {&q1, &q2};
  DevTmp<p29::line_coeffs>* ds[2] = {&L->d1, &L->d2};
  for (int k = 0; k < 2; k++) {
    if (qs[k]->inf) continue;
    p29::prepare_lines(*qs[k], &h[k * p29::kLines]);
    CAP_HIP(ds[k]->alloc(p29::kLines));
    CAP_HIP(hipMemcpyAsync(ds[k]->p, &h[k * p29::kLines], sizeof(p29::line_coeffs) * p29::kLines,
                           hipMemcpyHostToDevice, s));
  }
  return CAPGPU_OK;
}

// verdicts of `count` checks whose G1 inputs are already on the device
int run_checks(const g1_affine* d_p, const g1_affine* d_r, size_t count, const Lines& L, int* ok_host, hipStream_t s,
               int form) {
  DevTmp<int> d_ok;
  CAP_HIP(d_ok.alloc(count));
  if (form == CAPGPU_PAIRING_WAVE)
    launch("k_pairing_check2_wave", k_pairing_check2_wave,
           dim3((unsigned)((count + pw::kGroupsPerWave - 1) / pw::kGroupsPerWave)), dim3(64), 0, s, d_p, d_r,
           (uint32_t)count, (const p29::line_coeffs*)L.d1.p, (const p29::line_coeffs*)L.d2.p, d_ok.p);
  else
    launch("k_pairing_check2", k_pairing_check2, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, d_p, d_r,
           (uint32_t)count, (const p29::line_coeffs*)L.d1.p, (const p29::line_coeffs*)L.d2.p, d_ok.p);
  int rc = take_launch_error();
  if (rc) return rc;
  CAP_HIP(hipMemcpyAsync(ok_host, d_ok.p, sizeof(int) * count, hipMemcpyDeviceToHost, s));
  CAP_HIP(hipStreamSynchronize(s));
  (form == CAPGPU_PAIRING_WAVE ? g_wave_checks : g_lane_checks).fetch_add(count, std::memory_order_relaxed);
  return CAPGPU_OK;
}

// `count` checks on host points: upload, decide, copy the verdicts back
int check_pairs(const g1_affine* p, const g1_affine* r, size_t count, const pairing::g2_affine& Q1,
                const pairing::g2_affine& Q2, int* ok_out, int form) {
  Context& c = ctx();
  Entry lk(c);
  Lines L;
  int rc = upload_lines(Q1, Q2, &L, c.stream);
  if (rc) return rc;
  DevTmp<g1_affine> d_p, d_r;
  CAP_HIP(d_p.alloc(count));
  CAP_HIP(d_r.alloc(count));
  CAP_HIP(hipMemcpyAsync(d_p.p, p, sizeof(g1_affine) * count, hipMemcpyHostToDevice, c.stream));
  CAP_HIP(hipMemcpyAsync(d_r.p, r, sizeof(g1_affine) * count, hipMemcpyHostToDevice, c.stream));
  return run_checks(d_p, d_r, count, L, ok_out, c.stream, form);
}

// the body of capgpu_plonk_verify_each_dev (arguments checked by the caller, count >= 1) with the kernel named
int verify_each(const capgpu_verifying_key* const* vks, const pairing::g2_affine& h, const pairing::g2_affine& beta_h,
                const uint64_t* const* pub_inputs, const size_t* num_inputs, const capgpu_proof* const* proofs,
                const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, size_t count, int* ok_out, int form) {
  std::vector<EachTerms> et;
  int rc = batch_terms_each(vks, pub_inputs, num_inputs, proofs, ext_msgs, ext_msg_lens, count, &et);
  if (rc) return rc;
  // the proofs still in question, their terms flattened: a-terms then b-terms of each
  std::vector<size_t> idx;
  std::vector<uint32_t> first(1, 0), na;
  std::vector<g1_affine> pts;
  std::vector<fe> sc;
  for (size_t i = 0; i < count; i++) {
    ok_out[i] = 0;
    if (!et[i].valid) continue;
    idx.push_back(i);
    na.push_back((uint32_t)et[i].a.size());
    for (const EachTerm& t : et[i].a) pts.push_back(t.p), sc.push_back(t.s);
    for (const EachTerm& t : et[i].b) pts.push_back(t.p), sc.push_back(t.s);
    first.push_back((uint32_t)pts.size());
  }
  const size_t m = idx.size();
  if (m == 0) return CAPGPU_OK;
  Context& c = ctx();
  Entry lk(c);
  Lines L;
  rc = upload_lines(beta_h, h, &L, c.stream);
  if (rc) return rc;
  DevTmp<g1_affine> d_pts, d_a, d_nb;
  DevTmp<fe> d_sc;
  DevTmp<uint32_t> d_first, d_na;
  CAP_HIP(d_pts.alloc(pts.size()));
  CAP_HIP(d_sc.alloc(sc.size()));
  CAP_HIP(d_first.alloc(m + 1));
  CAP_HIP(d_na.alloc(m));
  CAP_HIP(d_a.alloc(m));
  CAP_HIP(d_nb.alloc(m));
  CAP_HIP(hipMemcpyAsync(d_pts.p, pts.data(), sizeof(g1_affine) * pts.size(), hipMemcpyHostToDevice, c.stream));
  CAP_HIP(hipMemcpyAsync(d_sc.p, sc.data(), sizeof(fe) * sc.size(), hipMemcpyHostToDevice, c.stream));
  CAP_HIP(hipMemcpyAsync(d_first.p, first.data(), sizeof(uint32_t) * (m + 1), hipMemcpyHostToDevice, c.stream));
  CAP_HIP(hipMemcpyAsync(d_na.p, na.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice, c.stream));
  launch("k_verify_terms", k_verify_terms, dim3((unsigned)m), dim3(kTermLanes), 0, c.stream, (const g1_affine*)d_pts.p,
         (const fe*)d_sc.p, (const uint32_t*)d_first.p, (const uint32_t*)d_na.p, d_a.p, d_nb.p);
  rc = take_launch_error();
  if (rc) return rc;
  std::vector<int> ok(m, 0);
  rc = run_checks(d_a, d_nb, m, L, ok.data(), c.stream, form);
  if (rc) return rc;
  for (size_t k = 0; k < m; k++) ok_out[idx[k]] = ok[k];
  return CAPGPU_OK;
}

}  // namespace
}  // namespace cap

using namespace cap;

extern "C" {

// ok_out[i] = (e(p_i, q1) e(r_i, q2) == 1): one lane per check under CAPGPU_PAIRING_LANE, one group of six lanes per
// check under CAPGPU_PAIRING_WAVE (capgpu_pairing_set_form)
int capgpu_pairing_check_pairs_dev(const uint64_t* p, const uint64_t* r, size_t count, const uint64_t q1[16],
                                   const uint64_t q2[16], int* ok_out) {
  if ((count && (!p || !r || !ok_out)) || !q1 || !q2) {
    set_error("capgpu_pairing_check_pairs_dev: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  const pairing::g2_affine Q1 = g2_from_abi(q1), Q2 = g2_from_abi(q2);
  if (!pairing::g2_on_curve(Q1) || !pairing::g2_on_curve(Q2)) {
    set_error("capgpu_pairing_check_pairs_dev: q1 or q2 is not on the twist curve");
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (count == 0) return CAPGPU_OK;
  if (count > (1u << 30)) {
    set_error("capgpu_pairing_check_pairs_dev: count %zu too large", count);
    return CAPGPU_ERR_INVALID_ARG;
  }
  for (size_t i = 0; i < count; i++)
    if (!g1_abi_on_curve(g1_from_abi(p + 8 * i)) || !g1_abi_on_curve(g1_from_abi(r + 8 * i))) {
      set_error("capgpu_pairing_check_pairs_dev: input %zu is not on the curve", i);
      return CAPGPU_ERR_INVALID_ARG;
    }
  return check_pairs((const g1_affine*)p, (const g1_affine*)r, count, Q1, Q2, ok_out, current_form());
}

// One verdict per proof: ok_out[i] is what capgpu_plonk_verify gives for proof i
int capgpu_plonk_verify_each_dev(const capgpu_verifying_key* const* vks, const uint64_t g2_h[16],
                                 const uint64_t g2_beta_h[16], const uint64_t* const* pub_inputs,
                                 const size_t* num_inputs, const capgpu_proof* const* proofs,
                                 const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, size_t count,
                                 int* ok_out) {
  if (!g2_h || !g2_beta_h || (count && (!ok_out || !vks || !pub_inputs || !num_inputs || !proofs))) {
    set_error("capgpu_plonk_verify_each_dev: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  pairing::g2_affine h, beta_h;
  int rc = open_key_from_abi(g2_h, g2_beta_h, &h, &beta_h);
  if (rc) return rc;
  if (count == 0) return CAPGPU_OK;
  if (count > (1u << 24)) {
    set_error("capgpu_plonk_verify_each_dev: count %zu too large", count);
    return CAPGPU_ERR_INVALID_ARG;
  }
  return verify_each(vks, h, beta_h, pub_inputs, num_inputs, proofs, ext_msgs, ext_msg_lens, count, ok_out,
                     current_form());
}

// One proof, the device's capgpu_plonk_verify: transcript and terms on the host, the ~35 scalar multiplications and the
// pairing check on the device, the check always in the wave form (one proof is the case it exists for)
int capgpu_plonk_verify_dev(const capgpu_verifying_key* vk, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                            const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len,
                            const capgpu_proof* proof, int* ok_out) {
  if (!vk || !g2_h || !g2_beta_h || !proof || !ok_out || (num_inputs && !pub_inputs)) {
    set_error("capgpu_plonk_verify_dev: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  *ok_out = 0;
  CAP_CHECK_INIT();
  pairing::g2_affine h, beta_h;
  int rc = open_key_from_abi(g2_h, g2_beta_h, &h, &beta_h);
  if (rc) return rc;
  return verify_each(&vk, h, beta_h, &pub_inputs, &num_inputs, &proof, &ext_msg, &ext_msg_len, 1, ok_out,
                     CAPGPU_PAIRING_WAVE);
}

int capgpu_pairing_set_form(int form) {
  if (form != CAPGPU_PAIRING_LANE && form != CAPGPU_PAIRING_WAVE) {
    set_error("capgpu_pairing_set_form: unknown form %d", form);
    return CAPGPU_ERR_INVALID_ARG;
  }
  g_form.store(form, std::memory_order_release);
  return CAPGPU_OK;
}
int capgpu_pairing_get_form(int* form_out) {
  if (!form_out) return CAPGPU_ERR_INVALID_ARG;
  *form_out = current_form();
  return CAPGPU_OK;
}
int capgpu_pairing_stats(uint64_t* lane_checks_out, uint64_t* wave_checks_out) {
  if (lane_checks_out) *lane_checks_out = g_lane_checks.load(std::memory_order_relaxed);
  if (wave_checks_out) *wave_checks_out = g_wave_checks.load(std::memory_order_relaxed);
  return CAPGPU_OK;
}

}  // extern "C"

// ---- for the batch verifier (verify.hip) ---------------------------------------------------------------------------
namespace cap {
int pairing_form() { return current_form(); }
int pairing_check2_wave_dev(const g1_affine& p, const pairing::g2_affine& q1, const g1_affine& r,
                            const pairing::g2_affine& q2, int* ok_out) {
  CAP_CHECK_INIT();
  return check_pairs(&p, &r, 1, q1, q2, ok_out, CAPGPU_PAIRING_WAVE);
}
}  // namespace cap
