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
#define CAP_TD_NO_KERNELS
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "context.hpp"
#include "curve29.hpp"
#include "launch.hpp"
#include "pairing29.hpp"
#include "pairing_wave.hpp"
#include "proof_codec.hpp"
#include "srs_check.hpp"
#include "verify_launch.hpp"

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

// enqueues `count` checks whose G1 inputs are already on the device; verdicts to d_ok (device)
int launch_checks(const g1_affine* d_p, const g1_affine* d_r, size_t count, const p29::line_coeffs* l1,
                  const p29::line_coeffs* l2, int* d_ok, hipStream_t s, int form) {
  if (form == CAPGPU_PAIRING_WAVE)
    launch("k_pairing_check2_wave", k_pairing_check2_wave,
           dim3((unsigned)((count + pw::kGroupsPerWave - 1) / pw::kGroupsPerWave)), dim3(64), 0, s, d_p, d_r,
           (uint32_t)count, l1, l2, d_ok);
  else
    launch("k_pairing_check2", k_pairing_check2, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, d_p, d_r,
           (uint32_t)count, l1, l2, d_ok);
  return take_launch_error();
}

// verdicts of `count` checks whose G1 inputs are already on the device
int run_checks(const g1_affine* d_p, const g1_affine* d_r, size_t count, const Lines& L, int* ok_host, hipStream_t s,
               int form) {
  DevTmp<int> d_ok;
  CAP_HIP(d_ok.alloc(count));
  int rc = launch_checks(d_p, d_r, count, L.d1.p, L.d2.p, d_ok.p, s, form);
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

// ---- the block verifier: front end, weights, fold, two one-shot MSMs, one check (K13) -----------------------------------
// capgpu_plonk_verify_block_dev / _resident: everything from the proofs' bytes to the verdicts is enqueued on the
// context's stream and the host waits once.  verify_front.hpp has the term order and the weight rule, verify_kernels.hpp
// the kernels up to the two sums, verify_launch.hpp their launch sequence (tests/hip/verifycheck.hip runs the same).
using vk::own_point_offset;
// The unweighted terms of every proof for k_verify_terms: one thread per (proof, term); scalars as canonical integers
__global__ __launch_bounds__(64) void k_verify_each_terms(const uint8_t* __restrict__ proofs,
                                                          const vf::DevVk* const* __restrict__ keys,
                                                          const uint32_t* __restrict__ meta, const fe* __restrict__ sc,
                                                          const int* __restrict__ valid, uint32_t count,
                                                          g1_affine* __restrict__ pts, fe* __restrict__ out,
                                                          uint32_t* __restrict__ first, uint32_t* __restrict__ na) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if (g >= count * vf::kTerms) return;
  const uint32_t i = g / vf::kTerms, t = g % vf::kTerms;
  g1_affine pt;
  fe s = Fr::zero();
  pt.x = Fq::zero();
  pt.y = Fq::zero();
  if (valid[i]) {
    pt = t < vf::kOwnTerms ? *(const g1_affine*)(proofs + (size_t)i * td::kPrBytes + own_point_offset(t))
                           : keys[meta[4 * i]]->pts[t - vf::kOwnTerms];
    s = Fr::from_mont(sc[g]);
  }
  pts[g] = pt;
  out[g] = s;
  if (t == 0) {
    first[i] = g;
    na[i] = vf::kATerms;
    if (i == count - 1) first[count] = count * vf::kTerms;
  }
}
// out[0] = the block's check and every proof valid; out[1 + i] = proof i's check and its flag (each_ok null: out[0] only)
__global__ __launch_bounds__(64) void k_verify_verdicts(const int* __restrict__ valid, const int* __restrict__ block_ok,
                                                        const int* __restrict__ each_ok, uint32_t count,
                                                        int* __restrict__ out) {
  bool all = true;
  for (uint32_t i = threadIdx.x; i < count; i += 64) {
    const bool v = valid[i] != 0;
    all = all && v;
    if (each_ok) out[1 + i] = (v && each_ok[i]) ? 1 : 0;
  }
  const bool every = __syncthreads_and(all) != 0;
  if (threadIdx.x == 0) out[0] = (every && block_ok[0]) ? 1 : 0;
}

// ---- uploaded verifying keys --------------------------------------------------------------------------------------------
struct VkRecord {
  vf::DevVk host;
  std::mutex mu;
  std::map<int, vf::DevVk*> dev;  // context slot -> replica
  void drop_replicas() {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& kv : dev) (void)hipFree(kv.second);
    dev.clear();
  }
  ~VkRecord() { drop_replicas(); }
};
std::mutex g_vk_mu;
std::map<uint64_t, std::shared_ptr<VkRecord>> g_vks;
std::atomic<uint64_t> g_block_calls{0}, g_block_waits{0};

// the key's table on context c, copied there on first use
int vk_on_context(VkRecord& r, Context& c, const vf::DevVk** out) {
  std::lock_guard<std::mutex> lk(r.mu);
  auto it = r.dev.find(c.slot);
  if (it == r.dev.end()) {
    vf::DevVk* d = nullptr;
    CAP_HIP(hipMalloc(&d, sizeof(vf::DevVk)));
    hipError_t e = hipMemcpyAsync(d, &r.host, sizeof(vf::DevVk), hipMemcpyHostToDevice, c.stream);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return hip_fail(e, "hipMemcpyAsync(verifying key)");
    }
    it = r.dev.emplace(c.slot, d).first;
  }
  *out = it->second;
  return CAPGPU_OK;
}

// the prepared lines of the last (beta_h, h) a context saw, by value
struct LinesCache {
  uint64_t words[32];
  Lines L;
};
std::mutex g_lines_mu;
std::map<int, std::unique_ptr<LinesCache>> g_lines;
int lines_on_context(Context& c, const uint64_t g2_h[16], const uint64_t g2_beta_h[16], const pairing::g2_affine& h,
                     const pairing::g2_affine& beta_h, const Lines** out) {
  std::lock_guard<std::mutex> lk(g_lines_mu);
  std::unique_ptr<LinesCache>& e = g_lines[c.slot];
  if (!e || memcmp(e->words, g2_beta_h, 128) || memcmp(e->words + 16, g2_h, 128)) {
    std::unique_ptr<LinesCache> fresh(new LinesCache);
    memcpy(fresh->words, g2_beta_h, 128);
    memcpy(fresh->words + 16, g2_h, 128);
    int rc = upload_lines(beta_h, h, &fresh->L, c.stream);
    if (rc) return rc;
    if (e) CAP_HIP(hipStreamSynchronize(c.stream));  // nothing enqueued may still read the tables about to go
    e = std::move(fresh);
  }
  *out = &e->L;
  return CAPGPU_OK;
}

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// body of the four entry points.  resident: pub_inputs and proofs are device memory.  byte_stride != 0: `proofs` are wire
// records (proof_codec.hpp) that far apart, decoded into the workspace first; decode_status_out: NULL or their statuses
int verify_block(const char* who, const uint64_t* vk_handles, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                 const uint64_t* pub_inputs, size_t num_inputs, const void* proofs, const uint8_t* const* ext_msgs,
                 const size_t* ext_msg_lens, size_t count, int* block_ok_out, int* each_ok_out, bool resident,
                 size_t byte_stride = 0, int* decode_status_out = nullptr) {
  if (!block_ok_out || !g2_h || !g2_beta_h || (count && (!vk_handles || !proofs)) || count > ((size_t)1 << 24)) {
    set_error("%s: bad argument (null pointer, or more than 2^24 proofs)", who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  *block_ok_out = 0;
  pairing::g2_affine h, beta_h;
  int rc = open_key_from_abi(g2_h, g2_beta_h, &h, &beta_h);
  if (rc) return rc;
  // the call's keys, each once, in order of first appearance
  std::vector<std::shared_ptr<VkRecord>> recs;
  std::vector<uint32_t> meta(4 * count, 0);
  size_t msg_bytes = 0, max_msg = 0;
  {
    std::map<uint64_t, uint32_t> seen;
    std::lock_guard<std::mutex> lk(g_vk_mu);
    for (size_t i = 0; i < count; i++) {
      auto s = seen.find(vk_handles[i]);
      if (s == seen.end()) {
        auto it = g_vks.find(vk_handles[i]);
        if (it == g_vks.end()) {
          set_error("%s: proof %zu names the unknown verifying-key handle %llu", who, i, (unsigned long long)vk_handles[i]);
          return CAPGPU_ERR_INVALID_ARG;
        }
        s = seen.emplace(vk_handles[i], (uint32_t)recs.size()).first;
        recs.push_back(it->second);
      }
      meta[4 * i] = s->second;
    }
  }
  for (const auto& r : recs)
    if (r->host.num_inputs > num_inputs) {
      set_error("%s: rows of %zu public inputs, a key expects %u", who, num_inputs, r->host.num_inputs);
      return CAPGPU_ERR_INVALID_ARG;
    }
  if (count && num_inputs && !pub_inputs) {
    set_error("%s: bad argument (no public inputs)", who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  for (size_t i = 0; i < count; i++) {
    const size_t len = (ext_msgs && ext_msg_lens && ext_msgs[i]) ? ext_msg_lens[i] : 0;
    if (len > ((size_t)1 << 20)) {
      set_error("%s: message %zu has %zu bytes (the limit is 2^20)", who, i, len);
      return CAPGPU_ERR_INVALID_ARG;
    }
    meta[4 * i + 1] = (uint32_t)msg_bytes;
    meta[4 * i + 2] = (uint32_t)len;
    msg_bytes += len;
    max_msg = std::max(max_msg, len);
  }
  if (msg_bytes >= ((size_t)1 << 31)) {
    set_error("%s: %zu message bytes in one call (the limit is 2^31 - 1)", who, msg_bytes);
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  if (count == 0) {
    *block_ok_out = 1;
    return CAPGPU_OK;
  }
  std::vector<uint8_t> msgs(msg_bytes ? msg_bytes : 1);
  for (size_t i = 0; i < count; i++)
    if (meta[4 * i + 2]) memcpy(&msgs[meta[4 * i + 1]], ext_msgs[i], meta[4 * i + 2]);

  Context& c = ctx();
  Entry lk(c);
  const Lines* L = nullptr;
  rc = lines_on_context(c, g2_h, g2_beta_h, h, beta_h, &L);
  if (rc) return rc;
  const size_t nkeys = recs.size();
  std::vector<const vf::DevVk*> keytab(nkeys);
  for (size_t k = 0; k < nkeys; k++)
    if ((rc = vk_on_context(*recs[k], c, &keytab[k]))) return rc;

  // the workspace, carved out of the context's staging scratch
  const size_t pre_stride = (max_msg + vf::kPrefixBytes + 32 * num_inputs + 15) / 16 * 16;
  const size_t msm_pts = vf::kOwnTerms * count + vf::kKeyTerms * nkeys, each_pts = each_ok_out ? vf::kTerms * count : 0;
  size_t at = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = at;
    at += up256(bytes ? bytes : 1);
    return o;
  };
  const bool from_bytes = byte_stride != 0;
  const size_t o_proofs = carve(resident || from_bytes ? 0 : sizeof(capgpu_proof) * count),
               o_pubs = carve(resident ? 0 : sizeof(fe) * num_inputs * count), o_meta = carve(16 * count),
               o_msgs = carve(msg_bytes), o_keys = carve(sizeof(void*) * nkeys), o_state = carve(64 * count),
               o_pre = carve(pre_stride * count), o_app = carve((size_t)vf::kAppBytes * count), o_ub = carve(32 * count),
               o_seed = carve(32), o_valid = carve(sizeof(int) * count), o_sc = carve(sizeof(fe) * vf::kTerms * count),
               o_w = carve(sizeof(fe) * count), o_mpts = carve(sizeof(g1_affine) * msm_pts),
               o_msc = carve(sizeof(fe) * msm_pts), o_desc = carve(sizeof(MsmVarDesc) * 2), o_sums = carve(sizeof(g1_jac) * 2),
               o_ab = carve(sizeof(g1_affine) * 2), o_bok = carve(sizeof(int)), o_epts = carve(sizeof(g1_affine) * each_pts),
               o_esc = carve(sizeof(fe) * each_pts), o_first = carve(sizeof(uint32_t) * (count + 1)),
               o_na = carve(sizeof(uint32_t) * count), o_ea = carve(each_ok_out ? sizeof(g1_affine) * count : 0),
               o_enb = carve(each_ok_out ? sizeof(g1_affine) * count : 0), o_eok = carve(sizeof(int) * count),
               o_out = carve(sizeof(int) * (count + 1));
  // from bytes: the records (a host caller's), the structs they decode to and their statuses
  const size_t rec_bytes = from_bytes ? (count - 1) * byte_stride + pc::kBytes : 0;
  const size_t o_rec = from_bytes && !resident ? carve(rec_bytes) : 0,
               o_dec = from_bytes ? carve(sizeof(capgpu_proof) * count) : 0,
               o_dst = from_bytes ? carve(sizeof(int) * count) : 0;
  const MsmVarDesc desc[2] = {{0, 0, (uint32_t)(vf::kATerms * count)},
                              {(uint64_t)(vf::kATerms * count), (uint32_t)(vf::kATerms * count),
                               (uint32_t)(msm_pts - vf::kATerms * count)}};
  const MsmVarPlan pl = msm_var_plan(desc[1].n, msm_pts, 2);
  if ((rc = scratch_reserve(c.stage_a, at))) return rc;
  if ((rc = scratch_reserve(c.msm_ws, pl.workspace_bytes))) return rc;
  char* d = (char*)c.stage_a.p;
  hipStream_t s = c.stream;
  const uint8_t* d_proofs = from_bytes ? (const uint8_t*)(d + o_dec)
                                       : (resident ? (const uint8_t*)proofs : (const uint8_t*)(d + o_proofs));
  const fe* d_pubs = resident ? (const fe*)pub_inputs : (const fe*)(d + o_pubs);
  if (!resident) {
    if (from_bytes) CAP_HIP(hipMemcpyAsync(d + o_rec, proofs, rec_bytes, hipMemcpyHostToDevice, s));
    else CAP_HIP(hipMemcpyAsync(d + o_proofs, proofs, sizeof(capgpu_proof) * count, hipMemcpyHostToDevice, s));
    if (num_inputs) CAP_HIP(hipMemcpyAsync(d + o_pubs, pub_inputs, sizeof(fe) * num_inputs * count, hipMemcpyHostToDevice, s));
  }
  CAP_HIP(hipMemcpyAsync(d + o_meta, meta.data(), 16 * count, hipMemcpyHostToDevice, s));
  if (msg_bytes) CAP_HIP(hipMemcpyAsync(d + o_msgs, msgs.data(), msg_bytes, hipMemcpyHostToDevice, s));
  CAP_HIP(hipMemcpyAsync(d + o_keys, keytab.data(), sizeof(void*) * nkeys, hipMemcpyHostToDevice, s));
  CAP_HIP(hipMemcpyAsync(d + o_desc, desc, sizeof desc, hipMemcpyHostToDevice, s));

  if (from_bytes &&
      (rc = pc::decode_launch(resident ? (const uint8_t*)proofs : (const uint8_t*)(d + o_rec), byte_stride, count, d + o_dec,
                              (int*)(d + o_dst), s)))
    return rc;
  const uint32_t n = (uint32_t)count;
  const vf::DevVk* const* d_keys = (const vf::DevVk* const*)(d + o_keys);
  const uint32_t* d_meta = (const uint32_t*)(d + o_meta);
  int* d_valid = (int*)(d + o_valid);
  fe *d_sc = (fe*)(d + o_sc), *d_w = (fe*)(d + o_w), *d_msc = (fe*)(d + o_msc);
  g1_affine *d_mpts = (g1_affine*)(d + o_mpts), *d_ab = (g1_affine*)(d + o_ab);
  const vk::FrontArgs fa{d_proofs, d_pubs, d_keys, d_meta, (const uint8_t*)(d + o_msgs), (uint8_t*)(d + o_state),
                         (uint8_t*)(d + o_pre), (uint8_t*)(d + o_app), (uint8_t*)(d + o_ub), d_valid, d_sc,
                         (uint32_t)num_inputs, (uint32_t)pre_stride, n};
  const vk::FoldArgs fold{fa, (uint32_t)nkeys, (uint8_t*)(d + o_seed), d_w, d_mpts, d_msc, (const MsmVarDesc*)(d + o_desc),
                          (g1_jac*)(d + o_sums), c.msm_ws.p, c.msm_ws.cap, d_ab};
  const int msm_rc = vk::fold_launch(fold, s);  // k_verify_front .. k_verify_affine (verify_launch.hpp)
  if ((rc = take_launch_error())) return rc;
  if (msm_rc) return hip_fail((hipError_t)msm_rc, "msm_var_run");
  if ((rc = launch_checks(d_ab, d_ab + 1, 1, L->d1.p, L->d2.p, (int*)(d + o_bok), s, CAPGPU_PAIRING_WAVE))) return rc;
  int form = CAPGPU_PAIRING_WAVE;
  if (each_ok_out) {
    form = current_form();
    launch("k_verify_each_terms", k_verify_each_terms, dim3((n * vf::kTerms + 63) / 64), dim3(64), 0, s, d_proofs, d_keys,
           d_meta, (const fe*)d_sc, (const int*)d_valid, n, (g1_affine*)(d + o_epts), (fe*)(d + o_esc),
           (uint32_t*)(d + o_first), (uint32_t*)(d + o_na));
    launch("k_verify_terms", k_verify_terms, dim3(n), dim3(kTermLanes), 0, s, (const g1_affine*)(d + o_epts),
           (const fe*)(d + o_esc), (const uint32_t*)(d + o_first), (const uint32_t*)(d + o_na), (g1_affine*)(d + o_ea),
           (g1_affine*)(d + o_enb));
    if ((rc = take_launch_error())) return rc;
    if ((rc = launch_checks((const g1_affine*)(d + o_ea), (const g1_affine*)(d + o_enb), count, L->d1.p, L->d2.p,
                            (int*)(d + o_eok), s, form)))
      return rc;
  }
  launch("k_verify_verdicts", k_verify_verdicts, dim3(1), dim3(64), 0, s, (const int*)d_valid, (const int*)(d + o_bok),
         each_ok_out ? (const int*)(d + o_eok) : (const int*)nullptr, n, (int*)(d + o_out));
  if ((rc = take_launch_error())) return rc;
  std::vector<int> out(each_ok_out ? count + 1 : 1);
  CAP_HIP(hipMemcpyAsync(out.data(), d + o_out, sizeof(int) * out.size(), hipMemcpyDeviceToHost, s));
  if (decode_status_out) CAP_HIP(hipMemcpyAsync(decode_status_out, d + o_dst, sizeof(int) * count, hipMemcpyDeviceToHost, s));
  g_block_calls.fetch_add(1, std::memory_order_relaxed);
  g_block_waits.fetch_add(1, std::memory_order_relaxed);
  CAP_HIP(hipStreamSynchronize(s));  // the call's one wait (also keeps the host arrays above alive until the copies are done)
  g_wave_checks.fetch_add(1, std::memory_order_relaxed);
  if (each_ok_out) (form == CAPGPU_PAIRING_WAVE ? g_wave_checks : g_lane_checks).fetch_add(count, std::memory_order_relaxed);
  *block_ok_out = out[0];
  if (each_ok_out) memcpy(each_ok_out, out.data() + 1, sizeof(int) * count);
  return CAPGPU_OK;
}

// ---- capgpu_srs_check (srs_check.hpp: the rule, the point kernel, the soundness argument) -------------------------------
// r_i = vf::weight_bits(seed, i), one wavefront per weight, written as canonical integers (what the MSM takes); all zero
// once the point pass has reported a fault: the fold that follows then touches no point (the sort skips zero digits)
__global__ __launch_bounds__(64) void k_srs_weights(const uint8_t* __restrict__ seed, uint32_t count,
                                                    const unsigned long long* __restrict__ fault, fe* __restrict__ w) {
  __shared__ uint8_t idx8[8], dig[32];
  td::KeccakTabs<td::LaneDev> tabs;
  tabs.init();
  const bool clean = fault[0] == sc::kNoIndex;
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {  // (uniform per block: every lane takes part in the sponge)
    const fe r = vf::weight_bits<td::LaneDev>(seed, i, tabs, idx8, dig);
    if (threadIdx.x == 0) w[i] = clean ? r : Fr::zero();
  }
}
// the two folds to affine form: out[0] = A, out[1] = B, out[2] = -B (what the check takes)
__global__ __launch_bounds__(64) void k_srs_affine(const g1_jac* __restrict__ sums, g1_affine* __restrict__ out) {
  if (blockIdx.x || threadIdx.x) return;
  const g1_jac in[2] = {sums[0], sums[1]};
  g1_affine o[2];
  td::to_affine(in, 2, o);
  out[0] = o[0];
  out[1] = o[1];
  if (!G1::is_inf(o[1])) o[1].y = Fq::neg(o[1].y);
  out[2] = o[1];
}

struct SrsDeviceOut {  // what one fold hands back: the point pass's two words, the check's verdict, A and B
  unsigned long long fault[2];
  int ok, pad;
  g1_affine ab[3];
};

int srs_check(uint64_t srs_handle, const uint64_t g2_h[16], const uint64_t g2_beta_h[16], const uint8_t* seed,
              uint32_t flags, capgpu_srs_report* out) {
  if (!out || !g2_h || !g2_beta_h || (flags & ~CAPGPU_SRS_CHECK_LOCATE)) {
    set_error("capgpu_srs_check: bad argument (null pointer, or flag bits other than CAPGPU_SRS_CHECK_LOCATE)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  memset(out, 0, sizeof *out);
  out->first_bad_point = out->first_bad_link = UINT64_MAX;
  pairing::g2_affine h, beta_h;
  int rc = open_key_from_abi(g2_h, g2_beta_h, &h, &beta_h);
  if (rc) return rc;
  CAP_CHECK_INIT();
  SrsRecord rec;
  if ((rc = srs_record(srs_handle, &rec))) return rc;
  if (rec.sharded()) {
    set_error("capgpu_srs_check: SRS %llu is sharded by point range over the devices of this process; the check runs on "
              "one device's table", (unsigned long long)srs_handle);
    return CAPGPU_ERR_INVALID_ARG;
  }
  uint8_t seed_bytes[32];
  if (seed) {
    memcpy(seed_bytes, seed, 32);
  } else if (getentropy(seed_bytes, 32) != 0) {
    set_error("capgpu_srs_check: the operating system gave no random seed (getentropy)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  Context& c = ctx();
  Entry lk(c);
  const MsmBases* B = nullptr;
  if ((rc = find_srs(srs_handle, &B))) return rc;
  const size_t n = B->n, links = n ? n - 1 : 0;
  out->points_checked = n;
  if (n == 0) return CAPGPU_OK;
  if (links >= ((size_t)1 << 31)) {
    set_error("capgpu_srs_check: %zu points (the limit is 2^31)", n);
    return CAPGPU_ERR_INVALID_ARG;
  }
  const Lines* L = nullptr;
  if (links && (rc = lines_on_context(c, g2_h, g2_beta_h, h, beta_h, &L))) return rc;

  // workspace: the seed, the device's answer, the two sums, the weights - from the staging scratch; the MSM's own
  size_t at = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = at;
    at += up256(bytes ? bytes : 1);
    return o;
  };
  const size_t o_seed = carve(32), o_out = carve(sizeof(SrsDeviceOut)), o_sums = carve(sizeof(g1_jac) * 2),
               o_w = carve(sizeof(fe) * links);
  if ((rc = scratch_reserve(c.stage_a, at))) return rc;
  if (links && (rc = scratch_reserve(c.msm_ws, msm_workspace_bytes(*B, links, 1)))) return rc;
  char* d = (char*)c.stage_a.p;
  hipStream_t s = c.stream;
  SrsDeviceOut* d_out = (SrsDeviceOut*)(d + o_out);
  g1_jac* d_sums = (g1_jac*)(d + o_sums);
  fe* d_w = (fe*)(d + o_w);
  SrsDeviceOut init, got;
  memset(&init, 0, sizeof init);
  init.fault[0] = init.fault[1] = sc::kNoIndex;
  CAP_HIP(hipMemcpyAsync(d + o_seed, seed_bytes, 32, hipMemcpyHostToDevice, s));
  CAP_HIP(hipMemcpyAsync(d_out, &init, sizeof init, hipMemcpyHostToDevice, s));
  launch("k_srs_points", sc::k_srs_points, dim3((unsigned)((n + sc::kPointThreads - 1) / sc::kPointThreads)),
         dim3(sc::kPointThreads), 0, s, (const g1_affine*)B->ext, (unsigned long long)n, (unsigned long long*)d_out->fault);
  if (links)
    launch("k_srs_weights", k_srs_weights, dim3((unsigned)std::min(links, (size_t)1 << 20)), dim3(64), 0, s,
           (const uint8_t*)(d + o_seed), (uint32_t)links, (const unsigned long long*)d_out->fault, d_w);
  if ((rc = take_launch_error())) return rc;
  // A and B over the first k weights, the check on them, the answer copied back: one wait
  auto fold = [&](size_t k) -> int {
    int r = scratch_reserve(c.msm_ws, msm_workspace_bytes(*B, k, 1));
    if (r) return r;
    for (int side = 0; side < 2; side++)
      if ((r = msm_run(*B, (size_t)side, d_w, 0, 1, 0, k, 1, 0, d_sums + side, c.msm_ws.p, c.msm_ws.cap, s)))
        return hip_fail((hipError_t)r, "msm_run");
    g1_affine* d_ab = (g1_affine*)d_out->ab;
    launch("k_srs_affine", k_srs_affine, dim3(1), dim3(64), 0, s, (const g1_jac*)d_sums, d_ab);
    if ((r = take_launch_error())) return r;
    if ((r = launch_checks(d_ab, d_ab + 2, 1, L->d1.p, L->d2.p, &d_out->ok, s, CAPGPU_PAIRING_WAVE))) return r;
    CAP_HIP(hipMemcpyAsync(&got, d_out, sizeof got, hipMemcpyDeviceToHost, s));
    CAP_HIP(hipStreamSynchronize(s));
    return CAPGPU_OK;
  };
  if (links) {
    if ((rc = fold(links))) return rc;
  } else {
    CAP_HIP(hipMemcpyAsync(&got, d_out, sizeof got, hipMemcpyDeviceToHost, s));
    CAP_HIP(hipStreamSynchronize(s));
  }
  if (got.fault[0] != sc::kNoIndex) {  // (the weights were zeroed: the fold added nothing and its verdict says nothing)
    out->verdict = 1;
    out->first_bad_point = got.fault[0];
    out->point_fault = (uint32_t)(got.fault[1] & 3);
    return CAPGPU_OK;
  }
  out->links_checked = links;
  if (!links) return CAPGPU_OK;
  out->pairing_checks = 1;
  memcpy(out->fold_a, &got.ab[0], 64);
  memcpy(out->fold_b, &got.ab[1], 64);
  if (!got.ok) {
    out->verdict = 2;
    if (flags & CAPGPU_SRS_CHECK_LOCATE) {
      // pass(k): the links below k fold to a pair that pairs up.  pass(0) holds, pass(links) has just failed: the lowest
      // bad link is the largest k with pass(k)
      size_t lo = 0, hi = links;
      while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if ((rc = fold(mid))) return rc;
        out->pairing_checks++;
        (got.ok ? lo : hi) = mid;
      }
      out->first_bad_link = lo;
    }
  }
  g_wave_checks.fetch_add(out->pairing_checks, std::memory_order_relaxed);
  return CAPGPU_OK;
}

}  // namespace
}  // namespace cap

using namespace cap;

extern "C" {

// Is the resident SRS a power sequence under this open key?  (srs_check.hpp; include/capgpu.h has the contract)
int capgpu_srs_check(uint64_t srs_handle, const uint64_t g2_h[16], const uint64_t g2_beta_h[16], const uint8_t seed[32],
                     uint32_t flags, capgpu_srs_report* out) {
  return srs_check(srs_handle, g2_h, g2_beta_h, seed, flags, out);
}

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

// ---- the block verifier (verify_front.hpp; kernels above) ---------------------------------------------------------------
// Checks a key once and keeps it for capgpu_plonk_verify_block_*: needs no device (a context gets its copy on first use)
int capgpu_plonk_vk_upload(const capgpu_verifying_key* vk, uint64_t* vk_handle_out) {
  if (!vk || !vk_handle_out) {
    set_error("capgpu_plonk_vk_upload: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  const uint64_t n = vk->domain_size;
  if (n < 4 || (n & (n - 1)) || n > ((uint64_t)1 << 28)) {
    set_error("capgpu_plonk_vk_upload: domain_size %llu is not a power of two in [4, 2^28]", (unsigned long long)n);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (vk->num_inputs > n) {
    set_error("capgpu_plonk_vk_upload: num_inputs %llu exceeds the domain", (unsigned long long)vk->num_inputs);
    return CAPGPU_ERR_INVALID_ARG;
  }
  auto rec = std::make_shared<VkRecord>();
  const int bad = vf::dev_vk_fill(vk, &rec->host);
  if (bad >= 0 && bad < 5) {
    set_error("capgpu_plonk_vk_upload: k[%d] is not canonical", bad);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (bad >= 5) {
    const bool sel = bad - 5 < 13;
    set_error("capgpu_plonk_vk_upload: %s[%d] is not a canonical point of the curve", sel ? "selector_comms" : "sigma_comms",
              sel ? bad - 5 : bad - 18);
    return CAPGPU_ERR_INVALID_ARG;
  }
  const uint64_t hnd = rt().next_handle.fetch_add(1);
  std::lock_guard<std::mutex> lk(g_vk_mu);
  g_vks[hnd] = rec;
  *vk_handle_out = hnd;
  return CAPGPU_OK;
}
int capgpu_plonk_vk_release(uint64_t vk_handle) {
  std::shared_ptr<VkRecord> rec;  // its device copies go when the last call that uses it has returned
  std::lock_guard<std::mutex> lk(g_vk_mu);
  auto it = g_vks.find(vk_handle);
  if (it == g_vks.end()) {
    set_error("capgpu_plonk_vk_release: unknown verifying-key handle %llu", (unsigned long long)vk_handle);
    return CAPGPU_ERR_INVALID_ARG;
  }
  rec = it->second;
  g_vks.erase(it);
  return CAPGPU_OK;
}
// txn_batch_verify (src/lib.rs:455-529) for a block: transcripts, scalars, group arithmetic and the pairing check on the
// device, one host wait.  *block_ok_out: the predicate of capgpu_plonk_batch_verify; each_ok_out[i]: capgpu_plonk_verify's
int capgpu_plonk_verify_block_dev(const uint64_t* vk_handles, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                                  const uint64_t* pub_inputs, size_t num_inputs, const capgpu_proof* proofs,
                                  const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, size_t count,
                                  int* block_ok_out, int* each_ok_out) {
  return verify_block("capgpu_plonk_verify_block_dev", vk_handles, g2_h, g2_beta_h, pub_inputs, num_inputs, proofs, ext_msgs,
                      ext_msg_lens, count, block_ok_out, each_ok_out, false);
}
int capgpu_plonk_verify_block_resident(const uint64_t* vk_handles, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                                       const void* d_pub_inputs, size_t num_inputs, const void* d_proofs,
                                       const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, size_t count,
                                       int* block_ok_out, int* each_ok_out) {
  return verify_block("capgpu_plonk_verify_block_resident", vk_handles, g2_h, g2_beta_h, (const uint64_t*)d_pub_inputs,
                      num_inputs, (const capgpu_proof*)d_proofs, ext_msgs, ext_msg_lens, count, block_ok_out, each_ok_out,
                      true);
}
// the same two with the proofs as their 769 wire bytes (k_proof_decode in front of the launch sequence, the same one wait)
int capgpu_plonk_verify_block_bytes(const uint64_t* vk_handles, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                                    const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* proof_bytes,
                                    size_t stride, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                    size_t count, int* block_ok_out, int* each_ok_out, int* decode_status_out) {
  if (stride < pc::kBytes) {
    set_error("capgpu_plonk_verify_block_bytes: stride %zu below the %u bytes of a record", stride, pc::kBytes);
    return CAPGPU_ERR_INVALID_ARG;
  }
  return verify_block("capgpu_plonk_verify_block_bytes", vk_handles, g2_h, g2_beta_h, pub_inputs, num_inputs, proof_bytes,
                      ext_msgs, ext_msg_lens, count, block_ok_out, each_ok_out, false, stride, decode_status_out);
}
int capgpu_plonk_verify_block_bytes_resident(const uint64_t* vk_handles, const uint64_t g2_h[16],
                                             const uint64_t g2_beta_h[16], const void* d_pub_inputs, size_t num_inputs,
                                             const void* d_proof_bytes, size_t stride, const uint8_t* const* ext_msgs,
                                             const size_t* ext_msg_lens, size_t count, int* block_ok_out,
                                             int* each_ok_out, int* decode_status_out) {
  if (stride < pc::kBytes) {
    set_error("capgpu_plonk_verify_block_bytes_resident: stride %zu below the %u bytes of a record", stride, pc::kBytes);
    return CAPGPU_ERR_INVALID_ARG;
  }
  return verify_block("capgpu_plonk_verify_block_bytes_resident", vk_handles, g2_h, g2_beta_h,
                      (const uint64_t*)d_pub_inputs, num_inputs, d_proof_bytes, ext_msgs, ext_msg_lens, count, block_ok_out,
                      each_ok_out, true, stride, decode_status_out);
}
int capgpu_verify_sync_stats(uint64_t* block_calls_out, uint64_t* stream_waits_out) {
  if (block_calls_out) *block_calls_out = g_block_calls.load(std::memory_order_relaxed);
  if (stream_waits_out) *stream_waits_out = g_block_waits.load(std::memory_order_relaxed);
  return CAPGPU_OK;
}

}  // extern "C"

// ---- for the batch verifier (verify.hip) ---------------------------------------------------------------------------
namespace cap {
// capgpu_shutdown: the contexts go, and with them what the block verifier keeps on them (uploaded keys stay, on the host)
void verify_block_reset() {
  {
    std::lock_guard<std::mutex> lk(g_vk_mu);
    for (auto& kv : g_vks) kv.second->drop_replicas();
  }
  std::lock_guard<std::mutex> lk(g_lines_mu);
  g_lines.clear();
}
int pairing_form() { return current_form(); }
int pairing_check2_wave_dev(const g1_affine& p, const pairing::g2_affine& q1, const g1_affine& r,
                            const pairing::g2_affine& q2, int* ok_out) {
  CAP_CHECK_INIT();
  return check_pairs(&p, &r, 1, q1, q2, ok_out, CAPGPU_PAIRING_WAVE);
}
}  // namespace cap
