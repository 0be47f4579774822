// Proving keys: construction (capgpu_plonk_preprocess*), the key blob, the registry with its per-device replicas, the
// wire -> variable table, key_check and key_info.  No device code: this unit compiles no kernel and launches none - what
// a key needs of the device (transforms, MSMs, the derived tables, the table's permutation) it asks of plonk.hip through
// prover.hpp, so a change here recompiles nothing of the prover's code object.
// field29.hpp reaches this unit through solve.hpp with the header's default CAP_FL_SCHED, not plonk.hip's: the macro
// selects the order in which Fl::mul adds its partial products, not a representation, the unit does no Fl arithmetic,
// and no type it shares with plonk.hip (ProvingKey, SolveSched, sp::Plan, sd::Sched, SolveTables) depends on it.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "context.hpp"
#include "host_util.hpp"
#include "params.hpp"
#include "plonk_key.hpp"
#include "prover.hpp"

namespace cap {

using namespace ks;

// ---- proving-key construction shared by preprocess and the blob loader -------------------------------------
static int key_init(ProvingKey& K, size_t n, size_t num_inputs, uint64_t srs_handle) {
  K.n = n;
  K.m = 6 * n;  // quotient domain: 3 * 2^(log n + 1) points
  K.ps = n + 8;
  while (((size_t)1 << K.log_n) < n) K.log_n++;
  K.log_m = K.log_n + 1;  // log2 of the power-of-two factor of m
  if (K.log_m > 25) {
    set_error("capgpu_plonk_preprocess: domain too large");
    return CAPGPU_ERR_INVALID_ARG;
  }
  K.num_inputs = num_inputs;
  K.srs_handle = srs_handle;
  K.device = ctx().device;
  K.recompute = env_int("CAPGPU_RECOMPUTE_PK_COSET", 0) != 0;
  CAP_HIP(hipMalloc(&K.coef, sizeof(fe) * 18 * K.ps));
  CAP_HIP(hipMalloc(&K.sig_eval, sizeof(fe) * NW * n));
  CAP_HIP(hipMalloc(&K.inv_nx1, sizeof(fe) * K.m));
  return CAPGPU_OK;
}

// verifying key and transcript prefix from the 18 affine commitments (13 selectors, then 5 sigmas)
static void key_set_vk(ProvingKey& K, const std::vector<g1_affine>& ha) {
  memset(&K.vk, 0, sizeof(K.vk));
  K.vk.domain_size = K.n;
  K.vk.num_inputs = K.num_inputs;
  for (int i = 0; i < NW; i++) fe_to_words(K.qc.k[i], K.vk.k[i]);
  for (int i = 0; i < NS; i++) affine_to_words(ha[i], K.vk.selector_comms[i]);
  for (int i = 0; i < NW; i++) affine_to_words(ha[NS + i], K.vk.sigma_comms[i]);
  // transcript prefix: field bits, domain size, #inputs, k_i, selector and sigma commitments
  SolidityTranscript t;
  t.append_u64_le(254);
  t.append_u64_le((uint64_t)K.n);
  t.append_u64_le((uint64_t)K.num_inputs);
  for (int i = 0; i < NW; i++) append_fr(t, K.qc.k[i]);
  for (int i = 0; i < 18; i++) append_g1(t, ha[i]);
  K.vk_bytes = t.buf;
}

// ---- the registry ------------------------------------------------------------------------------------------------------
// the registry's (home) copy of a key, without replicating it
int home_key(uint64_t h, std::shared_ptr<ProvingKey>* out) {
  Runtime& R = rt();
  std::lock_guard<std::mutex> lk(R.mu);
  auto it = R.keys.find(h);
  if (it == R.keys.end()) {
    set_error("capgpu: unknown proving key handle %llu", (unsigned long long)h);
    return CAPGPU_ERR_BAD_HANDLE;
  }
  *out = it->second;
  return CAPGPU_OK;
}

int clone_key_to_current(const ProvingKey& src, int src_device, std::shared_ptr<ProvingKey>* out) {
  Context& c = ctx();
  auto K = std::make_shared<ProvingKey>();
  K->n = src.n;
  K->m = src.m;
  K->ps = src.ps;
  K->log_n = src.log_n;
  K->log_m = src.log_m;
  K->num_inputs = src.num_inputs;
  K->srs_handle = src.srs_handle;
  K->qc = src.qc;
  K->qc29 = src.qc29;
  K->vk = src.vk;
  K->vk_bytes = src.vk_bytes;
  K->recompute = src.recompute;
  K->device = c.device;
  auto dup = [&](fe** dst, const fe* from, size_t count) -> int {
    if (!from) return CAPGPU_OK;
    CAP_HIP(hipMalloc(dst, sizeof(fe) * count));
    CAP_HIP(copy_between(*dst, c.device, from, src_device, sizeof(fe) * count, c.stream));
    return CAPGPU_OK;
  };
  int rc;
  if ((rc = dup(&K->coef, src.coef, 18 * src.ps))) return rc;
  if ((rc = dup(&K->sig_eval, src.sig_eval, (size_t)NW * src.n))) return rc;
  if ((rc = dup(&K->pk_coset, src.pk_coset, kPkcCols * src.m))) return rc;
  if ((rc = dup(&K->inv_nx1, src.inv_nx1, src.m))) return rc;
  {
    // the variable table and, with it, the permutation's index form (4 B x 5 n each) travel with the key
    std::lock_guard<std::mutex> lk(src.chk_mu);
    if (src.wire_vars && src.chk_perm) {
      const size_t bytes = sizeof(uint32_t) * NW * src.n;
      CAP_HIP(hipMalloc(&K->wire_vars, bytes));
      CAP_HIP(hipMalloc(&K->chk_perm, bytes));
      CAP_HIP(copy_between(K->wire_vars, c.device, src.wire_vars, src_device, bytes, c.stream));
      CAP_HIP(copy_between(K->chk_perm, c.device, src.chk_perm, src_device, bytes, c.stream));
      K->num_vars = src.num_vars;
      K->solve = src.solve;  // the host copy; the replica uploads its own tables on its first solve
    }
  }
  CAP_HIP(hipStreamSynchronize(c.stream));
  *out = K;
  return CAPGPU_OK;
}

// the key resident on the current context: replicated from its home on first use (same device: the same object)
int lookup_key(uint64_t h, std::shared_ptr<ProvingKey>* out) {
  Context& c = ctx();
  auto it = c.keys.find(h);
  if (it != c.keys.end()) {
    *out = it->second;
    return CAPGPU_OK;
  }
  std::shared_ptr<ProvingKey> home, rep;
  int rc = home_key(h, &home);
  if (rc) return rc;
  if (home->device == c.device && !force_replicate()) rep = home;
  else if ((rc = clone_key_to_current(*home, home->device, &rep))) return rc;
  else rt().replications++;
  if ((rc = home_key(h, &home))) return rc;  // freed while it was being copied
  c.keys[h] = rep;
  *out = rep;
  return CAPGPU_OK;
}

// The key of a part on the current context.  `home` (tickets only): the reference the ticket took at submission - a key
// freed since then (capgpu_plonk_free_key with the ticket outstanding) is proved from that reference instead of refused.
int part_key(uint64_t h, const std::shared_ptr<ProvingKey>* home, std::shared_ptr<ProvingKey>* out) {
  const int rc = lookup_key(h, out);
  if (rc != CAPGPU_ERR_BAD_HANDLE || !home || !*home) return rc;
  if ((*home)->device == ctx().device) {
    *out = *home;
    return CAPGPU_OK;
  }
  return clone_key_to_current(**home, (*home)->device, out);
}

// first id of the table ([5][n], host) that is not below num_vars: CAPGPU_ERR_INVALID_ARG naming its (wire, row)
static int vars_table_valid(const char* who, const uint32_t* wire_vars, size_t n, size_t num_vars) {
  if (!wire_vars || num_vars < 1 || num_vars > 0xffffffffull) {
    set_error("%s: bad argument (wire_vars: 5 columns of n ids, 1 <= num_vars < 2^32)", who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  for (size_t c = 0; c < (size_t)NW * n; c++)
    if (wire_vars[c] >= num_vars) {
      set_error("%s: wire_vars holds id %u at (wire %zu, row %zu), num_vars is %zu", who, wire_vars[c], c / n, c % n, num_vars);
      return CAPGPU_ERR_INVALID_ARG;
    }
  return CAPGPU_OK;
}

// the forms a key's COLUMNS (selectors, sigmas) come in
static bool bad_column_form(int form) {
  if (form == CAPGPU_INPUT_EVALS || form == CAPGPU_INPUT_COEFFS) return false;
  set_error("capgpu_plonk_preprocess: form %d is neither CAPGPU_INPUT_EVALS (0) nor CAPGPU_INPUT_COEFFS (1)", form);
  return true;
}

// capgpu_plonk_preprocess_ex, or - wire_vars != nullptr: capgpu_plonk_preprocess_vars - the same with the extended
// permutation built on the device from the circuit's wire -> variable table (`sigma_evals` is then unused and
// `input_form` is the selectors' alone); from the sigma values on, one code path finishes both keys.
static int preprocess_impl(uint64_t srs_handle, size_t n, size_t num_inputs, const uint64_t* selectors,
                           const uint64_t* sigma_evals, int input_form, const uint32_t* wire_vars, size_t num_vars,
                           uint64_t* pk_handle_out, capgpu_verifying_key* vk_out) {
  Context& c = ctx();
  Entry lk(c);
  // n >= 16: the five split-quotient commitments read 5 (n + 2) coefficients of the 6n-point quotient array
  if (!selectors || (!sigma_evals && !wire_vars) || !pk_handle_out || n < 16 || (n & (n - 1)) || num_inputs >= n) {
    set_error("capgpu_plonk_preprocess: bad argument (n must be a power of two >= 16, num_inputs < n)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  const MsmBases* B = nullptr;
  int rc = find_srs(srs_handle, &B);
  if (rc) return rc;
  if (B->n < n + 3) {
    set_error("capgpu_plonk_preprocess: SRS holds %zu powers, the circuit needs %zu (n + 3)", B->n, n + 3);
    return CAPGPU_ERR_INVALID_ARG;
  }
  hipStream_t s = c.stream;
  auto K = std::make_shared<ProvingKey>();
  if ((rc = key_init(*K, n, num_inputs, srs_handle))) return rc;
  const size_t ps = K->ps;
  // stage the evaluation columns, then interpolate
  DevTmp<fe> stage;
  DevTmp<g1_jac> d_comms;
  CAP_HIP(stage.alloc(18 * n));
  CAP_HIP(hipMemcpyAsync(stage, selectors, sizeof(fe) * NS * n, hipMemcpyHostToDevice, s));
  if (wire_vars) {
    // the permutation comes from the table, on the device: its index form stays with the key (the witness check needs no
    // discrete logarithm for it), its field form is the sigma VALUES a caller of capgpu_plonk_preprocess would have sent
    CAP_HIP(hipMalloc(&K->wire_vars, sizeof(uint32_t) * NW * n));
    CAP_HIP(hipMalloc(&K->chk_perm, sizeof(uint32_t) * NW * n));
    CAP_HIP(hipMemcpyAsync(K->wire_vars, wire_vars, sizeof(uint32_t) * NW * n, hipMemcpyHostToDevice, s));
    K->num_vars = num_vars;
    if ((rc = vars_build_perm(s, K->wire_vars, n, K->chk_perm))) return rc;
    vars_sigma_values(s, K->log_n, K->chk_perm, stage.p + (size_t)NS * n);
  } else {
    CAP_HIP(hipMemcpyAsync(stage.p + (size_t)NS * n, sigma_evals, sizeof(fe) * NW * n, hipMemcpyHostToDevice, s));
  }
  CAP_HIP(hipMemcpyAsync(K->sig_eval, stage.p + (size_t)NS * n, sizeof(fe) * NW * n, hipMemcpyDeviceToDevice, s));
  pad_columns(s, K->coef, ps, 0, stage.p, n, 0, 1, 18, n, ps);
  if (input_form == CAPGPU_INPUT_COEFFS && wire_vars) {
    // selector polynomials as they are; the table's sigma is VALUES: interpolate those five columns only
    if ((rc = run_ntt(s, K->log_n, K->coef + (size_t)NS * ps, ps, NW, 1, 0))) return rc;
  } else if (input_form == CAPGPU_INPUT_COEFFS) {
    // the 18 polynomials arrive as jf-relation computes them (compute_selector_polynomials /
    // compute_extended_permutation_polynomials): nothing to interpolate; round 2 reads sigma's VALUES on the domain
    if ((rc = run_ntt(s, K->log_n, K->sig_eval, n, NW, 0, 0))) return rc;
  } else if ((rc = run_ntt(s, K->log_n, K->coef, ps, 18, 1, 0))) {
    return rc;
  }
  if ((rc = key_finish_tables(s, *K))) return rc;
  // verifying key: commitments of the 18 polynomials
  CAP_HIP(d_comms.alloc(18));
  if ((rc = run_msm(s, *B, K->coef, ps, 1, 0, n, 18, d_comms))) return rc;
  std::vector<g1_jac> hj(18);
  std::vector<g1_affine> ha;
  CAP_HIP(hipMemcpyAsync(hj.data(), d_comms, sizeof(g1_jac) * 18, hipMemcpyDeviceToHost, s));
  CAP_HIP(hipStreamSynchronize(s));
  batch_to_affine(hj, ha);
  key_set_vk(*K, ha);
  if (vk_out) *vk_out = K->vk;
  // the Lagrange-form commit key of this domain under this SRS (round 1's wire commitments; built once per pair and kept
  // with the SRS): made here so that the first proof does not pay for it
  if (wire_commit_from_evals() && !comm_shard_prover()) {
    const MsmBases* Lag = nullptr;
    // (an optimisation: a key whose Lagrange-form table cannot be built proves from coefficients - see make_plan)
    if ((rc = find_lagrange(srs_handle, K->log_n, &Lag)) == CAPGPU_ERR_BAD_HANDLE) return rc;
    (void)hipGetLastError();
  }
  *pk_handle_out = register_key(K);
  return take_launch_error();
}

}  // namespace cap

using namespace cap;

extern "C" {

int capgpu_plonk_preprocess_ex(uint64_t srs_handle, size_t n, size_t num_inputs, const uint64_t* selectors,
                               const uint64_t* sigma_evals, int input_form, uint64_t* pk_handle_out,
                               capgpu_verifying_key* vk_out) {
  CAP_CHECK_INIT();
  if (bad_column_form(input_form)) return CAPGPU_ERR_INVALID_ARG;
  return preprocess_impl(srs_handle, n, num_inputs, selectors, sigma_evals, input_form, nullptr, 0, pk_handle_out, vk_out);
}

int capgpu_plonk_preprocess_vars(uint64_t srs_handle, size_t n, size_t num_inputs, const uint64_t* selectors,
                                 int selector_form, const uint32_t* wire_vars, size_t num_vars, uint64_t* pk_handle_out,
                                 capgpu_verifying_key* vk_out) {
  CAP_CHECK_INIT();
  if (bad_column_form(selector_form)) return CAPGPU_ERR_INVALID_ARG;
  if (n < 16 || (n & (n - 1))) {
    set_error("capgpu_plonk_preprocess: bad argument (n must be a power of two >= 16, num_inputs < n)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  int rc = vars_table_valid("capgpu_plonk_preprocess_vars", wire_vars, n, num_vars);
  if (rc) return rc;
  return preprocess_impl(srs_handle, n, num_inputs, selectors, nullptr, selector_form, wire_vars, num_vars, pk_handle_out,
                         vk_out);
}

int capgpu_plonk_preprocess(uint64_t srs_handle, size_t n, size_t num_inputs, const uint64_t* selectors,
                            const uint64_t* sigma_evals, uint64_t* pk_handle_out, capgpu_verifying_key* vk_out) {
  return capgpu_plonk_preprocess_ex(srs_handle, n, num_inputs, selectors, sigma_evals, CAPGPU_INPUT_EVALS, pk_handle_out,
                                    vk_out);
}

// ---- ProvingKey blob (layout in include/capgpu.h) ---------------------------------------------
int capgpu_plonk_key_serialize(uint64_t pk_handle, const uint64_t gamma_g[8], const uint64_t h[16],
                               const uint64_t beta_h[16], uint8_t* out, size_t cap, size_t* len_out) {
  CAP_CHECK_INIT();
  Context& c = ctx();
  Entry lk(c);
  if (!h || !beta_h || !len_out) {
    set_error("capgpu_plonk_key_serialize: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  std::shared_ptr<ProvingKey> K;
  int rc = lookup_key(pk_handle, &K);
  if (rc) return rc;
  const MsmBases* B = nullptr;
  if ((rc = find_srs(K->srs_handle, &B))) return rc;
  const size_t n = K->n, ps = K->ps, n_ck = n + 3;
  // upper bound: every polynomial at full length
  const SrsEntry* E0 = find_srs_entry(K->srs_handle);
  const size_t bound = 2 * 8 + 18 * (8 + 32 * n) + 8 + 32 * n_ck + 8 +
                       (E0 ? std::max(E0->ck_gamma_pts.size(), (size_t)32 * n_ck) : 0) + 1024;
  if (!out) {
    *len_out = bound;
    return CAPGPU_OK;
  }
  hipStream_t s = c.stream;
  std::vector<uint8_t> coef(32 * 18 * ps), ck(32 * n_ck);
  if ((rc = params::fr_mont_to_bytes(K->coef, 18 * ps, coef.data(), s))) return rc;
  if ((rc = params::compress_g1(B->ext, 1, n_ck, ck.data(), s))) return rc;
  params::Writer w;
  auto poly = [&](int idx) {  // DensePolynomial: no trailing zero coefficients
    const uint8_t* p = &coef[32 * (size_t)idx * ps];
    size_t len = n;
    auto zero = [&](size_t i) {
      for (int b = 0; b < 32; b++)
        if (p[32 * i + b]) return false;
      return true;
    };
    while (len && zero(len - 1)) len--;
    w.u64(len);
    w.put(p, 32 * len);
  };
  w.u64(NW);
  for (int i = 0; i < NW; i++) poly(NS + i);
  w.u64(NS);
  for (int i = 0; i < NS; i++) poly(i);
  w.u64(n_ck);
  w.put(ck.data(), ck.size());
  {
    // CommitKey::powers_of_gamma_g (Vec<G1>, degrees 0 .. n_ck - 1 - what jf-plonk's trim emits).  A key loaded from a
    // ProvingKey blob re-emits the blob's vector.  A key preprocessed under a loaded UniversalSrs takes the degrees
    // 0 .. n_ck - 1 from that SRS's BTreeMap, in order - all of them or, when one is missing, none (a sparse map must
    // not turn into a shorter vector with the degrees lost).  A synthetic SRS has no hiding powers: empty vector.
    const SrsEntry* E = find_srs_entry(K->srs_handle);
    std::vector<uint8_t> gp;
    if (E && !E->ck_gamma_pts.empty()) {
      gp = E->ck_gamma_pts;
    } else if (E && !E->gamma_deg.empty()) {
      std::map<uint64_t, size_t> at;
      for (size_t i = 0; i < E->gamma_deg.size(); i++) at[E->gamma_deg[i]] = i;
      bool all = true;
      for (uint64_t d = 0; d < n_ck && all; d++) all = at.count(d) != 0;
      if (all)
        for (uint64_t d = 0; d < n_ck; d++)
          gp.insert(gp.end(), E->gamma_pts.begin() + 32 * at[d], E->gamma_pts.begin() + 32 * at[d] + 32);
    }
    w.u64(gp.size() / 32);
    if (!gp.empty()) w.put(gp.data(), gp.size());
  }
  params::OpenKey ok;
  {
    g1_affine g0;
    if (!params::g1_decompress_host(ck.data(), &g0)) return CAPGPU_ERR_SERIALIZATION;
    ok.g = g0;
  }
  // open key's gamma_g: the caller's, else what the blob this key (or its SRS) was loaded from held - the key blob's own
  // value, or degree 0 of a UniversalSrs's hiding powers - else infinity (a synthetic SRS has none)
  ok.gamma_g.x = ok.gamma_g.y = Fq::zero();
  if (gamma_g) {
    ok.gamma_g = params::g1_from_words(gamma_g);
  } else if (const SrsEntry* Eg = find_srs_entry(K->srs_handle)) {
    if (Eg->has_ck_gamma_g) {
      ok.gamma_g = Eg->ck_gamma_g;
    } else {
      for (size_t i = 0; i < Eg->gamma_deg.size(); i++)
        if (Eg->gamma_deg[i] == 0) {
          g1_affine g0;
          if (params::g1_decompress_host(&Eg->gamma_pts[32 * i], &g0)) ok.gamma_g = g0;
          break;
        }
    }
  }
  ok.h = params::g2_from_words(h);
  ok.beta_h = params::g2_from_words(beta_h);
  params::write_vk(w, K->vk, ok);
  w.u8(0);  // plookup_pk = None
  *len_out = w.buf.size();
  if (cap < w.buf.size()) {
    set_error("capgpu_plonk_key_serialize: buffer of %zu bytes, %zu needed", cap, w.buf.size());
    return CAPGPU_ERR_INVALID_ARG;
  }
  memcpy(out, w.buf.data(), w.buf.size());
  return CAPGPU_OK;
}

int capgpu_plonk_key_deserialize(const uint8_t* bytes, size_t len, uint64_t* srs_handle_out, uint64_t* pk_handle_out,
                                 capgpu_verifying_key* vk_out, uint64_t h_out[16], uint64_t beta_h_out[16],
                                 size_t* consumed_out) {
  CAP_CHECK_INIT();
  Context& c = ctx();
  Entry lk(c);
  if (!bytes || !srs_handle_out || !pk_handle_out) {
    set_error("capgpu_plonk_key_deserialize: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  params::Reader rd(bytes, len);
  auto fail = [&](const char* why) {
    set_error("capgpu_plonk_key_deserialize: %s (byte %zu of %zu)", why, rd.pos, len);
    return CAPGPU_ERR_SERIALIZATION;
  };
  struct Span {
    const uint8_t* p;
    uint64_t len;
  };
  Span polys[18];  // internal order: 13 selectors, then 5 sigmas
  uint64_t cnt = 0;
  if (!rd.count(8, &cnt)) return fail("unexpected end of input");
  if (cnt != NW) return fail("sigmas: a TurboPlonk key has 5 of them");
  for (int i = 0; i < NW; i++) {
    if (!rd.count(32, &polys[NS + i].len)) return fail("unexpected end of input");
    polys[NS + i].p = rd.take(32 * polys[NS + i].len);
  }
  if (!rd.count(8, &cnt)) return fail("unexpected end of input");
  if (cnt != NS) return fail("selectors: a TurboPlonk key has 13 of them");
  for (int i = 0; i < NS; i++) {
    if (!rd.count(32, &polys[i].len)) return fail("unexpected end of input");
    polys[i].p = rd.take(32 * polys[i].len);
  }
  uint64_t n_ck = 0, n_gamma = 0;
  if (!rd.count(32, &n_ck)) return fail("unexpected end of input");
  const uint8_t* ck = rd.take(32 * n_ck);
  if (!rd.count(32, &n_gamma)) return fail("unexpected end of input");
  const uint8_t* gamma = rd.take(32 * n_gamma);
  capgpu_verifying_key vk;
  params::OpenKey ok;
  if (const char* why = params::read_vk(rd, &vk, &ok)) return fail(why);
  const uint8_t* tag = rd.take(1);
  if (!tag) return fail("unexpected end of input");
  if (*tag) return fail("plookup proving keys are not supported");
  const size_t n = vk.domain_size;
  if (n < 16 || (n & (n - 1)) || vk.num_inputs >= n)
    return fail("domain_size must be a power of two >= 16 above num_inputs");
  if (n_ck < n + 3) return fail("commit key shorter than domain_size + 3");
  for (int i = 0; i < 18; i++)
    if (polys[i].len > n) return fail("polynomial longer than the domain");
  // the prover's quotient kernel is specialised to the k_i of jf-plonk; refuse anything else
  for (int i = 0; i < NW; i++) {
    uint64_t want[4];
    fe_to_words(Fr::to_mont(fe_from_words(K_CANON[i])), want);
    if (memcmp(want, vk.k[i], 32) != 0) return fail("coset representatives k_i differ from jf-plonk's");
  }

  hipStream_t s = c.stream;
  int rc;
  // commit key -> device -> window table
  uint64_t srs_handle = 0;
  {
    DevTmp<g1_affine> d_ck;
    CAP_HIP(d_ck.alloc(std::max<uint64_t>(n_ck, n_gamma)));
    rc = n_gamma ? params::decompress_g1(gamma, n_gamma, d_ck, s) : CAPGPU_OK;  // validated; bytes kept below
    if (rc == CAPGPU_OK) rc = params::decompress_g1(ck, n_ck, d_ck, s);
    if (rc == CAPGPU_OK) rc = register_srs(d_ck, n_ck, &srs_handle);
    if (rc) return rc;
    if (SrsEntry* E = find_srs_entry(srs_handle)) {
      E->ck_gamma_pts.assign(gamma, gamma + 32 * n_gamma);
      E->ck_gamma_g = ok.gamma_g;
      E->has_ck_gamma_g = true;
    }
  }
  auto K = std::make_shared<ProvingKey>();
  auto bail = [&](int code) {
    // the SRS was registered a moment ago on THIS context and nobody else knows its handle: drop it here (going through
    // capgpu_srs_free would take the other contexts' locks while this one is held - out of lock order)
    (void)hipStreamSynchronize(c.stream);
    c.srs.erase(srs_handle);
    std::lock_guard<std::mutex> rlk(rt().mu);
    rt().srs.erase(srs_handle);
    return code;
  };
  if ((rc = key_init(*K, n, vk.num_inputs, srs_handle))) return bail(rc);
  const size_t ps = K->ps;
  {
    std::vector<uint8_t> coef(32 * 18 * ps, 0);
    for (int i = 0; i < 18; i++)
      if (polys[i].len) memcpy(&coef[32 * (size_t)i * ps], polys[i].p, 32 * polys[i].len);
    if ((rc = params::fr_bytes_to_mont(coef.data(), 18 * ps, K->coef, s))) return bail(rc);
  }
  // sigma evaluations on the domain (round 2 reads them)
  pad_columns(s, K->sig_eval, n, 0, K->coef + (size_t)NS * ps, ps, 0, 1, NW, n, n);
  if ((rc = run_ntt(s, K->log_n, K->sig_eval, n, NW, 0, 0))) return bail(rc);
  if ((rc = key_finish_tables(s, *K))) return bail(rc);
  std::vector<g1_affine> ha(18);
  for (int i = 0; i < NS; i++) ha[i] = params::g1_from_words(vk.selector_comms[i]);
  for (int i = 0; i < NW; i++) ha[NS + i] = params::g1_from_words(vk.sigma_comms[i]);
  key_set_vk(*K, ha);
  CAP_HIP(hipStreamSynchronize(s));
  if (vk_out) *vk_out = K->vk;
  if (h_out) params::g2_to_words(ok.h, h_out);
  if (beta_h_out) params::g2_to_words(ok.beta_h, beta_h_out);
  if (consumed_out) *consumed_out = rd.pos;
  *pk_handle_out = register_key(K);
  *srs_handle_out = srs_handle;
  return CAPGPU_OK;
}

int capgpu_plonk_key_info(uint64_t pk_handle, size_t* domain_size_out, size_t* num_inputs_out,
                          uint64_t* srs_handle_out) {
  CAP_CHECK_INIT();
  std::shared_ptr<ProvingKey> K;
  int rc = home_key(pk_handle, &K);
  if (rc) return rc;
  if (domain_size_out) *domain_size_out = K->n;
  if (num_inputs_out) *num_inputs_out = K->num_inputs;
  if (srs_handle_out) *srs_handle_out = K->srs_handle;
  return CAPGPU_OK;
}

// Does this proving key produce this verifying key?  The 18 commitments preprocess_impl makes, made again from the key's
// resident polynomials and compared with vk's (NULL: the key's own - what capgpu_plonk_key_deserialize took from the blob)
int capgpu_plonk_key_check(uint64_t pk_handle, const capgpu_verifying_key* vk, capgpu_key_report* out) {
  if (!out) {
    set_error("capgpu_plonk_key_check: bad argument (no report)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  memset(out, 0, sizeof *out);
  CAP_CHECK_INIT();
  Context& c = ctx();
  Entry lk(c);
  std::shared_ptr<ProvingKey> K;
  int rc = lookup_key(pk_handle, &K);
  if (rc) return rc;
  const capgpu_verifying_key& want = vk ? *vk : K->vk;
  if (want.domain_size != K->n || want.num_inputs != K->num_inputs || memcmp(want.k, K->vk.k, sizeof want.k)) {
    out->verdict = 1;
    return CAPGPU_OK;
  }
  const MsmBases* B = nullptr;
  if ((rc = find_srs(K->srs_handle, &B))) return rc;
  hipStream_t s = c.stream;
  DevTmp<g1_jac> d_comms;
  CAP_HIP(d_comms.alloc(18));
  if ((rc = run_msm(s, *B, K->coef, K->ps, 1, 0, K->n, 18, d_comms))) return rc;
  std::vector<g1_jac> hj(18);
  std::vector<g1_affine> ha;
  CAP_HIP(hipMemcpyAsync(hj.data(), d_comms, sizeof(g1_jac) * 18, hipMemcpyDeviceToHost, s));
  CAP_HIP(hipStreamSynchronize(s));
  if ((rc = take_launch_error())) return rc;
  batch_to_affine(hj, ha);
  for (int i = 17; i >= 0; i--) {
    uint64_t w[8];
    affine_to_words(ha[i], w);
    if (memcmp(w, i < NS ? want.selector_comms[i] : want.sigma_comms[i - NS], sizeof w)) {
      out->column = (uint32_t)i;
      out->columns_differing++;
    }
  }
  if (out->columns_differing) {
    out->verdict = 2;
    return CAPGPU_OK;
  }
  // the witness check's test of sigma (kept with the key, like the tables that test derives)
  rc = key_check_tables(*K);
  if (rc == CAPGPU_ERR_INVALID_ARG && K->chk_rc == CAPGPU_ERR_INVALID_ARG) {
    out->verdict = 3;
    return CAPGPU_OK;
  }
  return rc;
}

int capgpu_plonk_key_num_vars(uint64_t pk_handle, size_t* num_vars_out) {
  CAP_CHECK_INIT();
  std::shared_ptr<ProvingKey> K;
  int rc = home_key(pk_handle, &K);
  if (rc) return rc;
  if (num_vars_out) *num_vars_out = K->wire_vars ? K->num_vars : 0;
  return CAPGPU_OK;
}

int capgpu_plonk_input_stats(uint64_t* witness_bytes_h2d_out, uint64_t* gather_launches_out) {
  if (witness_bytes_h2d_out) *witness_bytes_h2d_out = g_witness_h2d.load();
  if (gather_launches_out) *gather_launches_out = g_gather_launches.load();
  return CAPGPU_OK;
}

// Attaches a wire -> variable table to a key made without one.  Runs on a context of the key's home device: the table's
// permutation is built there (vars_build_perm) and compared, cell for cell, with the index form of the key's own sigma.
int capgpu_plonk_key_set_vars(uint64_t pk_handle, const uint32_t* wire_vars, size_t num_vars) {
  CAP_CHECK_INIT();
  std::shared_ptr<ProvingKey> K;
  int rc = home_key(pk_handle, &K);
  if (rc) return rc;
  if ((rc = vars_table_valid("capgpu_plonk_key_set_vars", wire_vars, K->n, num_vars))) return rc;
  Runtime& R = rt();
  Context* home = nullptr;
  for (auto& cp : R.ctxs)
    if (cp->device == K->device) {
      home = cp.get();
      break;
    }
  if (!home) {
    set_error("capgpu_plonk_key_set_vars: no context on the key's device %d", K->device);
    return CAPGPU_ERR_BAD_HANDLE;
  }
  uint32_t* replaced = nullptr;  // the table the key had: freed below, behind whatever launch may still read it
  {
    ScopedCtx sc(*home);
    Entry lk(*home);
    hipStream_t s = home->stream;
    const size_t n = K->n, cells = (size_t)NW * n;
    DevTmp<uint32_t> table, perm;
    DevTmp<unsigned long long> first;
    CAP_HIP(table.alloc(cells));
    CAP_HIP(perm.alloc(cells));
    CAP_HIP(first.alloc(1));
    CAP_HIP(hipMemcpyAsync(table, wire_vars, sizeof(uint32_t) * cells, hipMemcpyHostToDevice, s));
    if ((rc = vars_build_perm(s, table, n, perm))) return rc;
    if ((rc = key_check_tables(*K))) return rc;  // the key's own permutation in index form (derived once per key)
    unsigned long long h_first = ~0ull;
    CAP_HIP(hipMemcpyAsync(first, &h_first, sizeof h_first, hipMemcpyHostToDevice, s));
    vars_first_difference(s, perm.p, K->chk_perm, cells, first.p);
    CAP_HIP(hipMemcpyAsync(&h_first, first, sizeof h_first, hipMemcpyDeviceToHost, s));
    CAP_HIP(hipStreamSynchronize(s));
    if ((rc = take_launch_error())) return rc;
    if (h_first != ~0ull) {
      set_error("capgpu_plonk_key_set_vars: the table's permutation is not the key's: first difference at (wire %llu, row "
                "%llu); the key is unchanged", h_first / n, h_first % n);
      return CAPGPU_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> klk(K->chk_mu);
    replaced = K->wire_vars;
    K->wire_vars = table.p;
    K->num_vars = num_vars;
    K->solve.reset();  // the solver's schedule was derived from the table that leaves
    table.p = nullptr;
  }
  // replicas on other devices were cloned without the table (or with the old one): they are made again on next use
  for (auto& cp : R.ctxs) {
    Context& c = *cp;
    ScopedCtx sc(c);
    Entry lk(c);
    auto it = c.keys.find(pk_handle);
    if (it == c.keys.end()) continue;
    if (replaced || it->second.get() != K.get()) (void)hipStreamSynchronize(c.stream);
    if (it->second.get() != K.get()) c.keys.erase(it);
  }
  if (replaced) {
    ScopedCtx sc(*home);
    (void)hipFree(replaced);
  }
  return CAPGPU_OK;
}

int capgpu_plonk_free_key(uint64_t pk_handle) {
  CAP_CHECK_INIT();
  Runtime& R = rt();
  {
    std::lock_guard<std::mutex> lk(R.mu);
    auto it = R.keys.find(pk_handle);
    if (it == R.keys.end()) {
      set_error("capgpu: unknown proving key handle %llu", (unsigned long long)pk_handle);
      return CAPGPU_ERR_BAD_HANDLE;
    }
    R.keys.erase(it);
  }
  // every context that holds the key (or a replica) drains its stream before letting go of the tables
  for (auto& cp : R.ctxs) {
    Context& c = *cp;
    ScopedCtx sc(c);
    Entry lk(c);
    auto it = c.keys.find(pk_handle);
    if (it == c.keys.end()) continue;
    (void)hipStreamSynchronize(c.stream);
    c.keys.erase(it);
  }
  return CAPGPU_OK;
}

}  // extern "C"
