// The prover proper of plonk.hip - a component of that translation unit, like tickets.hpp, coalescer.hpp and
// transcript_dev.hpp, included by it alone (behind the graph cache and the host pool, which it uses): the
// launch wrappers and their scratch sizes, the batch workspace, the mode getters, the helpers of host-resident and
// variable-form input, and the three types a proving call is made of -
//   ProvePlan  every mode decision of a call, made once (make_plan);
//   ProveRun   the steps of a planned call - input, round bodies, results - and the two drivers that order them, each
//              step with the scratch it asks for (`*_needs`) beside it;
//   ProveNeeds what a plan asks of a context's buffers (capgpu_plonk_reserve).
// prove_batch (plonk.hip) validates, plans, checks the witnesses, carves, picks the graph set and calls a driver.
// What plonk_keys.hip and plonk_solver.hip - units without device code - call of this file is declared in prover.hpp and stands outside the
// anonymous namespace: run_ntt, run_msm, pad_columns, wire_commit_from_evals and the two input counters.  Carver, which
// plonk_solver.hip lays its scratch out with too, is prover.hpp's.
#pragma once
#include "check_kernels.hpp"
#include "context.hpp"
#include "host_util.hpp"
#include "launch.hpp"
#include "outcome.hpp"
#include "params.hpp"
#include "plonk_kernels.hpp"
#include "plonk_key.hpp"
#include "prover.hpp"
#include "round_launch.hpp"
#include "transcript_dev.hpp"
#include "vars_kernels.hpp"

namespace cap {
namespace {

// ---- launch helpers (the round kernels' own: round_launch.hpp) ----------------------------------------------------
// Bytes of Context::ntt_scratch the transforms below ask for.  One expression each, shared with the `*_needs` of ProveRun
// (capgpu_plonk_reserve sizes a context ahead from what a proving call WOULD request).
inline size_t ntt_scratch_inplace(size_t stride, size_t count) { return sizeof(fe) * stride * count; }
inline size_t ntt_scratch_from(uint32_t log_n, size_t count) { return (sizeof(fe) << log_n) * count; }
// (forward: count * 3 sub-transforms of M elements; inverse: their outputs and as much again for the passes in between.
// The five-coset forms - `five` - run 2 M + M / 2 per array: forward 2 M for the passes, inverse 2.5 M outputs + 2 M)
inline size_t ntt3_scratch(uint32_t log_mm, size_t count, bool five = false) {
  return five ? (sizeof(fe) << log_mm) / 2 * 9 * count : (sizeof(fe) << log_mm) * 6 * count;
}
// ... of Context::stage_b for `cnt` host-resident witnesses on a domain of n points
inline size_t wires_stage_bytes(size_t cnt, size_t n) { return sizeof(fe) * cnt * NW * n; }

}  // namespace
int run_ntt(hipStream_t s, uint32_t log_n, fe* data, size_t stride, uint32_t count, int dir, int coset) {
  Context& c = ctx();
  const NttDomain* dom = nullptr;
  int rc = get_domain(log_n, &dom);
  if (rc) return rc;
  rc = scratch_reserve(c.ntt_scratch, ntt_scratch_inplace(stride, count));
  if (rc) return rc;
  rc = ntt_run(*dom, c.small, data, (fe*)c.ntt_scratch.p, stride, count, dir, coset, s);
  if (rc) return hip_fail((hipError_t)rc, "ntt_run");
  return CAPGPU_OK;
}
namespace {

// out-of-place form: `count` arrays of src_len elements at src (src_stride apart; zero-extended to the transform
// size inside the kernel) -> transforms at dst (dst_stride apart).  Saves the padded copy an in-place call needs.
// post_scalar (plain inverse transforms only): takes the place of n^-1 (NttIo::post_scalar)
int run_ntt_from(hipStream_t s, uint32_t log_n, const fe* src, size_t src_stride, size_t src_len, fe* dst,
                 size_t dst_stride, uint32_t count, int dir, int coset, const fe* post_scalar = nullptr) {
  Context& c = ctx();
  const NttDomain* dom = nullptr;
  int rc = get_domain(log_n, &dom);
  if (rc) return rc;
  rc = scratch_reserve(c.ntt_scratch, ntt_scratch_from(log_n, count));
  if (rc) return rc;
  NttIo io{};
  io.src = src;
  io.src_outer = src_stride;
  io.src_inner = 0;
  io.src_group = 1;
  io.src_len = src_len;
  io.dst_outer = dst_stride;
  io.dst_inner = 0;
  io.dst_group = 1;
  if (post_scalar) {
    io.has_post_scalar = 1;
    io.post_scalar = *post_scalar;
  }
  rc = ntt_run(*dom, c.small, dst, (fe*)c.ntt_scratch.p, dst_stride, count, dir, coset, s, &io);
  if (rc) return hip_fail((hipError_t)rc, "ntt_run");
  return CAPGPU_OK;
}

// the quotient domain: N = 6n = 3 * 2^(log n + 1) points (ntt.hpp)
int quot_domains(uint32_t log_mm, const Ntt3Domain** d3, const NttDomain** dm) {
  int rc = get_domain3(log_mm, d3);
  if (rc) return rc;
  return get_domain(log_mm, dm);
}
// coset evaluations on the 6n domain of `count` polynomials read through io (one polynomial family per call)
int run_ntt3_fwd(hipStream_t s, uint32_t log_mm, fe* data, uint32_t count, const NttIo& io) {
  Context& c = ctx();
  const Ntt3Domain* d3 = nullptr;
  const NttDomain* dm = nullptr;
  int rc = quot_domains(log_mm, &d3, &dm);
  if (rc) return rc;
  if ((rc = scratch_reserve(c.ntt_scratch, ntt3_scratch(log_mm, count)))) return rc;
  rc = ntt3_forward(*d3, *dm, c.small, data, io, count, (fe*)c.ntt_scratch.p, s);
  if (rc) return hip_fail((hipError_t)rc, "ntt3_forward");
  return CAPGPU_OK;
}
// the same on five of the six n-cosets (ntt.hpp: ntt3_forward5 / ntt3_inverse5)
int run_ntt3_fwd5(hipStream_t s, uint32_t log_mm, fe* data, uint32_t count, const NttIo& io) {
  Context& c = ctx();
  const Ntt3Domain* d3 = nullptr;
  const NttDomain *dm = nullptr, *dh = nullptr;
  int rc = quot_domains(log_mm, &d3, &dm);
  if (rc || (rc = get_domain(log_mm - 1, &dh))) return rc;
  if ((rc = scratch_reserve(c.ntt_scratch, ntt3_scratch(log_mm, count, true)))) return rc;
  rc = ntt3_forward5(*d3, *dm, *dh, c.small, data, io, count, (fe*)c.ntt_scratch.p, s);
  if (rc) return hip_fail((hipError_t)rc, "ntt3_forward5");
  return CAPGPU_OK;
}
int run_ntt3_inv5(hipStream_t s, uint32_t log_mm, fe* data, uint32_t count, const fe* top, const fe* add) {
  Context& c = ctx();
  const Ntt3Domain* d3 = nullptr;
  const NttDomain *dm = nullptr, *dh = nullptr;
  int rc = quot_domains(log_mm, &d3, &dm);
  if (rc || (rc = get_domain(log_mm - 1, &dh))) return rc;
  if ((rc = scratch_reserve(c.ntt_scratch, ntt3_scratch(log_mm, count, true)))) return rc;
  rc = ntt3_inverse5(*d3, *dm, *dh, c.small, data, count, (fe*)c.ntt_scratch.p, s, top, add);
  if (rc) return hip_fail((hipError_t)rc, "ntt3_inverse5");
  return CAPGPU_OK;
}
// add: see ntt3_inverse
int run_ntt3_inv(hipStream_t s, uint32_t log_mm, fe* data, uint32_t count, const fe* add = nullptr) {
  Context& c = ctx();
  const Ntt3Domain* d3 = nullptr;
  const NttDomain* dm = nullptr;
  int rc = quot_domains(log_mm, &d3, &dm);
  if (rc) return rc;
  if ((rc = scratch_reserve(c.ntt_scratch, ntt3_scratch(log_mm, count)))) return rc;
  rc = ntt3_inverse(*d3, *dm, c.small, data, count, (fe*)c.ntt_scratch.p, s, add);
  if (rc) return hip_fail((hipError_t)rc, "ntt3_inverse");
  return CAPGPU_OK;
}

}  // namespace
int run_msm(hipStream_t s, const MsmBases& B, const fe* scalars, size_t outer_stride, uint32_t inner,
            size_t inner_stride, size_t n, uint32_t batch, g1_jac* d_out) {
  Context& c = ctx();
  auto local = [&](size_t lo, size_t len) -> int {
    int rc = scratch_reserve(c.msm_ws, msm_workspace_bytes(B, len, batch));
    if (rc) return rc;
    rc = msm_run(B, lo, scalars + lo, outer_stride, inner, inner_stride, len, batch, 1, d_out, c.msm_ws.p, c.msm_ws.cap, s);
    return rc ? hip_fail((hipError_t)rc, "msm_run") : CAPGPU_OK;
  };
  if (!comm_shard_prover()) return local(0, n);
  // Mode A of BASELINE config 4 (capgpu_plonk_shard_msm): every rank proves the same batch, each commitment MSM is cut
  // by point range over the ranks and finished by one all-gather of 96-byte partials + G - 1 additions.
  // All ranks then hold the same commitments, derive the same challenges and stay in lock step.  A rank whose local
  // part fails still enters the exchange (comm_allgather_sum), so every rank leaves with an error.  Under the loopback
  // communicator this process plays the ranks one after the other.
  const size_t world = (size_t)comm_world();
  const bool loop = comm_loopback();
  for (size_t rank = loop ? 0 : (size_t)comm_rank(), last = loop ? world - 1 : rank; rank <= last; rank++) {
    if (loop) comm_loopback_rank((int)rank);
    const size_t base = n / world, rem = n % world;
    const size_t lo = rank * base + std::min(rank, rem), len = base + (rank < rem ? 1 : 0);
    int rc = comm_allgather_sum(d_out, batch, s, local(lo, len));
    if (rc) return rc;
  }
  return CAPGPU_OK;
}
// pk::pad_copy for the key builders of plonk_keys.hip
void pad_columns(hipStream_t s, fe* dst, size_t dst_outer, size_t dst_inner, const fe* src, size_t src_outer,
                 size_t src_inner, uint32_t inner, uint32_t count, size_t len, size_t total) {
  pad_copy(s, dst, dst_outer, dst_inner, src, src_outer, src_inner, inner, count, len, total);
}

// A key's constants as the kernels take them.  ProvingKey keeps them in ks::QuotConst, the definition a unit without
// device code sees (plonk_key.hpp); this unit sees the kernels' own too and holds the two together.
static_assert(ks::NW == NW && ks::NS == NS && ks::kPkcCols == kPkcCols && sizeof(ks::QuotConst) == sizeof(QuotConst) &&
                  offsetof(ks::QuotConst, g) == offsetof(QuotConst, g) && offsetof(ks::QuotConst, k) == offsetof(QuotConst, k) &&
                  offsetof(ks::QuotConst, zh_inv) == offsetof(QuotConst, zh_inv),
              "plonk_key.hpp restates the key's shape for the host units");
static inline QuotConst quot_const(const ks::QuotConst& q) {
  QuotConst r;
  memcpy(&r, &q, sizeof r);
  return r;
}
namespace {

struct BatchWs {
  fe *wpoly, *wev, *pi, *num, *den, *pre, *sfx, *scan_tot, *inv_total, *zpoly, *coset, *pkc, *t, *pows, *pows_small, *pw, *batchpoly,
      *hbuf, *quot, *evals, *eval_partial, *d_pub, *d_blind;
  Chal* chal;
  Chal* chal29;  // the same challenges in the internal form
  uint32_t* flags;
  g1_jac* comms;
  EvalDesc* edesc;
  LinTerm* terms;
  const fe** key_ptrs;  // [3][P]: sigma evaluations / coset columns / coefficients of every proof's key (mixed-key batches)
  // the five-coset quotient: its top coefficients [P][8] (k_quotient_top) and the row test's keys and verdicts (r3_body)
  fe* top;
  CheckKey* chk_keys;
  CheckOut* chk_out;
  // device transcript only (capgpu_plonk_set_transcript): the proofs in ABI layout, zeta, and the transcript's bytes
  uint8_t *d_proofs, *tr_state, *tr_pre, *tr_app;
  uint32_t* tr_pre_len;
  fe* zeta;
  // ... and what k_prove_outcomes reads and writes (capgpu_plonk_prove_each*): the witness check's verdicts, the status words
  unsigned long long* chk_first;
  int32_t* status;
  size_t total;
};
constexpr uint32_t kLinTerms = 29;
static_assert(oc::kCheckNoFault == pk::kNoFault && sizeof(pk::CheckOut::first) == sizeof(unsigned long long),
              "k_prove_outcomes reads the witness check's verdicts (CheckOut::first)");
static_assert(kLinTerms == (uint32_t)td::kLinScalars, "transcript_dev.hpp derives the scalars of k_lincomb's terms");

BatchWs carve(void* base, const ProvingKey& K, uint32_t P, size_t num_inputs, bool coeffs, uint32_t tr_stride = 0) {
  Carver c(base);
  BatchWs w{};
  size_t n = K.n, m = K.m, ps = K.ps;
  w.wpoly = c.take<fe>((size_t)P * NW * ps);
  // coefficient-form input: the witness VALUES round 2 reads are one forward transform of the caller's polynomials
  w.wev = coeffs ? c.take<fe>((size_t)P * NW * n) : nullptr;
  // kappa PI(X), kappa = 1 / (5^(6n) - 1): what round 3 adds to the quotient's coefficients (pi_fold)
  w.pi = num_inputs ? c.take<fe>((size_t)P * n) : nullptr;
  w.num = c.take<fe>((size_t)P * n);
  w.den = c.take<fe>((size_t)P * n);
  w.pre = c.take<fe>((size_t)P * n);
  w.sfx = c.take<fe>((size_t)P * n);
  w.scan_tot = c.take<fe>((size_t)P * 2 * (cdiv(ps, kScanBlock) + 1));
  w.inv_total = c.take<fe>(P);
  w.zpoly = c.take<fe>((size_t)P * ps);
  w.coset = c.take<fe>((size_t)P * 6 * m);
  w.pkc = K.recompute ? c.take<fe>((size_t)kPkcCols * m) : nullptr;
  w.t = c.take<fe>((size_t)P * m);
  w.pows = c.take<fe>((size_t)P * 4 * ps);
  w.pw = c.take<fe>((size_t)P * 4 * 24);
  w.pows_small = c.take<fe>((size_t)P * 4 * (kPowLow + (ps + kPowLow - 1) / kPowLow));
  w.batchpoly = c.take<fe>((size_t)P * 2 * ps);
  w.hbuf = c.take<fe>((size_t)P * 2 * ps);
  w.quot = c.take<fe>((size_t)P * 2 * ps);
  w.evals = c.take<fe>((size_t)P * 10);
  w.eval_partial = c.take<fe>((size_t)P * 10 * kEvalChunks);
  w.d_pub = c.take<fe>((size_t)P * (num_inputs ? num_inputs : 1));
  w.d_blind = c.take<fe>((size_t)P * 13);
  w.chal = c.take<Chal>(P);
  w.chal29 = c.take<Chal>(P);
  w.flags = c.take<uint32_t>(P);
  w.comms = c.take<g1_jac>((size_t)P * 5);
  w.edesc = c.take<EvalDesc>((size_t)P * 10);
  w.terms = c.take<LinTerm>((size_t)P * kLinTerms);
  w.key_ptrs = c.take<const fe*>((size_t)P * 3);
  w.top = c.take<fe>((size_t)P * 8);
  w.chk_keys = c.take<CheckKey>(P);
  w.chk_out = c.take<CheckOut>(P);
  if (tr_stride) {  // (last: the host mode's layout is a prefix of this one)
    w.d_proofs = c.take<uint8_t>((size_t)P * td::kPrBytes);
    w.zeta = c.take<fe>(P);
    w.tr_state = c.take<uint8_t>((size_t)P * 64);
    w.tr_app = c.take<uint8_t>((size_t)P * td::kAppBytes);
    w.tr_pre_len = c.take<uint32_t>(P);
    w.tr_pre = c.take<uint8_t>((size_t)P * tr_stride);
    w.chk_first = c.take<unsigned long long>(P);
    w.status = c.take<int32_t>(P);
  }
  w.total = c.off + 256;
  return w;
}

// the 18 fixed polynomials -> coset evaluations on the 6n quotient domain
int compute_pk_coset(hipStream_t s, const ProvingKey& K, fe* dst) {
  return run_ntt3_fwd(s, K.log_m, dst, 18, NttIo{K.coef, K.ps, 0, K.n, 1, K.m, 0, 1});
}
// columns 18 .. 21 of the same table: k_j x_i, j = 1 .. 4 (k_quotient's folded permutation terms)
int compute_pk_kx(hipStream_t s, const ProvingKey& K, fe* dst) {
  const Ntt3Domain* dq = nullptr;
  if (int rc = get_domain3(K.log_m, &dq)) return rc;
  kx_columns(s, dst + (size_t)18 * K.m, (const fe*)dq->xs29, quot_const(K.qc29), K.m);
  return CAPGPU_OK;
}
// CAPGPU_QUOT_FOLD (read per call): 1, the default - k_quotient's permutation terms with beta folded out; 0 - the direct
// form for every proof (A/B in one build); 2 - folded, with every proof's 1 / beta zeroed first: all of them take the route
// of a proof with beta = 0 (the folded launch leaves them out, the direct launch behind it takes them) - for tests.
int quotient_fold() {
  return env_int("CAPGPU_QUOT_FOLD", 1, 0, 2);
}
// CAPGPU_QUOT_COSETS (read per call): 5, the default - round 3 evaluates on five of the six n-cosets of the quotient domain
// and takes the quotient's top 8 coefficients from the polynomials; 6 - all six, the top coefficients
// from the interpolation (A/B in one build, tests).  Domains below n = 16 and keys of the reference schedule
// (ProvingKey::recompute) take six whatever it says.
int quotient_cosets() {
  return env_int("CAPGPU_QUOT_COSETS", 5, 5, 6);
}

// Round 1's wire commitments: from the wire polynomials' coefficients (jf-plonk's way: KZG10::commit under
// src/proof/transfer.rs:181-186) or from the witness VALUES on the Lagrange-form commit key of the domain (lagrange.hip) -
// the same group elements, the same proof bytes; a CAP witness is mostly zeros, booleans and small limbs, whose MSM scalars
// have one non-zero digit or none.  capgpu_plonk_set_wire_commit: 0 coefficients, 1 evaluations, -1 the default
// (evaluations; CAPGPU_WIRE_COMMIT=coeffs turns it off for the process).
std::atomic<int> g_wire_commit{-1};
}  // namespace
bool wire_commit_from_evals() {
  static const int env_default = [] {
    const char* e = getenv("CAPGPU_WIRE_COMMIT");
    return (e && (!strcmp(e, "coeffs") || !strcmp(e, "0"))) ? 0 : 1;
  }();
  const int m = g_wire_commit.load(std::memory_order_relaxed);
  return (m < 0 ? env_default : m) != 0;
}
namespace {

// Where the Fiat-Shamir transcript of a prove call runs (capgpu_plonk_set_transcript; CAPGPU_TRANSCRIPT=device|host sets
// the process default): on the host - between the rounds the commitments come back, the host hashes them and sends the
// challenges - or on the device (transcript_dev.hpp), where the whole call is enqueued at once and waited for once.
std::atomic<int> g_transcript{-1};
int transcript_mode() {
  static const int env_default = [] {
    const char* e = getenv("CAPGPU_TRANSCRIPT");
    return (e && (!strcmp(e, "device") || !strcmp(e, "1"))) ? CAPGPU_TRANSCRIPT_DEVICE : CAPGPU_TRANSCRIPT_HOST;
  }();
  const int m = g_transcript.load(std::memory_order_relaxed);
  return m < 0 ? env_default : m;
}
// the round-2 inversion as a device kernel (the pre-round-4 schedule); the device transcript always does
bool perm_inv_on_device() {
  static const bool on = env_int("CAPGPU_PERM_INV_ON_DEVICE", 0) != 0;
  return on;
}
// The witnesses are checked against their circuits before anything is committed to (the check itself: plonk.hip).
std::atomic<int> g_precheck{0};             // capgpu_plonk_set_precheck
thread_local bool tl_prechecked = false;    // the batch this thread is about to prove has been checked already (coalescer)

// The stream the chunks of host-resident wire columns are copied on: a copy on the launch stream itself would queue up
// behind the kernels of the chunk before it (calls are serialised by the process lock; created on first use).
hipStream_t h2d_stream() {
  Context& c = ctx();
  if (!c.copy_stream && hipStreamCreateWithFlags(&c.copy_stream, hipStreamNonBlocking) != hipSuccess)
    c.copy_stream = nullptr;
  return c.copy_stream;
}
// Small batches leave most of the chip idle during round 1's commitment MSMs (a chain of a dozen short launches per MSM
// launch): the wire polynomials' interpolation, blinding and coset transforms - which round 3 needs, not the commitments
// when those are taken from evaluations - run beside them on a side stream of the context (fork / join by events inside
// segment 0, so a captured graph gets two branches).  CAPGPU_R1_OVERLAP_MAX: largest batch that does so (default 3, 0 =
// off).  Measured, same box (profiles/small_launch_ab_r05.txt): batch 1 2.59 -> 2.38 ms, batch 2 3.8 -> 3.7 ms, batch 4
// even, batches of 8 and 16 1-2 % SLOWER - there the transforms no longer fit beside the MSMs, they only slow them down.
uint32_t r1_overlap_max() {
  static const uint32_t v = [] {
    const int x = env_int("CAPGPU_R1_OVERLAP_MAX", 3);
    return (uint32_t)(x < 0 ? 0 : (x > 4096 ? 4096 : x));
  }();
  return v;
}
hipStream_t side_stream(Context& c) {
  if (!c.side_stream) {
    if (hipStreamCreateWithFlags(&c.side_stream, hipStreamNonBlocking) != hipSuccess) c.side_stream = nullptr;
    if (c.side_stream && (hipEventCreateWithFlags(&c.ev_fork, hipEventDisableTiming) != hipSuccess ||
                          hipEventCreateWithFlags(&c.ev_join, hipEventDisableTiming) != hipSuccess)) {
      (void)hipStreamDestroy(c.side_stream);
      c.side_stream = nullptr;
    }
    (void)hipGetLastError();
  }
  return c.side_stream;
}
// The parts of ONE dealt host batch (capgpu_plonk_prove_batch cuts it over two contexts of a device) copy their witnesses
// in PART ORDER, not side by side: two copies at once share the link, both parts' first chunks land late and the GPU idles
// for both; in part order the first part's first chunk lands after half that time and its kernels run while the second
// part's witnesses arrive (round-5 VERDICT item 2: pcie_inclusive 0.92 of the resident rate).  A part takes its turn
// before its first copy - for a BOUNDED time: it holds its context's lock while it waits, and a concurrent batch whose
// parts picked the contexts in the other order would otherwise deadlock with it (tests/test_gpu_multidev.py found that);
// after 100 ms it copies anyway, side by side as before round 6 - and passes it on when its last copy has landed; the
// dealer passes a part's turn on when the part returns, whatever happened inside (an error path never holds the others
// up).  Only batches of 64 proofs and more take turns: below that the copies are too short to matter.
struct H2dTurn {
  std::mutex mu;
  std::condition_variable cv;
  uint32_t next = 0;
  bool wait_for(uint32_t idx, uint32_t timeout_ms) {  // false: timed out (the caller goes ahead regardless)
    std::unique_lock<std::mutex> lk(mu);
    return cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), [&] { return next >= idx; });
  }
  void pass(uint32_t idx) {  // part idx is done copying (idempotent)
    std::lock_guard<std::mutex> lk(mu);
    if (next < idx + 1) next = idx + 1;
    cv.notify_all();
  }
};
thread_local H2dTurn* tl_h2d_turn = nullptr;
thread_local uint32_t tl_h2d_index = 0;
static bool h2d_in_part_order() {
  static const bool on = env_int("CAPGPU_H2D_PART_ORDER", 1) != 0;
  return on;
}

// chunks of proofs the host-resident wire columns of a batch are copied and committed in (round 1 of prove_batch)
uint32_t h2d_chunks(uint32_t P) {
  static const int forced = env_int("CAPGPU_PROVE_CHUNKS", 0, 1, 16);  // tests: any batch in 1..16 chunks
  if (forced) return std::min<uint32_t>((uint32_t)forced, P);
  return P >= 64 ? 4u : (P >= 32 ? 2u : 1u);  // a chunk's commitments should still fill the chip (>= 80 MSMs)
}
// first proof of chunk ck (ck = chunks: P).  Equal chunks - except that the FIRST chunk of a batch of >= 64 proofs that
// starts on an idle device is kept short (CAPGPU_PROVE_FIRST_CHUNK proofs, default 16; 0 = equal chunks): nothing runs
// until it has landed.
uint32_t h2d_chunk_start(uint32_t P, uint32_t chunks, uint32_t ck, bool short_first) {
  static const uint32_t first = (uint32_t)env_int("CAPGPU_PROVE_FIRST_CHUNK", 16, 0, 4096);
  if (ck == 0) return 0;
  if (ck >= chunks) return P;
  if (!short_first || first == 0 || chunks < 3 || first * chunks >= P) return (uint32_t)((uint64_t)P * ck / chunks);
  return first + (uint32_t)((uint64_t)(P - first) * (ck - 1) / (chunks - 1));
}

// ---- variable-form input (CAPGPU_INPUT_VARS; kernels: vars_kernels.hpp) ------------------------------------------------
// A witness arrives as one value per variable and becomes the five wire columns on the device, through the table its key
// keeps: 32 B x num_vars over the link instead of 32 B x 5 n.  Everything behind the gather is the evals path.
}  // namespace
std::atomic<uint64_t> g_witness_h2d{0}, g_gather_launches{0};  // capgpu_plonk_input_stats
namespace {
inline void count_witness_h2d(size_t bytes) { g_witness_h2d.fetch_add(bytes, std::memory_order_relaxed); }

// Context::stage_b for `cnt` witnesses in variable form: the five columns the gather writes ([cnt][5 n], where the evals
// path copies them) and - host-resident input only - behind them the staged value vectors ([cnt][stride])
inline size_t vars_stage_bytes(size_t cnt, size_t n, size_t stride, bool host) {
  return wires_stage_bytes(cnt, n) + (host ? sizeof(fe) * cnt * stride : 0);
}
// the value vectors of a batch on the device: proof p's at d_vars + p * stride, its key's num_vars <= stride of them used
struct VarsIn {
  const fe* d_vars;
  size_t stride;
};
bool key_lacks_table(const ProvingKey& K) {
  if (K.wire_vars) return false;
  set_error("capgpu_plonk: CAPGPU_INPUT_VARS: key has no variable table (capgpu_plonk_preprocess_vars or "
            "capgpu_plonk_key_set_vars gives it one)");
  return true;
}
// columns of proofs [p0, p0 + cnt) into d_cols ([P][5][n]): one launch per run of proofs that share a key
void gather_vars(hipStream_t s, const ProvingKey& K, const std::vector<const ProvingKey*>* keys, uint32_t p0, uint32_t cnt,
                 const VarsIn& in, fe* d_cols) {
  const size_t cells = (size_t)NW * K.n;
  for (uint32_t p = p0; p < p0 + cnt;) {
    uint32_t q = p0 + cnt;
    if (keys)
      for (q = p + 1; q < p0 + cnt && (*keys)[q] == (*keys)[p];) q++;
    const ProvingKey& Kp = keys ? *(*keys)[p] : K;
    // enough lanes to fill the chip; the proofs beyond that are the lane's loop (the table stays in its register)
    const uint32_t rows = std::min<uint32_t>(q - p, (uint32_t)std::max<size_t>(1, ((size_t)1 << 20) / (2 * cells)));
    launch("k_gather_vars", k_gather_vars, dim3(cdiv(2 * cells, kThreads), rows), dim3(kThreads), 0, s,
           (const uint4*)(in.d_vars + (size_t)p * in.stride), in.stride, (const uint32_t*)Kp.wire_vars, cells, q - p,
           (uint4*)(d_cols + (size_t)p * cells));
    g_gather_launches.fetch_add(1, std::memory_order_relaxed);
    p = q;
  }
}

// the pinned result area of a batch of P proofs: the proofs, the degree flags and the status words of an outcome call
// (device transcript), or a round's commitments, the grand-product totals, the evaluations and the flags (host transcript)
size_t prove_pinned_bytes(uint32_t P, bool dev_tr) {
  if (dev_tr) return (size_t)P * td::kPrBytes + sizeof(uint32_t) * P + sizeof(int32_t) * P + 768;
  return sizeof(g1_jac) * P * NW + sizeof(fe) * P * 11 + sizeof(uint32_t) * P + 1024;
}
// bytes per proof of the device transcript's prefix (init message || vk_bytes || public inputs), in steps of 256: the
// stride is part of a captured graph's signature
uint32_t transcript_stride(size_t longest) { return (uint32_t)((longest + 256) / 256 * 256); }

// ---- the plan of one call: every mode decision, made once ----------------------------------------------------------
// What a batch of P proofs under K will do - which form its input has and where it is, whether the witnesses are checked
// first, where the transcript runs, which commit key rounds 1 and 2 commit on, whether round 1 runs in chunks or beside
// a side stream, whether the segments replay as graphs.  prove_batch runs the plan, prove_needs sizes it and
// capgpu_plonk_reserve reserves what it sizes: none of them decides a mode of its own.
struct ProvePlan {
  uint32_t P = 0;
  int form = CAPGPU_INPUT_EVALS;
  bool coeffs = false, vars = false;
  bool host = false;       // the input arrives in host memory ...
  bool r1_copies = false;  // ... and is copied inside round 1, chunk by chunk (not up front, for the witness check)
  bool precheck = false;   // capgpu_plonk_set_precheck: the witnesses are checked against their circuits first
  // the transcript on the device (capgpu_plonk_set_transcript) - except under sharded commitment MSMs, whose partial
  // commitments meet through a host-driven exchange: those calls keep the host transcript
  bool dev_tr = false;
  uint32_t tr_stride = 0;      // bytes per proof of the transcript's prefix: init message || vk_bytes || public inputs
  bool inv_on_device = false;  // the round-2 inversion as a device kernel
  uint32_t chunks = 1;         // chunks of proofs round 1 copies and commits host-resident input in
  // small batches run rounds 1-2 on two streams (r1_overlap_max); decided once, because it shapes the captured graphs
  bool overlap = false;
  hipStream_t s2 = nullptr;
  bool graphs = false;  // small batches replay their kernel segments as hipGraphs (see ProveGraphSet)
  bool five = false;    // round 3 on five of the six n-cosets (quotient_cosets)
  const MsmBases* B = nullptr;
  const MsmBases* Lag = nullptr;  // the Lagrange-form commit key rounds 1 and 2 commit on (null: from coefficients)
  const MsmBases& wire_key() const { return Lag ? *Lag : *B; }
};

// `longest_prefix`: the longest transcript prefix among the proofs (init message || vk_bytes || public inputs).
// `sizing` (capgpu_plonk_reserve): the plan of a call that is not being made - it takes the superset where a proving
// call looks at its own thread and stream (a witness check the coalescer may already have run, a side stream the call
// may not get), and leaves no trace event.
int make_plan(Context& c, const ProvingKey& K, uint32_t P, int form, bool host, size_t longest_prefix, bool sizing,
              ProvePlan* out) {
  ProvePlan pl;
  pl.P = P;
  pl.form = form;
  pl.coeffs = form == CAPGPU_INPUT_COEFFS;
  pl.vars = form == CAPGPU_INPUT_VARS;
  pl.host = host;
  int rc = find_srs(K.srs_handle, &pl.B);
  if (rc) return rc;
  // The check reads whole witnesses, so host-resident ones are copied in one go, ahead of it, instead of chunk by chunk in
  // round 1.
  pl.precheck = g_precheck.load(std::memory_order_relaxed) != 0 && (sizing || !tl_prechecked);
  pl.r1_copies = host && !pl.precheck;
  // the Lagrange-form commit key (built on the first proof of this domain size under this SRS if preprocess did not);
  // sharded commitment MSMs (mode A of config 4) cut the monomial key by point range: they keep the coefficient form
  // The Lagrange-form key is an OPTIMISATION (the same commitments come from the coefficients): when it cannot be had -
  // its table is as large as the SRS's window table and is built on first use with temporaries of its own - the proof is
  // made the coefficient way instead of failing.  Only a bad handle is an error of the call.
  if (wire_commit_from_evals() && !comm_shard_prover() && (rc = find_lagrange(K.srs_handle, K.log_n, &pl.Lag))) {
    if (rc == CAPGPU_ERR_BAD_HANDLE) return rc;
    pl.Lag = nullptr;
    (void)hipGetLastError();
    if (!sizing) trace("pb_lagrange_fallback", c.slot, rc);
  }
  pl.dev_tr = transcript_mode() == CAPGPU_TRANSCRIPT_DEVICE && !comm_shard_prover();
  pl.five = quotient_cosets() == 5 && K.log_n >= 4 && !K.recompute;
  if (pl.dev_tr) {
    if (longest_prefix > (1u << 30)) {
      set_error("capgpu_plonk_prove: transcript init message of %zu bytes", longest_prefix);
      return CAPGPU_ERR_INVALID_ARG;
    }
    pl.tr_stride = transcript_stride(longest_prefix);
  }
  pl.inv_on_device = perm_inv_on_device() || pl.dev_tr;
  pl.chunks = pl.r1_copies ? h2d_chunks(P) : 1;
  // (graphs and the side stream only on the library's own stream: a caller's - capgpu_set_stream - may carry work of its own)
  const bool own = !c.prof.on && c.stream == c.own_stream;
  pl.overlap = pl.chunks == 1 && P <= r1_overlap_max() && (sizing || (own && !comm_shard_prover())) &&
               (pl.s2 = side_stream(c)) != nullptr;
  // (a captured segment keeps the launches it was captured with: only the default form of k_quotient is captured)
  pl.graphs = P <= graph_max_batch() && pl.chunks == 1 && own && comm_shard_slot() < 0 && quotient_fold() == 1;
  *out = pl;
  return CAPGPU_OK;
}

// ---- capgpu_plonk_reserve: what a plan would ask of the context's scratch ----------------------------------------
// The largest request per buffer.  Every step of ProveRun that reserves scratch has a `*_needs` beside it that asks the
// SAME size functions its launches use (carve, msm_workspace_bytes, ntt*_scratch, prove_pinned_bytes, *_stage_bytes);
// ProveRun::needs adds them up over the plan's schedule.
struct ProveNeeds {
  size_t prove_ws = 0, msm_ws = 0, ntt_scratch = 0, stage_a = 0, stage_b = 0, pinned = 0;
  void ntt(size_t bytes) { ntt_scratch = std::max(ntt_scratch, bytes); }
  void msm(const MsmBases& T, size_t len, uint32_t batch) { msm_ws = std::max(msm_ws, msm_workspace_bytes(T, len, batch)); }
};

// ---- one call's arguments ---------------------------------------------------------------------------------------------
// msgs / msg_lens (optional): one transcript init message per proof; otherwise ext_msg is shared by the batch.
// keys (optional): the proving key of every proof - keys of ONE domain size under ONE SRS (the reference proves transfer,
// mint and freeze notes side by side, src/utils/params_builder.rs:194-226; proofs of different circuits on the same
// domain share every MSM and NTT launch, only k_perm_numden / k_quotient and the descriptors of rounds 4-5 read key
// data).  K is then keys[0] - it lends the domain-level tables and the workspace - and pub_inputs holds P rows of
// `num_inputs` = the largest count among the keys, a key with fewer inputs using the first of its row.
// form: CAPGPU_INPUT_EVALS - d_wires / h_wires hold the wire assignment, 5 columns of n values per proof (round 1
// interpolates them); CAPGPU_INPUT_COEFFS - they hold the 5 wire POLYNOMIALS, n coefficients each, as jf-relation's
// compute_wire_polynomials returns them (src/proof/transfer.rs:181-186 holds that circuit): round 1 takes them as they
// are and round 2's witness values come from ONE forward transform on the device.  The proofs are the same bytes.
// CAPGPU_INPUT_VARS - the input is one value per variable, `vin->stride` elements per proof at vin->d_vars; d_wires is
// device scratch for the five columns, which k_gather_vars writes there through the keys' tables (chunk by chunk behind
// the chunk's copy when the values are still on the host); from there on the call is the evals form.
// h_wires (optional): the input is still in host memory - h_wires[p] points to the 5 n elements (variable form:
// num_vars values) of proof p - and d_wires (variable form: vin->d_vars) is an empty device buffer for them.
// Round 1 then runs in chunks of proofs - copy, interpolate, blind, commit - so that the copy of a chunk (pageable
// memory: the call blocks the host, not the device) overlaps the commitments of the one before.
struct ProveRequest {
  const fe* d_wires = nullptr;
  const uint64_t* pub_inputs = nullptr;
  size_t num_inputs = 0;
  const uint64_t* blinders = nullptr;
  capgpu_proof* proofs = nullptr;
  const uint8_t* ext_msg = nullptr;
  size_t ext_len = 0;
  const uint8_t* const* msgs = nullptr;
  const size_t* msg_lens = nullptr;
  const std::vector<const ProvingKey*>* keys = nullptr;
  const uint64_t* const* h_wires = nullptr;
  int form = CAPGPU_INPUT_EVALS;
  const VarsIn* vin = nullptr;
  // capgpu_plonk_prove_each*: one record per proof.  The call then proves PAST an unsatisfied witness - neither the
  // witness check nor the degree check ends it - and every proof gets its own verdict (outcome.hpp); null: all or nothing.
  capgpu_prove_outcome* outcomes = nullptr;
};

// ---- one call's run ---------------------------------------------------------------------------------------------------
// The steps of a planned call on a carved workspace: input, the five rounds' kernels, the results, and the two drivers
// that put them in order - run_host_transcript() (the host hashes between the rounds: eight graph segments, six or seven
// host waits) and run_device_transcript() (one segment, one wait).  begin() comes first in either.
struct ProveRun {
  // no exit path - an error between a fork and its join in particular - may leave the side stream running kernels on this
  // context's workspace: the next call (or a scratch growth) would pull it from under them.  (First
  // member: it drains after everything else here is gone.)
  struct SideDrain {
    Context& c;
    bool armed;
    ~SideDrain() {
      if (armed && c.side_stream) (void)hipStreamSynchronize(c.side_stream);
    }
  } side_drain;
  Context& c;
  const hipStream_t s;
  const ProvePlan& pl;
  const ProvingKey& K;
  const ProveRequest& rq;
  BatchWs w{};                  // prove_batch carves it ...
  ProveGraphSet* gs = nullptr;  // ... and picks the graph set, between the witness check and the driver
  const uint32_t P;
  const size_t n, m, ps, num_inputs;
  const fe* const d_wires;
  const uint64_t* pub_inputs;       // (mixed keys: redirected to pub_rows)
  const uint64_t* const* h_wires;  // the rows round 1 still has to copy (null: the input is resident)
  const NttDomain* dom_n = nullptr;
  const Ntt3Domain* dom_q = nullptr;
  const fe omega;
  const QuotConst qc29;  // K.qc29 as the kernels take it
  std::vector<uint64_t> pub_rows;  // mixed keys: the unused tail of a shorter key's row must be zero on the device
  std::vector<const fe*> key_ptrs;
  const fe* const* sig_of = nullptr;
  const fe* const* pkc_of = nullptr;
  const fe* const* coef_of = nullptr;
  std::vector<CheckKey> chk_keys;
  std::vector<SolidityTranscript> tr;  // host transcript only
  // Results the host needs between the rounds come back into PINNED memory of the context: a device-to-host copy into
  // pageable memory makes the runtime wait for the stream on the host first and copy through a staging buffer of its own
  // - two host round trips where one is needed, seven times per proof.
  g1_jac* hj = nullptr;         // [5 P] commitments of a round
  fe* h_tot = nullptr;          // [P] grand-product totals out, their inverses back
  bool beta_zero_possible = true;  // some proof's beta may be 0 (r3_body); the host transcript knows better
  fe* h_evals = nullptr;        // [10 P]
  uint32_t* h_flags = nullptr;  // [P]
  uint8_t* h_proofs = nullptr;  // [P] device transcript: the proofs in ABI layout, then the degree flags
  int32_t* h_status = nullptr;  // [P] device transcript, outcome calls: k_prove_outcomes' status words
  // outcome calls under capgpu_plonk_set_precheck: the check's verdicts (prove_batch keeps them instead of returning);
  // on the device they are in w.chk_first
  const capgpu_witness_fault* faults = nullptr;
  const size_t proofs_bytes;
  std::vector<g1_affine> ha;

  ProveRun(Context& c_, const ProvePlan& pl_, const ProvingKey& K_, const ProveRequest& rq_)
      : side_drain{c_, false}, c(c_), s(c_.stream), pl(pl_), K(K_), rq(rq_), P(pl_.P), n(K_.n), m(K_.m), ps(K_.ps),
        num_inputs(rq_.num_inputs), d_wires(rq_.d_wires), pub_inputs(rq_.pub_inputs),
        h_wires(pl_.r1_copies ? rq_.h_wires : nullptr), omega(ntt_root_of_unity(K_.log_n)), qc29(quot_const(K_.qc29)),
        proofs_bytes((size_t)pl_.P * td::kPrBytes) {}
  ProveRun(const ProveRun&) = delete;
  ProveRun& operator=(const ProveRun&) = delete;

  const ProvingKey& key_of(uint32_t p) const { return rq.keys ? *(*rq.keys)[p] : K; }
  template <class F>
  int seg(int id, F&& enqueue) {
    return run_segment(c, gs, id, enqueue);
  }
  hipError_t wait_stream() {  // every host wait on the proving stream goes through here (capgpu_plonk_sync_stats)
    g_stream_waits++;
    return hipStreamSynchronize(s);
  }
  // the whole schedule's requests (see ProveNeeds); the witness check's are prove_batch's own (plonk.hip)
  static void needs(const ProvePlan& pl, const ProvingKey& K, ProveNeeds& nd) {
    input_needs(pl, K, nd);
    begin_needs(pl, K, nd);
    if (pl.chunks > 1) {  // either placement of the short first chunk
      for (int short_first = 0; short_first < 2; short_first++)
        for (uint32_t ck = 0; ck < pl.chunks; ck++) {
          const uint32_t cnt = h2d_chunk_start(pl.P, pl.chunks, ck + 1, short_first != 0) -
                               h2d_chunk_start(pl.P, pl.chunks, ck, short_first != 0);
          if (cnt) r1_chunk_needs(pl, K, cnt, nd);
        }
    } else {
      r1_chunk_needs(pl, K, pl.P, nd);
      r1_overlapped_needs(pl, K, pl.P, nd);
    }
    r1_tail_needs(pl, K, pl.P, nd);
    cosets_needs(pl, K, pl.P, nd);
    commit_z_needs(pl, K, pl.P, nd);
    r3_needs(pl, K, pl.P, nd);
    r5_needs(pl, K, pl.P, nd);
  }

  // ---- input ----------------------------------------------------------------------------------------------------------
  // elements per proof of the input as it arrives, and where host-resident input is copied to
  size_t in_elems() const { return pl.vars ? rq.vin->stride : (size_t)NW * n; }
  size_t in_len(uint32_t p) const { return pl.vars ? key_of(p).num_vars : in_elems(); }
  // Host-resident input of proofs [p0, p1) -> its rows of the device buffer, on stream `st`.  A proof in variable form
  // brings the num_vars values of ITS key - callers of different keys gathered into one batch do not pad their buffers to
  // the row length -, so only full rows that follow each other in host memory travel as one copy (a plain batch: one per
  // chunk).
  int copy_input(uint32_t p0, uint32_t p1, hipStream_t st) {
    const size_t elems = in_elems();
    fe* const in_dst = const_cast<fe*>(pl.vars ? rq.vin->d_vars : d_wires);
    for (uint32_t p = p0; p < p1;) {
      uint32_t q = p + 1;
      while (q < p1 && in_len(q - 1) == elems && rq.h_wires[q] == rq.h_wires[q - 1] + (size_t)4 * elems) q++;
      const size_t bytes = sizeof(fe) * ((size_t)(q - 1 - p) * elems + in_len(q - 1));
      CAP_HIP(hipMemcpyAsync(in_dst + (size_t)p * elems, rq.h_wires[p], bytes, hipMemcpyHostToDevice, st));
      count_witness_h2d(bytes);
      p = q;
    }
    return CAPGPU_OK;
  }
  // variable form: the columns of proofs [p0, p0 + cnt) out of their value vectors
  void gather_vars(uint32_t p0, uint32_t cnt) { cap::gather_vars(s, K, rq.keys, p0, cnt, *rq.vin, const_cast<fe*>(d_wires)); }
  // Context::stage_b, which the entry points reserve for host-resident input and for the gathered columns
  static void input_needs(const ProvePlan& pl, const ProvingKey& K, ProveNeeds& nd) {
    if (pl.host) nd.stage_b = wires_stage_bytes(pl.P, K.n);
    if (pl.vars) nd.stage_b = vars_stage_bytes(pl.P, K.n, K.num_vars, pl.host);
  }
  // Host-resident input, chunk by chunk: each chunk's copy on the copy stream, its kernels - and, when the batch is
  // chunked, its commitments - behind it on the proving stream.
  int copy_chunks() {
    int rc;
    H2dTurn* const turn = h_wires ? tl_h2d_turn : nullptr;
    const uint32_t turn_idx = tl_h2d_index;
    if (turn) {
      const bool in_time = turn->wait_for(turn_idx, 100);
      trace("pb_h2d_turn", c.slot, in_time ? (int64_t)turn_idx : -1);
    }
    const bool short_first = h_wires && (!turn || turn_idx == 0);  // (a later part's copies run under the first part's kernels)
    for (uint32_t ck = 0; ck < pl.chunks; ck++) {
      const uint32_t p0 = h2d_chunk_start(P, pl.chunks, ck, short_first), p1 = h2d_chunk_start(P, pl.chunks, ck + 1, short_first);
      if (h_wires) {
        hipStream_t cs = pl.chunks > 1 ? h2d_stream() : nullptr;
        if (!cs) cs = s;
        if (cs != s && ck == 0) {  // the staging area may still be read by kernels of a call that returned early
          hipEvent_t ev;
          CAP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
          hipError_t e1 = hipEventRecord(ev, s), e2 = e1 == hipSuccess ? hipStreamWaitEvent(cs, ev, 0) : e1;
          (void)hipEventDestroy(ev);
          CAP_HIP(e2);
        }
        // one copy per run of proofs that are contiguous in host memory (a plain batch: one per chunk)
        trace("pb_h2d_issue", c.slot, ck);
        if ((rc = copy_input(p0, p1, cs))) return rc;
        trace("pb_h2d_issued", c.slot, ck);
        if (cs != s) {  // the chunk's kernels wait for its copy, not for the copies after it
          hipEvent_t ev;
          CAP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
          hipError_t e1 = hipEventRecord(ev, cs), e2 = e1 == hipSuccess ? hipStreamWaitEvent(s, ev, 0) : e1;
          (void)hipEventDestroy(ev);  // released once the recorded work is done
          CAP_HIP(e2);
        }
        if (pl.vars) gather_vars(p0, p1 - p0);  // the chunk's columns, behind its copy
      }
      if (pl.chunks > 1 && (rc = r1_chunk_kernels(p0, p1 - p0, true))) return rc;
    }
    if (turn) {
      // (a pageable source has landed when hipMemcpyAsync returns; a pinned one when its stream has drained: the next part
      // gets the link to itself either way.  This part's kernels are already enqueued behind their chunks.)
      if (pl.chunks > 1 && c.copy_stream) CAP_HIP(hipStreamSynchronize(c.copy_stream));
      turn->pass(turn_idx);
    }
    return CAPGPU_OK;
  }

  // ---- the head of either driver: per-call values up, the pinned result area, the input --------------------------------
  int begin() {
    int rc;
    side_drain.armed = pl.overlap;
    if ((rc = get_domain(K.log_n, &dom_n))) return rc;
    if ((rc = get_domain3(K.log_m, &dom_q))) return rc;
    g_prove_calls++;
    if (!pl.dev_tr) {
      tr.resize(P);
      parallel_for(P, [&](uint32_t p) {
        if (rq.msgs) {
          if (rq.msgs[p] && rq.msg_lens[p]) tr[p].append(rq.msgs[p], rq.msg_lens[p]);
        } else if (rq.ext_msg && rq.ext_len) {
          tr[p].append(rq.ext_msg, rq.ext_len);
        }
        const ProvingKey& Kp = key_of(p);
        tr[p].append(Kp.vk_bytes.data(), Kp.vk_bytes.size());
        for (size_t i = 0; i < Kp.num_inputs; i++) append_fr(tr[p], fe_from_words(pub_inputs + 4 * (p * num_inputs + i)));
      });
    }
    if (rq.keys && num_inputs) {
      pub_rows.assign(pub_inputs, pub_inputs + (size_t)4 * P * num_inputs);
      for (uint32_t p = 0; p < P; p++)
        for (size_t i = key_of(p).num_inputs; i < num_inputs; i++)
          for (int k = 0; k < 4; k++) pub_rows[4 * (p * num_inputs + i) + k] = 0;
      pub_inputs = pub_rows.data();
    }
    if (num_inputs)
      CAP_HIP(hipMemcpyAsync(w.d_pub, pub_inputs, sizeof(fe) * P * num_inputs, hipMemcpyHostToDevice, s));
    if (rq.keys) {
      key_ptrs.resize((size_t)3 * P);
      for (uint32_t p = 0; p < P; p++) {
        key_ptrs[p] = key_of(p).sig_eval;
        key_ptrs[P + p] = key_of(p).pk_coset;
        key_ptrs[2 * P + p] = key_of(p).coef;
      }
      CAP_HIP(hipMemcpyAsync(w.key_ptrs, key_ptrs.data(), sizeof(const fe*) * key_ptrs.size(), hipMemcpyHostToDevice, s));
      sig_of = w.key_ptrs;
      pkc_of = w.key_ptrs + P;
      coef_of = w.key_ptrs + 2 * P;
    }
    if (pl.five) {  // the row test's keys (prove_planned has built the selector values of every key)
      chk_keys.resize(P);
      for (uint32_t p = 0; p < P; p++) chk_keys[p] = CheckKey{key_of(p).chk_sel, nullptr, (uint32_t)key_of(p).num_inputs, 0};
      CAP_HIP(hipMemcpyAsync(w.chk_keys, chk_keys.data(), sizeof(CheckKey) * P, hipMemcpyHostToDevice, s));
      CAP_HIP(hipMemsetAsync(w.chk_out, 0xff, sizeof(CheckOut) * P, s));  // first = kNoFault
    }
    CAP_HIP(hipMemcpyAsync(w.d_blind, rq.blinders, sizeof(fe) * P * 13, hipMemcpyHostToDevice, s));
    CAP_HIP(hipMemsetAsync(w.flags, 0, sizeof(uint32_t) * P, s));
    // (reserved before the first launch: a growing area drains the context's streams)
    if ((rc = pinned_reserve(c, prove_pinned_bytes(P, pl.dev_tr)))) return rc;
    if (pl.dev_tr) {
      h_proofs = (uint8_t*)c.pin_host;
      h_flags = (uint32_t*)(h_proofs + (proofs_bytes + 255) / 256 * 256);
      h_status = (int32_t*)((char*)h_flags + (sizeof(uint32_t) * P + 255) / 256 * 256);
    } else {
      char* b = (char*)c.pin_host;
      hj = (g1_jac*)b;
      b += (sizeof(g1_jac) * P * NW + 255) / 256 * 256;
      h_tot = (fe*)b;
      b += (sizeof(fe) * P + 255) / 256 * 256;
      h_evals = (fe*)b;
      b += (sizeof(fe) * P * 10 + 255) / 256 * 256;
      h_flags = (uint32_t*)b;
    }
    return copy_chunks();
  }
  static void begin_needs(const ProvePlan& pl, const ProvingKey& K, ProveNeeds& nd) {
    nd.prove_ws = carve(nullptr, K, pl.P, K.num_inputs, pl.coeffs, pl.tr_stride).total;
    nd.pinned = prove_pinned_bytes(pl.P, pl.dev_tr);
  }

  // ---- results ----------------------------------------------------------------------------------------------------------
  // `keep_busy` enqueues work that does not depend on the next challenge: it runs on the GPU while the host turns the
  // commitments into challenges
  int fetch_comms(uint32_t count, const std::function<int()>& keep_busy = nullptr) {
    CAP_HIP(hipMemcpyAsync(hj, w.comms, sizeof(g1_jac) * count, hipMemcpyDeviceToHost, s));
    CAP_HIP(wait_stream());
    if (keep_busy) {
      int brc = keep_busy();
      if (brc) return brc;
    }
    // Jacobian -> affine on the host while the GPU waits for the next challenge: chunks of 64 points (one shared
    // inversion each) spread over the pool instead of one serial pass over up to 5P points
    ha.resize(count);
    const uint32_t chunk = 64, nchunks = (count + chunk - 1) / chunk;
    parallel_for(nchunks, [&](uint32_t ci) {
      const uint32_t lo = ci * chunk, hi = std::min(count, lo + chunk);
      std::vector<g1_jac> in(hj + lo, hj + hi);
      std::vector<g1_affine> out;
      batch_to_affine(in, out);
      std::copy(out.begin(), out.end(), ha.begin() + lo);
    });
    return CAPGPU_OK;
  }
  int degree_verdict(const uint32_t* flags) const {
    for (uint32_t p = 0; p < P; p++) {
      if (flags[p]) {
        char b[256];
        oc::degree_text(p, flags[p], b, sizeof b);
        set_error("%s", b);
        return CAPGPU_ERR_PROOF;
      }
    }
    return CAPGPU_OK;
  }
  // outcome calls, host transcript: every proof's record from its flags word and the check's verdict, on the host
  void host_outcomes(const uint32_t* flags) const {
    for (uint32_t p = 0; p < P; p++) oc::finish_outcome(flags[p], faults ? &faults[p] : nullptr, &rq.outcomes[p], &rq.proofs[p]);
  }

  // ---- round 1: wire polynomials, public-input polynomial, 5 commitments ------------------------------
  // the interpolations read the witness columns / public inputs where they are and write the coefficient arrays (no
  // padded copies); k_blind sets the 8-element tail of every wire polynomial (two blinders, six zeros)
  // the five commitments of proofs [p0, p0 + cnt): MSMs of the blinded polynomials' n + 2 coefficients on the monomial key,
  // or - same group elements - of each column's n VALUES followed by its two blinders on the Lagrange-form key.  The
  // scalars of the second form are staged in the quotient's array, which round 3 writes long after these MSMs.
  int commit_wires(uint32_t p0, uint32_t cnt) {
    g1_jac* out = w.comms + (size_t)p0 * NW;
    if (!pl.Lag) return run_msm(s, *pl.B, w.wpoly + (size_t)p0 * NW * ps, ps, 1, 0, n + 2, cnt * NW, out);
    fe* stage = w.t + (size_t)p0 * NW * (n + 2);
    const fe* ev = (pl.coeffs ? (const fe*)w.wev : d_wires) + (size_t)p0 * NW * n;
    launch("k_stage_evals", k_stage_evals, dim3(cdiv(n + 2, kThreads), cnt * NW), dim3(kThreads), 0, s, ev, n, n,
           (const fe*)(w.d_blind + (size_t)p0 * 13), (uint32_t)NW, 0u, 2u, stage);
    return run_msm(s, *pl.Lag, stage, n + 2, 1, 0, n + 2, cnt * NW, out);
  }
  // kernels of one chunk of proofs [p0, p0 + cnt): interpolation (or, from coefficient-form input, the copy into place
  // and the forward transform round 2 reads), blinding, and - when the batch is chunked - the chunk's commitments
  int r1_chunk_kernels(uint32_t p0, uint32_t cnt, bool commit) {
    const size_t wo = (size_t)p0 * NW * n;
    fe* wp = w.wpoly + (size_t)p0 * NW * ps;
    int r;
    if (pl.coeffs) {
      pad_copy(s, wp, ps, 0, d_wires + wo, n, 0, 1, cnt * NW, n, n);
      if ((r = run_ntt_from(s, K.log_n, d_wires + wo, n, n, w.wev + wo, n, cnt * NW, 0, 0))) return r;
    } else if ((r = run_ntt_from(s, K.log_n, d_wires + wo, n, n, wp, ps, cnt * NW, 1, 0))) {
      return r;
    }
    launch("k_blind", k_blind<1>, dim3(cnt * NW), dim3(64), 0, s, wp, ps, n, (const fe*)(w.d_blind + (size_t)p0 * 13),
           (uint32_t)NW, 0u, 2u, cnt * NW);
    if (commit && (r = commit_wires(p0, cnt))) return r;
    return CAPGPU_OK;
  }
  // (r1_chunk_kernels and commit_wires of `cnt` proofs: a chunk, or the batch)
  static void r1_chunk_needs(const ProvePlan& pl, const ProvingKey& K, uint32_t cnt, ProveNeeds& nd) {
    nd.ntt(ntt_scratch_from(K.log_n, (size_t)cnt * NW));
    nd.msm(pl.wire_key(), K.n + 2, cnt * NW);
  }
  // The public-input polynomial enters the quotient's numerator linearly and multiplies nothing, so it never goes to the
  // 6n domain: on the coset 5 <omega_6n> every point has x^(6n) = 5^(6n), hence 1 / Z_H(x) = kappa (1 + x^n + ... + x^(5n))
  // with kappa = 1 / (5^(6n) - 1), and the interpolant of PI(x) / Z_H(x) is kappa PI(X) (1 + X^n + ... + X^(5n)) exactly.
  // w.pi holds kappa PI(X) - kappa rides on the interpolation's n^-1 - and round 3's inverse transform adds it to each of
  // the six blocks of n coefficients (ntt3_inverse).  No public inputs: nothing to add, no array.
  int pi_fold(hipStream_t st) {
    if (!num_inputs) return CAPGPU_OK;
    return run_ntt_from(st, K.log_n, w.d_pub, num_inputs, num_inputs, w.pi, n, P, 1, 0, &dom_q->kappa_n_inv29);
  }
  int r1_tail_kernels() {
    int r;
    if ((r = pi_fold(s))) return r;
    if (pl.chunks == 1 && (r = commit_wires(0, P))) return r;
    return CAPGPU_OK;
  }
  static void r1_tail_needs(const ProvePlan&, const ProvingKey& K, uint32_t cnt, ProveNeeds& nd) {
    if (K.num_inputs) nd.ntt(ntt_scratch_from(K.log_n, cnt));  // the public-input polynomial
  }
  // round 3's coset evaluations of the wire polynomials (on the 6n quotient domain, straight from their coefficient
  // arrays: the transform zero-extends them) depend on nothing the transcript still has to produce.  w.coset: [P][6][m],
  // the wires at 0..4, z at 5.
  // (five cosets: [M][M][M / 2] at the head of every array of m)
  int r3_wire_cosets(hipStream_t st) {
    const NttIo io{w.wpoly, NW * ps, ps, n + 2, NW, 6 * m, m, NW};
    return pl.five ? run_ntt3_fwd5(st, K.log_m, w.coset, P * NW, io) : run_ntt3_fwd(st, K.log_m, w.coset, P * NW, io);
  }
  // the commitment to z and - independent of it - z's coset evaluations for round 3: one after the other (the second while
  // the host hashes), or, for the small batches of `overlap`, side by side on the two streams
  int z_cosets(hipStream_t st) {
    const NttIo io{w.zpoly, ps, 0, n + 3, 1, 6 * m, 0, 1};
    return pl.five ? run_ntt3_fwd5(st, K.log_m, w.coset + 5 * m, P, io) : run_ntt3_fwd(st, K.log_m, w.coset + 5 * m, P, io);
  }
  // (r3_wire_cosets and z_cosets)
  static void cosets_needs(const ProvePlan& pl, const ProvingKey& K, uint32_t cnt, ProveNeeds& nd) {
    nd.ntt(ntt3_scratch(K.log_m, (size_t)cnt * NW, pl.five));
    nd.ntt(ntt3_scratch(K.log_m, cnt, pl.five));
  }
  int r1_overlapped() {
    int r;
    const hipStream_t s2 = pl.s2;
    // every transform below shares c.ntt_scratch: those of the side stream run in its order, the one in front of the
    // fork before them.  The largest size is reserved now - a growth later would free a buffer still in use.
    if ((r = scratch_reserve(c.ntt_scratch, ntt3_scratch(K.log_m, (size_t)P * NW, pl.five)))) return r;
    auto interpolate_and_blind = [&](hipStream_t st) -> int {
      int q = CAPGPU_OK;
      if (pl.coeffs) pad_copy(st, w.wpoly, ps, 0, d_wires, n, 0, 1, P * NW, n, n);
      else q = run_ntt_from(st, K.log_n, d_wires, n, n, w.wpoly, ps, P * NW, 1, 0);
      if (q) return q;
      launch("k_blind", k_blind<1>, dim3(P * NW), dim3(64), 0, st, w.wpoly, ps, n, (const fe*)w.d_blind, (uint32_t)NW, 0u,
             2u, P * NW);
      return CAPGPU_OK;
    };
    // in front of the fork: what the commitments read
    if (pl.coeffs && (r = run_ntt_from(s, K.log_n, d_wires, n, n, w.wev, n, P * NW, 0, 0))) return r;
    if (!pl.Lag && (r = interpolate_and_blind(s))) return r;
    CAP_HIP(hipEventRecord(c.ev_fork, s));
    CAP_HIP(hipStreamWaitEvent(s2, c.ev_fork, 0));
    // side stream: the polynomials and their coset evaluations
    if (pl.Lag && (r = interpolate_and_blind(s2))) return r;
    if ((r = pi_fold(s2))) return r;
    if ((r = r3_wire_cosets(s2))) return r;
    // main stream: the five commitments
    if ((r = commit_wires(0, P))) return r;
    CAP_HIP(hipEventRecord(c.ev_join, s2));
    CAP_HIP(hipStreamWaitEvent(s, c.ev_join, 0));
    return CAPGPU_OK;
  }
  static void r1_overlapped_needs(const ProvePlan& pl, const ProvingKey& K, uint32_t cnt, ProveNeeds& nd) {
    if (pl.overlap) nd.ntt(ntt3_scratch(K.log_m, (size_t)cnt * NW, pl.five));  // reserved first, the largest
  }
  int r1_body() {
    if (pl.overlap) return r1_overlapped();
    int r = pl.chunks == 1 ? r1_chunk_kernels(0, P, false) : CAPGPU_OK;
    return r ? r : r1_tail_kernels();
  }

  // ---- round 2: permutation grand product --------------------------------------------------------------
  // z's values -> its commitment.  From coefficients (jf-plonk's way): interpolate, blind, MSM on the monomial key.  From
  // evaluations (the Lagrange-form key): the MSM of the n values and the three blinders needs neither - it starts at
  // once, and the small batches of `overlap` interpolate, blind and transform z to the cosets beside it.
  int finish_and_commit_z() {
    int r;
    const hipStream_t s2 = pl.s2;
    const MsmBases* const Lag = pl.Lag;
    perm_finish(s, w.pre, w.sfx, w.den, w.inv_total, n, P, w.zpoly, ps);
    auto interpolate_and_blind = [&](hipStream_t st) -> int {
      int q = run_ntt(st, K.log_n, w.zpoly, ps, P, 1, 0);
      if (q) return q;
      launch("k_blind", k_blind<0>, dim3(P), dim3(64), 0, st, w.zpoly, ps, n, (const fe*)w.d_blind, 1u, 10u, 3u, P);
      return CAPGPU_OK;
    };
    if (Lag) {  // (the values are staged before the in-place interpolation overwrites them)
      launch("k_stage_evals", k_stage_evals, dim3(cdiv(n + 3, kThreads), P), dim3(kThreads), 0, s, (const fe*)w.zpoly, ps, n,
             (const fe*)w.d_blind, 1u, 10u, 3u, w.t);
    }
    if (!pl.overlap) {
      if ((r = interpolate_and_blind(s))) return r;
      return Lag ? run_msm(s, *Lag, w.t, n + 3, 1, 0, n + 3, P, w.comms) : run_msm(s, *pl.B, w.zpoly, ps, 1, 0, n + 3, P, w.comms);
    }
    if (!Lag && (r = interpolate_and_blind(s))) return r;  // the monomial MSM reads the blinded coefficients
    CAP_HIP(hipEventRecord(c.ev_fork, s));
    CAP_HIP(hipStreamWaitEvent(s2, c.ev_fork, 0));
    if (Lag && (r = interpolate_and_blind(s2))) return r;
    if ((r = z_cosets(s2))) return r;
    r = Lag ? run_msm(s, *Lag, w.t, n + 3, 1, 0, n + 3, P, w.comms) : run_msm(s, *pl.B, w.zpoly, ps, 1, 0, n + 3, P, w.comms);
    CAP_HIP(hipEventRecord(c.ev_join, s2));
    CAP_HIP(hipStreamWaitEvent(s, c.ev_join, 0));
    return r;
  }
  static void commit_z_needs(const ProvePlan& pl, const ProvingKey& K, uint32_t cnt, ProveNeeds& nd) {
    nd.ntt(ntt_scratch_inplace(K.ps, cnt));
    nd.msm(pl.wire_key(), K.n + 3, cnt);
  }
  int r2_body() {
    perm_numden(s, pl.coeffs ? (const fe*)w.wev : d_wires, K.sig_eval, sig_of, dom_n->tw_fwd, w.chal, qc29, n, P, w.num,
                w.den);
    {
      uint32_t nb = cdiv(n, kScanBlock);
      scan_exclusive<0, 0>(s, w.num, w.pre, n, n, P, w.scan_tot);
      scan_exclusive<0, 1>(s, w.den, w.sfx, n, n, P, w.scan_tot + (size_t)P * nb);
    }
    if (pl.inv_on_device) {
      // (the product is a function of the secret witness: the device kernel runs a fixed-length chain, as the host does)
      perm_inv_total(s, w.sfx, w.den, n, w.inv_total, P);
    } else {
      perm_total(s, w.sfx, w.den, n, w.inv_total, P);
      return CAPGPU_OK;  // the segment ends here: the host inverts the totals (run_host_transcript)
    }
    return finish_and_commit_z();
  }

  // ---- round 3: quotient polynomial (its six coset transforms were enqueued behind the round 1 and 2 MSMs) ------
  int r3_body() {
    int r;
    const fe* pkc = K.pk_coset;
    if (K.recompute) {
      // reference schedule: the 18 selector / sigma polynomials are re-transformed for every proof
      for (uint32_t p = 0; p < P; p++)
        if ((r = compute_pk_coset(s, K, w.pkc))) return r;
      if ((r = compute_pk_kx(s, K, w.pkc))) return r;
      pkc = w.pkc;
    }
    const int fold = quotient_fold();
    if (fold == 2)
      CAP_HIP(hipMemset2DAsync(&w.chal29[0].beta_inv, sizeof(Chal), 0, sizeof(fe), P, s));
    // five cosets: 5n points per proof; the key's columns and the domain's tables are those of the whole domain, read at
    // every other element of block 2 (k_quotient: `it`)
    const uint32_t five = pl.five ? 1u : 0u;
    const size_t pts = pl.five ? 5 * n : m;
    if (fold)
      quotient<true>(s, P, pts, pkc, pkc_of, w.coset, dom_q->xs29, K.inv_nx1, w.chal29, qc29, m, 1u, five, w.t);
    // the direct form: for every proof (fold = 0), or behind the folded launch for the proofs it left out - beta = 0.
    // The host transcript knows whether there is one; the device transcript does not, and its launch is P x m / 256
    // workgroups that load one word and leave.
    if (!fold || fold == 2 || beta_zero_possible)
      quotient<false>(s, P, pts, pkc, pkc_of, w.coset, dom_q->xs29, K.inv_nx1, w.chal29, qc29, m, fold ? 1u : 0u, five,
                      w.t);
    // k_quotient leaves the public-input term out; it arrives here as coefficients (pi_fold), before the degree check
    if (pl.five) {
      // the top 8 coefficients from the polynomials; then what the sixth coset used to witness - that the numerator is
      // divisible by Z_H at all - is tested on the rows themselves (k_rows_verdict): bit 1 of the flags, as before
      quotient_top(s, P, w.wpoly, w.zpoly, K.coef, coef_of, dom_n->tw_fwd, w.chal, n, ps, w.top);
      launch("k_check_gates", k_check_gates, dim3(cdiv(n, kThreads), P), dim3(kThreads), 0, s,
             pl.coeffs ? (const fe*)w.wev : d_wires, (const fe*)w.d_pub, num_inputs, (const CheckKey*)w.chk_keys, n, w.chk_out);
      launch("k_rows_verdict", k_rows_verdict, dim3(cdiv(P, 64)), dim3(64), 0, s, (const CheckOut*)w.chk_out,
             (const fe*)w.pre, (const fe*)w.num, (const fe*)w.sfx, (const fe*)w.den, n, w.flags, P);
      if ((r = run_ntt3_inv5(s, K.log_m, w.t, P, w.top, w.pi))) return r;
    } else if ((r = run_ntt3_inv(s, K.log_m, w.t, P, w.pi))) {
      return r;
    }
    {
      size_t lo = NW * (n + 1) + 3;  // first index that must be zero: degree is exactly 5(n+1)+2
      check_degree(s, P, w.t, m, lo, w.flags);
    }
    return run_msm(s, *pl.B, w.t, m, NW, n + 2, n + 2, P * NW, w.comms);
  }
  static void r3_needs(const ProvePlan& pl, const ProvingKey& K, uint32_t cnt, ProveNeeds& nd) {
    if (K.recompute) nd.ntt(ntt3_scratch(K.log_m, 18));
    nd.ntt(ntt3_scratch(K.log_m, cnt, pl.five));
    nd.msm(*pl.B, K.n + 2, cnt * NW);
  }

  // ---- round 4: evaluations -------------------------------------------------------------------------------
  // what is evaluated where: pointers only, known when the call starts
  std::vector<EvalDesc> make_edesc() const {
    std::vector<EvalDesc> ed((size_t)P * 10);
    for (uint32_t p = 0; p < P; p++) {
      const fe* pz = w.pows + ((size_t)p * 4 + 0) * ps;
      const fe* pzw = w.pows + ((size_t)p * 4 + 1) * ps;
      for (int i = 0; i < NW; i++) ed[p * 10 + i] = EvalDesc{w.wpoly + ((size_t)p * NW + i) * ps, pz, (uint32_t)(n + 2), 0};
      for (int i = 0; i < NW - 1; i++)
        ed[p * 10 + NW + i] = EvalDesc{key_of(p).coef + (size_t)(NS + i) * ps, pz, (uint32_t)n, 0};
      ed[p * 10 + 9] = EvalDesc{w.zpoly + (size_t)p * ps, pzw, (uint32_t)(n + 3), 0};
    }
    return ed;
  }
  int r4_body() {
    powers(s, P * 4, w.pw, w.pows_small, w.pows, ps);
    evaluate(s, P * 10, w.edesc, n + 3, w.eval_partial, w.evals);
    return CAPGPU_OK;
  }

  // ---- round 5: linearisation + opening proofs ---------------------------------------------------------
  // the polynomials and lengths of proof p's 29 linear terms, in the order td::lin_scalars derives their scalars
  void term_polys(uint32_t p, LinTerm* T) const {
    int t = 0;
    auto add = [&](const fe* poly, size_t len) {
      T[t].poly = poly;
      T[t].len = (uint32_t)len;
      t++;
    };
    const fe* const coef = key_of(p).coef;
    for (int j = 0; j < NS; j++) add(coef + (size_t)j * ps, n);
    add(w.zpoly + (size_t)p * ps, n + 3);
    add(coef + (size_t)(NS + NW - 1) * ps, n);
    for (int j = 0; j < NW; j++) add(w.t + (size_t)p * m + (size_t)j * (n + 2), n + 2);
    for (int j = 0; j < NW; j++) add(w.wpoly + ((size_t)p * NW + j) * ps, n + 2);
    for (int j = 0; j < NW - 1; j++) add(coef + (size_t)(NS + j) * ps, n);
  }
  // batchpoly[p][0] = linear combination, batchpoly[p][1] = z polynomial
  int r5_body() {
    lincomb(s, P, w.terms, kLinTerms, w.batchpoly, 2 * ps, ps);
    pad_copy(s, w.batchpoly + ps, 2 * ps, 0, w.zpoly, ps, 0, 1, P, n + 3, ps);
    // the suffix sums go to batchpoly (its contents are dead once h is formed)
    divide_linear(s, P * 2, w.batchpoly, w.pows, ps, n + 3, w.hbuf, w.scan_tot, w.quot);
    return run_msm(s, *pl.B, w.quot, ps, 1, 0, n + 2, P * 2, w.comms);
  }
  static void r5_needs(const ProvePlan& pl, const ProvingKey& K, uint32_t cnt, ProveNeeds& nd) {
    nd.msm(*pl.B, K.n + 2, cnt * 2);
  }

  // ---- the transcript on the device: every per-call value goes up now, the five rounds are ONE run of launches (one
  // graph segment), the proofs come back in ABI layout with the degree flags, and the host waits once ----------------
  // (The uploads below come from pageable vectors, like the blinders and public inputs of begin(): the runtime may stage
  // such a copy on the host before it returns.  They sit at the head of the call, ahead of every launch - the host is
  // never made to wait for the call's own kernels - and are not counted by capgpu_plonk_sync_stats.)
  int run_device_transcript() {
    int rc;
    if ((rc = begin())) return rc;
    const uint32_t tr_stride = pl.tr_stride;
    std::vector<uint8_t> h_pre((size_t)P * tr_stride, 0);
    std::vector<uint32_t> h_pre_len(P);
    parallel_for(P, [&](uint32_t p) {
      uint8_t* b = &h_pre[(size_t)p * tr_stride];
      size_t o = 0;
      auto put = [&](const void* src, size_t len) {
        memcpy(b + o, src, len);
        o += len;
      };
      if (rq.msgs) {
        if (rq.msgs[p] && rq.msg_lens[p]) put(rq.msgs[p], rq.msg_lens[p]);
      } else if (rq.ext_msg && rq.ext_len) {
        put(rq.ext_msg, rq.ext_len);
      }
      const ProvingKey& Kp = key_of(p);
      put(Kp.vk_bytes.data(), Kp.vk_bytes.size());
      for (size_t i = 0; i < Kp.num_inputs; i++) {
        uint8_t e[32];
        serialize_fr(fe_from_words(pub_inputs + 4 * (p * num_inputs + i)), e);
        put(e, 32);
      }
      h_pre_len[p] = (uint32_t)o;
    });
    CAP_HIP(hipMemcpyAsync(w.tr_pre, h_pre.data(), h_pre.size(), hipMemcpyHostToDevice, s));
    CAP_HIP(hipMemcpyAsync(w.tr_pre_len, h_pre_len.data(), sizeof(uint32_t) * P, hipMemcpyHostToDevice, s));
    CAP_HIP(hipMemsetAsync(w.tr_state, 0, (size_t)P * 64, s));
    const std::vector<EvalDesc> ed = make_edesc();
    CAP_HIP(hipMemcpyAsync(w.edesc, ed.data(), sizeof(EvalDesc) * ed.size(), hipMemcpyHostToDevice, s));
    std::vector<LinTerm> terms((size_t)P * kLinTerms);
    memset((void*)terms.data(), 0, sizeof(LinTerm) * terms.size());
    for (uint32_t p = 0; p < P; p++) term_polys(p, &terms[(size_t)p * kLinTerms]);
    CAP_HIP(hipMemcpyAsync(w.terms, terms.data(), sizeof(LinTerm) * terms.size(), hipMemcpyHostToDevice, s));
    const td::TrBufs tb{w.tr_state, w.tr_pre, w.tr_pre_len, w.tr_app, tr_stride};
    td::LinIn lin_base;
    memset((void*)&lin_base, 0, sizeof lin_base);
    for (int i = 0; i < NW; i++) lin_base.k[i] = K.qc.k[i];
    lin_base.n = n;
    if ((rc = seg(0, [&]() -> int {
           int r;
           if ((r = r1_body())) return r;
           launch("k_tr_comms_r1", td::k_tr_comms<1>, dim3(P), dim3(64), 0, s, tb, (const g1_jac*)w.comms, w.d_proofs, w.chal,
                  w.chal29, w.zeta, w.pw, omega, P);
           if (!pl.overlap && (r = r3_wire_cosets(s))) return r;
           if ((r = r2_body())) return r;
           launch("k_tr_comms_r2", td::k_tr_comms<2>, dim3(P), dim3(64), 0, s, tb, (const g1_jac*)w.comms, w.d_proofs, w.chal,
                  w.chal29, w.zeta, w.pw, omega, P);
           if (!pl.overlap && (r = z_cosets(s))) return r;
           if ((r = r3_body())) return r;
           launch("k_tr_comms_r3", td::k_tr_comms<3>, dim3(P), dim3(64), 0, s, tb, (const g1_jac*)w.comms, w.d_proofs, w.chal,
                  w.chal29, w.zeta, w.pw, omega, P);
           if ((r = r4_body())) return r;
           launch("k_tr_evals", td::k_tr_evals, dim3(P), dim3(64), 0, s, tb, (const fe*)w.evals, w.d_proofs,
                  (const Chal*)w.chal, (const fe*)w.zeta, w.terms, lin_base, P);
           if ((r = r5_body())) return r;
           launch("k_tr_open", td::k_tr_open, dim3(cdiv(P, 64)), dim3(64), 0, s, (const g1_jac*)w.comms, w.d_proofs, P);
           // outcome calls: the status words, and the records of failed proofs blanked before the copy below takes them
           if (rq.outcomes)
             launch("k_prove_outcomes", oc::k_prove_outcomes, dim3(P), dim3(64), 0, s, P, (const uint32_t*)w.flags,
                    faults ? (const unsigned long long*)w.chk_first : nullptr, w.status, w.d_proofs);
           return CAPGPU_OK;
         })))
      return rc;
    uint32_t* flags = h_flags;
    CAP_HIP(hipMemcpyAsync(h_proofs, w.d_proofs, proofs_bytes, hipMemcpyDeviceToHost, s));
    CAP_HIP(hipMemcpyAsync(flags, w.flags, sizeof(uint32_t) * P, hipMemcpyDeviceToHost, s));
    if (rq.outcomes) CAP_HIP(hipMemcpyAsync(h_status, w.status, sizeof(int32_t) * P, hipMemcpyDeviceToHost, s));
    CAP_HIP(wait_stream());
    trace("pb_r5_done", c.slot);
    if ((rc = take_launch_error())) return rc;
    if (rq.outcomes) {
      for (uint32_t p = 0; p < P; p++) {  // (the device applied the rule: its status word, its blanked record)
        capgpu_prove_outcome& o = rq.outcomes[p];
        memset(&o, 0, sizeof o);
        o.status = h_status[p];
        o.degree_flags = flags[p];
        if (faults) o.fault = faults[p];
      }
    } else if ((rc = degree_verdict(flags))) {
      return rc;
    }
    memcpy(rq.proofs, h_proofs, proofs_bytes);
    side_drain.armed = false;  // (every join was waited for in stream order and the stream has drained)
    return CAPGPU_OK;
  }

  // ---- the transcript on the host: between the rounds the commitments come back, the host hashes them and sends the
  // challenges ----------------------------------------------------------------------------------------------------------
  int run_host_transcript() {
    int rc;
    if ((rc = begin())) return rc;
    capgpu_proof* const proofs = rq.proofs;
    if ((rc = seg(0, [&]() -> int { return r1_body(); }))) return rc;
    // (enqueued behind the commitments while the host hashes - unless the side stream already ran them beside the MSMs)
    if ((rc = fetch_comms(P * NW, [&]() -> int {
           if (pl.overlap) return CAPGPU_OK;
           return seg(1, [&]() -> int { return r3_wire_cosets(s); });
         })))
      return rc;
    trace("pb_r1_done", c.slot);
    std::vector<Chal> chal(P);
    parallel_for(P, [&](uint32_t p) {
      for (int i = 0; i < NW; i++) {
        append_g1(tr[p], ha[p * NW + i]);
        affine_to_words(ha[p * NW + i], proofs[p].wires_poly_comms[i]);
      }
      (void)get_challenge(tr[p]);  // plookup's tau: drawn by jf-plonk even when the circuit has no lookups
      chal[p].beta = get_challenge(tr[p]);
      chal[p].gamma = get_challenge(tr[p]);
      chal[p].alpha = Fr::zero();
      chal[p].alpha2 = Fr::zero();
      chal[p].beta_inv = Fr::is_zero(chal[p].beta) ? Fr::zero() : Fr::inv(chal[p].beta);  // beta is public
      chal[p].alpha_beta5 = Fr::zero();
    });
    // (a segment replayed as a graph keeps the launches of its capture: there the direct launch always follows)
    beta_zero_possible = pl.graphs;
    for (uint32_t p = 0; p < P; p++) beta_zero_possible = beta_zero_possible || Fr::is_zero(chal[p].beta);
    CAP_HIP(hipMemcpyAsync(w.chal, chal.data(), sizeof(Chal) * P, hipMemcpyHostToDevice, s));

    if ((rc = seg(2, [&]() -> int { return r2_body(); }))) return rc;
    if (!pl.inv_on_device) {
      // 1 / prod(den) per proof on the host: P products come back (32 B each), one shared inversion (Montgomery's trick),
      // P inverses go out - a round trip of tens of microseconds against 0.17 ms of a single device thread
      std::vector<fe> pref(P);
      fe* tot = h_tot;
      CAP_HIP(hipMemcpyAsync(tot, w.inv_total, sizeof(fe) * P, hipMemcpyDeviceToHost, s));
      CAP_HIP(wait_stream());
      // (a proof whose product is zero - one of its denominators vanished, probability ~ 2^-236 - must not poison the
      // shared inversion: it is left out of the chain and gets the inverse 0, as the per-proof device inversion gave it)
      fe acc = Fr::one();
      for (uint32_t p = 0; p < P; p++) {
        pref[p] = acc;
        if (!Fr::is_zero(tot[p])) acc = Fr::mul(acc, tot[p]);
      }
      // (the product is a function of the secret witness: a fixed-length Fermat chain - 254 squarings whatever the value,
      // ~20 us once per batch - instead of the variable-time Euclidean Fr::inv the public scalars of the other rounds use)
      acc = Fr::inv_fermat(acc);
      for (uint32_t p = P; p-- > 0;) {
        if (Fr::is_zero(tot[p])) continue;
        const fe inv_p = Fr::mul(acc, pref[p]);
        acc = Fr::mul(acc, tot[p]);
        tot[p] = inv_p;
      }
      CAP_HIP(hipMemcpyAsync(w.inv_total, tot, sizeof(fe) * P, hipMemcpyHostToDevice, s));
      if ((rc = seg(7, [&]() -> int { return finish_and_commit_z(); }))) return rc;
    }
    if ((rc = fetch_comms(P, [&]() -> int {  // likewise the coset evaluations of z
           if (pl.overlap) return CAPGPU_OK;
           return seg(3, [&]() -> int { return z_cosets(s); });
         })))
      return rc;
    trace("pb_r2_done", c.slot);
    parallel_for(P, [&](uint32_t p) {
      append_g1(tr[p], ha[p]);
      affine_to_words(ha[p], proofs[p].prod_perm_poly_comm);
      chal[p].alpha = get_challenge(tr[p]);
      chal[p].alpha2 = Fr::sqr(chal[p].alpha);
      const fe b2 = Fr::sqr(chal[p].beta);
      chal[p].alpha_beta5 = Fr::mul(chal[p].alpha, Fr::mul(Fr::sqr(b2), chal[p].beta));
    });
    CAP_HIP(hipMemcpyAsync(w.chal, chal.data(), sizeof(Chal) * P, hipMemcpyHostToDevice, s));
    std::vector<Chal> chal29(P);
    parallel_for(P, [&](uint32_t p) {
      auto conv = [](const fe& a) { return Fr29::pack(Fr29::canonical(Fr29::from_ext(a))); };
      chal29[p].beta = conv(chal[p].beta);
      chal29[p].gamma = conv(chal[p].gamma);
      chal29[p].alpha = conv(chal[p].alpha);
      chal29[p].alpha2 = conv(chal[p].alpha2);
      chal29[p].beta_inv = conv(chal[p].beta_inv);
      chal29[p].alpha_beta5 = conv(chal[p].alpha_beta5);
    });
    CAP_HIP(hipMemcpyAsync(w.chal29, chal29.data(), sizeof(Chal) * P, hipMemcpyHostToDevice, s));

    if ((rc = seg(4, [&]() -> int { return r3_body(); }))) return rc;
    uint32_t* flags = h_flags;
    CAP_HIP(hipMemcpyAsync(flags, w.flags, sizeof(uint32_t) * P, hipMemcpyDeviceToHost, s));
    if ((rc = fetch_comms(P * NW))) return rc;
    trace("pb_r3_done", c.slot);
    // (an outcome call goes on through rounds 4 and 5 for every proof: a failed one is blanked at the end)
    if (!rq.outcomes && (rc = degree_verdict(flags))) return rc;
    std::vector<fe> zeta(P);
    std::vector<fe> pw((size_t)P * 4 * 24);
    parallel_for(P, [&](uint32_t p) {
      for (int i = 0; i < NW; i++) {
        append_g1(tr[p], ha[p * NW + i]);
        affine_to_words(ha[p * NW + i], proofs[p].split_quot_poly_comms[i]);
      }
      zeta[p] = get_challenge(tr[p]);
      fe bases4[4];  // zeta, zeta omega and their inverses, from one inversion
      td::zeta_bases(zeta[p], omega, bases4);
      for (int q = 0; q < 4; q++) {
        fe x = bases4[q];
        for (int b = 0; b < 24; b++) {
          pw[((size_t)p * 4 + q) * 24 + b] = x;
          x = Fr::sqr(x);
        }
      }
    });

    CAP_HIP(hipMemcpyAsync(w.pw, pw.data(), sizeof(fe) * pw.size(), hipMemcpyHostToDevice, s));
    const std::vector<EvalDesc> ed = make_edesc();
    CAP_HIP(hipMemcpyAsync(w.edesc, ed.data(), sizeof(EvalDesc) * ed.size(), hipMemcpyHostToDevice, s));
    if ((rc = seg(5, [&]() -> int { return r4_body(); }))) return rc;
    fe* evals = h_evals;
    CAP_HIP(hipMemcpyAsync(evals, w.evals, sizeof(fe) * (size_t)P * 10, hipMemcpyDeviceToHost, s));
    CAP_HIP(wait_stream());
    trace("pb_r4_done", c.slot);

    std::vector<LinTerm> terms((size_t)P * kLinTerms);
    parallel_for(P, [&](uint32_t p) {
      const fe* ev = &evals[(size_t)p * 10];
      const fe *we = ev, *se = ev + NW;
      for (int i = 0; i < 10; i++) append_fr(tr[p], ev[i]);
      for (int i = 0; i < NW; i++) fe_to_words(we[i], proofs[p].wires_evals[i]);
      for (int i = 0; i < NW - 1; i++) fe_to_words(se[i], proofs[p].wire_sigma_evals[i]);
      fe_to_words(ev[9], proofs[p].perm_next_eval);
      // the scalars of the linear terms: the derivation the device transcript runs as well (td::lin_scalars)
      td::LinIn in;
      for (int i = 0; i < 10; i++) in.ev[i] = ev[i];
      in.beta = chal[p].beta;
      in.gamma = chal[p].gamma;
      in.alpha = chal[p].alpha;
      in.alpha2 = chal[p].alpha2;
      in.zeta = zeta[p];
      in.v = get_challenge(tr[p]);
      for (int i = 0; i < NW; i++) in.k[i] = K.qc.k[i];
      in.n = n;
      fe sc[td::kLinScalars];
      td::lin_scalars(in, sc);
      LinTerm* T = &terms[(size_t)p * kLinTerms];
      term_polys(p, T);
      for (uint32_t t = 0; t < kLinTerms; t++) T[t].scalar = td::to_internal(sc[t]);  // k_lincomb is on the lazy field
    });
    CAP_HIP(hipMemcpyAsync(w.terms, terms.data(), sizeof(LinTerm) * terms.size(), hipMemcpyHostToDevice, s));
    if ((rc = seg(6, [&]() -> int { return r5_body(); }))) return rc;
    if ((rc = fetch_comms(P * 2))) return rc;
    trace("pb_r5_done", c.slot);
    for (uint32_t p = 0; p < P; p++) {
      affine_to_words(ha[p * 2], proofs[p].opening_proof);
      affine_to_words(ha[p * 2 + 1], proofs[p].shifted_opening_proof);
    }
    if (rq.outcomes) host_outcomes(flags);
    side_drain.armed = false;  // (every join was waited for in stream order and the stream has drained)
    return take_launch_error();
  }
};

}  // namespace
}  // namespace cap
