// Device-resident TurboPlonk prover, batched over P proofs that share a proving key.
//
// Replaces `jf_plonk::proof_system::PlonkKzgSnark::{preprocess, prove}` for CAP's
// circuits - call sites src/proof/transfer.rs:133 and :181-186, src/proof/mint.rs:76
// and :113, src/proof/freeze.rs:102 and :151 (algorithm: SURVEY.md §3.2 / Appendix A).
// The host keeps only what is O(1) per proof: the Keccak transcript, the challenge
// arithmetic and Jacobian -> affine of the 13 commitments.  All O(n) work - 7 iNTT(n),
// the coset transforms of the quotient step (jf-plonk: 26 of size 8n; here 7 of size 6n per
// proof, the 18 key columns being cached and the public-input term added as coefficients),
// 13 MSM, grand product, quotient, evaluations, linearisation, openings - runs on the GPU without leaving HBM between rounds.  With capgpu_plonk_set_transcript(DEVICE)
// the O(1) steps move there too (transcript_dev.hpp) and a call is enqueued whole: one host wait instead of six or seven.
//
// MI355X-first choices: a batch of P proofs is proved in lockstep so that every launch
// is P times larger (13 MSMs become 5 launches of 5P / P / 5P / 2P MSMs; NTTs are
// batched the same way); with 288 GB of HBM the proving key also keeps the coset
// evaluations of its 18 fixed polynomials resident (set CAPGPU_RECOMPUTE_PK_COSET=1 to
// re-transform them for every proof exactly as the reference schedule does).
// k_quotient is one long chain of products per coset point: column-wise multiplication schedule (field29.hpp), measured
// 16.75 -> 16.04 ms per step
#define CAP_FL_SCHED 1
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "check_kernels.hpp"
#include "coalescer.hpp"
#include "compact.hpp"
#include "compact_kernels.hpp"
#include "context.hpp"
#include "given_gather.hpp"
#include "host_util.hpp"
#include "launch.hpp"
#include "notes.hpp"
#include "params.hpp"
#include "plonk_kernels.hpp"
#include "plonk_key.hpp"
#include "prover.hpp"
#include "solve.hpp"
#include "solve_defer.hpp"
#include "tickets.hpp"
#include "transcript_dev.hpp"
#include "vars_kernels.hpp"

namespace cap {

using namespace pk;

// ---- hipGraph replay of the small-batch schedule -------------------------------------------------------------------
// One proof is ~100 kernel launches in five Fiat-Shamir rounds, most of them a few microseconds long: at batch 1 .. 16 the
// gaps between dependent launches and the host's launch calls are a visible part of the proof's latency (the reference's
// criterion bench times ONE note per iteration, benches/transfer.rs:103-105; rayon callers arrive one note at a time).
// The kernels between two host synchronisations (the transcript needs the commitments of a round before it can hand out
// the next challenge) form a SEGMENT whose launches depend on nothing but the call's signature - key, batch size, buffers:
// every per-call value (challenges, descriptors, blinders) travels through device memory written by copies that stay
// outside the segments.  The first call of a signature runs directly (it sizes the scratch buffers), the second is
// captured segment by segment (hipStreamBeginCapture ... hipGraphInstantiate), later ones replay seven hipGraphLaunch
// calls.  CAPGPU_GRAPH_MAX_BATCH (default 16; 0 = off) bounds the batch sizes that take this path.
constexpr int kGraphSegs = 8;
struct ProveGraphSig {
  uint64_t key_uid = 0, srs = 0;
  uint32_t P = 0;
  size_t num_inputs = 0;
  int form = 0;
  bool multi = false;
  const void *d_wires = nullptr, *ws = nullptr, *msm_ws = nullptr, *ntt_scratch = nullptr, *bases = nullptr;
  const void* lagrange = nullptr;  // the Lagrange-form commit key round 1 commits on (null: from coefficients)
  hipStream_t stream = nullptr;
  // rounds 1-2 with the side stream (segments 1 and 3 are then empty: their transforms were captured inside segments 0
  // and 7): a set captured one way must never be replayed the other way - round 3 would read stale coset evaluations
  bool overlap = false;
  // where the transcript runs (capgpu_plonk_set_transcript) and, on the device, the stride of its prefix array: the two
  // modes cut the schedule differently (eight segments / one), and the stride is baked into the captured launches
  int transcript = 0;
  uint32_t tr_stride = 0;
  // capgpu_plonk_prove_each*: 0 a plain call, 1 an outcome call, 2 one whose witnesses were checked first - the device
  // transcript's segment of an outcome call ends in k_prove_outcomes, which reads the check's verdicts or does not
  int outcomes = 0;
  bool five = false;  // round 3 on five of the six n-cosets (CAPGPU_QUOT_COSETS): other transforms, other launches
  bool operator==(const ProveGraphSig& o) const {
    return key_uid == o.key_uid && srs == o.srs && P == o.P && num_inputs == o.num_inputs && form == o.form &&
           multi == o.multi && d_wires == o.d_wires && ws == o.ws && msm_ws == o.msm_ws && ntt_scratch == o.ntt_scratch &&
           bases == o.bases && lagrange == o.lagrange && stream == o.stream && overlap == o.overlap && transcript == o.transcript &&
           tr_stride == o.tr_stride && outcomes == o.outcomes && five == o.five;
  }
};
struct ProveGraphSet {
  ProveGraphSig sig;
  hipGraphExec_t exec[kGraphSegs] = {};
  uint32_t seen = 0;    // calls with this signature so far
  bool broken = false;  // a capture failed: this signature stays on direct launches
  uint64_t stamp = 0;
  ProveGraphSet() = default;
  ProveGraphSet(const ProveGraphSet&) = delete;
  ProveGraphSet& operator=(const ProveGraphSet&) = delete;
  ~ProveGraphSet() { drop(); }
  void drop() {
    for (auto& e : exec)
      if (e) {
        (void)hipGraphExecDestroy(e);
        e = nullptr;
      }
  }
};
struct ProveGraphCache {
  std::vector<std::unique_ptr<ProveGraphSet>> sets;
  uint64_t clock = 0;
};
static std::atomic<uint64_t> g_graph_captured{0}, g_graph_replayed{0};
// capgpu_plonk_sync_stats: prove_batch calls, and the times they made the host wait for the proving stream
static std::atomic<uint64_t> g_prove_calls{0}, g_stream_waits{0};

static_assert(sizeof(capgpu_proof) == td::kPrBytes && offsetof(capgpu_proof, prod_perm_poly_comm) == td::kPrZ &&
                  offsetof(capgpu_proof, split_quot_poly_comms) == td::kPrQuot &&
                  offsetof(capgpu_proof, opening_proof) == td::kPrOpen &&
                  offsetof(capgpu_proof, shifted_opening_proof) == td::kPrShifted &&
                  offsetof(capgpu_proof, wires_evals) == td::kPrWireEvals &&
                  offsetof(capgpu_proof, wire_sigma_evals) == td::kPrSigmaEvals &&
                  offsetof(capgpu_proof, perm_next_eval) == td::kPrNext,
              "transcript_dev.hpp writes capgpu_proof by offset");


namespace {

// hipGraph replay is used only on a HIP runtime at least as new as the one this library was built with.  A process that
// loaded ANOTHER libamdhip64.so.7 first runs the library on that copy (same SONAME: the loader keeps the first) - PyTorch's
// wheel bundles ROCm 7.0.2's - and round 6 caught three crashes INSIDE that runtime, under stream capture / graph launch
// (tests/test_gpu_graphs.py, test_gpu_input_forms.py, test_gpu_lagrange.py; one in ~12 suite runs; never on /opt/rocm's
// 7.2 in thousands of captures: tools/gpu_capture_stress.py, the fuzz campaigns).  On an older runtime small batches launch
// directly - a few per cent of latency - unless CAPGPU_GRAPH_FORCE=1.
bool graph_runtime_ok() {
  static const bool ok = [] {
    if (env_int("CAPGPU_GRAPH_FORCE", 0) != 0) return true;
    int v = 0;
    if (hipRuntimeGetVersion(&v) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return v >= HIP_VERSION;
  }();
  return ok;
}
uint32_t graph_max_batch() {
  if (!graph_runtime_ok()) return 0;
  const int x = env_int("CAPGPU_GRAPH_MAX_BATCH", 16);
  return (uint32_t)(x < 0 ? 0 : (x > 64 ? 64 : x));
}
// the graph set of this call's signature, or nullptr when the call launches directly (first sighting, failed capture)
ProveGraphSet* graph_set_for(Context& c, const ProveGraphSig& sig) {
  if (!c.prove_graphs) c.prove_graphs = std::make_shared<ProveGraphCache>();
  ProveGraphCache& gc = *c.prove_graphs;
  gc.clock++;
  for (auto& sp : gc.sets)
    if (sp->sig == sig) {
      sp->stamp = gc.clock;
      sp->seen++;
      return sp->broken ? nullptr : sp.get();
    }
  // a new signature: it replaces a stale one of the same (key, batch, form) - a scratch buffer moved - or the least
  // recently used of 8
  ProveGraphSet* slot = nullptr;
  for (auto& sp : gc.sets)
    if (sp->sig.key_uid == sig.key_uid && sp->sig.P == sig.P && sp->sig.form == sig.form && sp->sig.multi == sig.multi &&
        sp->sig.d_wires == sig.d_wires && sp->sig.transcript == sig.transcript && sp->sig.outcomes == sig.outcomes)
      slot = sp.get();
  if (!slot && gc.sets.size() >= 8) {
    slot = gc.sets[0].get();
    for (auto& sp : gc.sets)
      if (sp->stamp < slot->stamp) slot = sp.get();
  }
  if (!slot) {
    gc.sets.emplace_back(new ProveGraphSet);
    slot = gc.sets.back().get();
  }
  if (slot->exec[0] || slot->seen) (void)hipStreamSynchronize(c.stream);  // an instantiated graph may still be running
  slot->drop();
  slot->sig = sig;
  slot->seen = 1;
  slot->broken = false;
  slot->stamp = gc.clock;
  return nullptr;  // first call with this signature: direct launches (they size every scratch buffer)
}
// runs one segment: replay, or capture + instantiate + launch, or - without a graph set - the launches themselves
template <class F>
int run_segment(Context& c, ProveGraphSet* g, int id, F&& enqueue) {
  if (!g || g->broken) return enqueue();
  hipStream_t s = c.stream;
  if (g->exec[id]) {
    CAP_HIP(hipGraphLaunch(g->exec[id], s));
    g_graph_replayed++;
    return CAPGPU_OK;
  }
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    g->broken = true;
    return enqueue();
  }
  const LaunchError before = launch_error();  // an error latched by an earlier segment of this call must survive the attempt
  c.capturing = true;
  int rc = enqueue();
  c.capturing = false;
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamEndCapture(s, &graph);
  if (rc == CAPGPU_OK && e == hipSuccess && graph && launch_error().code == before.code) {
    hipGraphExec_t ex = nullptr;
    e = hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e == hipSuccess && ex) {
      g->exec[id] = ex;
      g_graph_captured++;
      CAP_HIP(hipGraphLaunch(ex, s));
      return CAPGPU_OK;
    }
  } else if (graph) {
    (void)hipGraphDestroy(graph);
  }
  // nothing of the captured attempt has run: abandon graphs for this signature and enqueue the segment directly
  (void)hipGetLastError();
  launch_error() = before;
  g->broken = true;
  return enqueue();
}

// The per-proof host work between rounds runs on the context's own pool (host_pool.hpp).
HostPool& host_pool() {
  Context& c = ctx();
  if (!c.pool) c.pool.reset(new HostPool(HostPool::default_threads((unsigned)std::max<size_t>(num_contexts(), 1))));
  return *c.pool;
}

template <class F>
void parallel_for(uint32_t count, F&& fn) {
  HostPool& pool = host_pool();
  if (pool.size() <= 1 || count <= 1) {
    for (uint32_t i = 0; i < count; i++) fn(i);
    return;
  }
  std::function<void(uint32_t)> job = [&](uint32_t i) { fn(i); };
  pool.run(count, job);
}

}  // namespace
}  // namespace cap

// the prover proper: launch wrappers, workspace, ProvePlan / ProveRun / ProveNeeds
#include "prove_run.hpp"

namespace cap {
namespace {

// ---- witness check ---------------------------------------------------------------------------------------------------
// The reference refuses a witness that does not satisfy its circuit before it calls the SNARK, and names the constraint
// (`check_circuit_satisfiability`, src/proof/transfer.rs:167-177; mint.rs and freeze.rs likewise).  Here: two launches over
// the resident witnesses (check_kernels.hpp) against two tables a key derives on its first check.

// the selector values alone (K.chk_mu held): what the gate pass reads - the witness check's, and the row test of the
// five-coset quotient (prove_run.hpp: r3_body), which needs no index form of sigma
int key_gate_table_locked(const ProvingKey& K) {
  if (K.chk_sel) return CAPGPU_OK;
  hipStream_t s = ctx().stream;
  const size_t n = K.n;
  DevTmp<fe> sel;
  CAP_HIP(sel.alloc((size_t)NS * n));
  int rc = run_ntt_from(s, K.log_n, K.coef, K.ps, n, sel, n, NS, 0, 0);
  if (rc) return rc;
  ntt_table_to_internal(sel, sel, (size_t)NS * n, s);
  CAP_HIP(hipStreamSynchronize(s));
  if ((rc = take_launch_error())) return rc;
  K.chk_sel = sel.p;
  sel.p = nullptr;
  return CAPGPU_OK;
}
int key_gate_table(const ProvingKey& K) {
  std::lock_guard<std::mutex> lk(K.chk_mu);
  return key_gate_table_locked(K);
}

}  // namespace

// selector values on the domain and the index form of sigma, on the current context's stream; synchronous
int key_check_tables(const ProvingKey& K) {
  std::lock_guard<std::mutex> lk(K.chk_mu);
  if (K.chk_rc <= 0) {
    if (K.chk_rc) set_error("%s", K.chk_err.c_str());
    return K.chk_rc;
  }
  Context& c = ctx();
  hipStream_t s = c.stream;
  const size_t cells = (size_t)NW * K.n;
  DevTmp<uint32_t> perm, bad;
  int rc = key_gate_table_locked(K);
  if (rc) return rc;
  if (K.chk_perm) {  // a key that knows its variable table has the index form already: no discrete logarithms
    K.chk_rc = CAPGPU_OK;
    return CAPGPU_OK;
  }
  CAP_HIP(perm.alloc(cells));
  CAP_HIP(bad.alloc(1));
  wc29::PermConsts pc;
  memset(&pc, 0, sizeof pc);
  pc.log_n = K.log_n;
  auto conv = [](const fe& a) { return Fr29::pack(Fr29::canonical(Fr29::from_ext(a))); };
  for (int i = 0; i < NW; i++) pc.kinv[i] = conv(Fr::inv(K.qc.k[i]));
  fe w = Fr::inv(ntt_root_of_unity(K.log_n));
  for (uint32_t b = 0; b < K.log_n && b < 28; b++) {
    pc.winv[b] = conv(w);
    w = Fr::sqr(w);
  }
  CAP_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), s));
  launch("k_perm_index", k_perm_index, dim3(cdiv(cells, kThreads)), dim3(kThreads), 0, s, (const fe*)K.sig_eval, pc, cells,
         perm.p, bad.p);
  uint32_t h_bad = 0;
  CAP_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  CAP_HIP(hipStreamSynchronize(s));
  if ((rc = take_launch_error())) return rc;
  if (h_bad) {
    set_error("capgpu_plonk_check_witness: sigma is not a permutation of the extended domain (a value of sigma lies in "
              "none of the five cosets k_i H)");
    K.chk_err = last_error();
    K.chk_rc = CAPGPU_ERR_INVALID_ARG;
    return K.chk_rc;
  }
  K.chk_perm = perm.p;
  perm.p = nullptr;
  K.chk_rc = CAPGPU_OK;
  return CAPGPU_OK;
}

namespace {

// check_batch's verdicts inside its d_small (the head of check_resident's Context::stage_a): they stay there until the
// next check, and an outcome call's k_prove_outcomes takes its copy of CheckOut::first from them (prove_batch)
CheckOut* check_out_at(void* d_small, uint32_t P) {
  return (CheckOut*)((char*)d_small + (sizeof(CheckKey) * P + 255) / 256 * 256);
}
size_t check_small_bytes(uint32_t P) {
  return (sizeof(CheckKey) + sizeof(CheckOut) + sizeof(uint32_t)) * (size_t)P + 768;
}

// Verdicts of P witnesses whose VALUES are resident at d_vals ([P][5][n]); d_pub: [P][pub_stride] on the device; d_small:
// check_small_bytes(P) of device scratch.  Runs on the current context's stream and waits for it.  gates_only: the values
// were gathered from variables through the keys' own tables - every copy constraint holds by construction.
int check_batch(const ProvingKey& K, const std::vector<const ProvingKey*>* keys, uint32_t P, const fe* d_vals,
                const fe* d_pub, size_t pub_stride, void* d_small, capgpu_witness_fault* faults, bool gates_only = false) {
  Context& c = ctx();
  hipStream_t s = c.stream;
  const size_t n = K.n;
  std::vector<CheckKey> hk(P);
  int rc;
  for (uint32_t p = 0; p < P; p++) {
    const ProvingKey& Kp = keys ? *(*keys)[p] : K;
    if (Kp.n != n) {
      set_error("capgpu_plonk_check_witness_multi: the keys of one batch must share the domain size");
      return CAPGPU_ERR_INVALID_ARG;
    }
    if ((p == 0 || keys) && (rc = key_check_tables(Kp))) return rc;
    hk[p] = CheckKey{Kp.chk_sel, Kp.chk_perm, (uint32_t)Kp.num_inputs, 0};
  }
  CheckKey* dk = (CheckKey*)d_small;
  CheckOut* dout = check_out_at(d_small, P);
  uint32_t* dto = (uint32_t*)((char*)dout + (sizeof(CheckOut) * P + 255) / 256 * 256);
  std::vector<CheckOut> ho(P, CheckOut{kNoFault, 0, 0});
  std::vector<uint32_t> hto(P);
  CAP_HIP(hipMemcpyAsync(dk, hk.data(), sizeof(CheckKey) * P, hipMemcpyHostToDevice, s));
  CAP_HIP(hipMemcpyAsync(dout, ho.data(), sizeof(CheckOut) * P, hipMemcpyHostToDevice, s));
  launch("k_check_gates", k_check_gates, dim3(cdiv(n, kThreads), P), dim3(kThreads), 0, s, d_vals, d_pub, pub_stride,
         (const CheckKey*)dk, n, dout);
  if (!gates_only) {
    launch("k_check_copies", k_check_copies, dim3(cdiv((size_t)NW * n, kThreads), P), dim3(kThreads), 0, s, d_vals,
           (const CheckKey*)dk, n, dout);
    launch("k_check_targets", k_check_targets, dim3(cdiv(P, 64)), dim3(64), 0, s, (const CheckKey*)dk,
           (const CheckOut*)dout, P, (size_t)NW * n, dto);
  }
  CAP_HIP(hipMemcpyAsync(ho.data(), dout, sizeof(CheckOut) * P, hipMemcpyDeviceToHost, s));
  if (!gates_only) CAP_HIP(hipMemcpyAsync(hto.data(), dto, sizeof(uint32_t) * P, hipMemcpyDeviceToHost, s));
  CAP_HIP(hipStreamSynchronize(s));
  if ((rc = take_launch_error())) return rc;
  for (uint32_t p = 0; p < P; p++) {
    capgpu_witness_fault& f = faults[p];
    memset(&f, 0, sizeof f);
    f.gates_failed = ho[p].gates;
    f.copies_failed = ho[p].copies;
    if (ho[p].first == kNoFault) continue;
    if (ho[p].first < kCopyKeyBase) {
      f.kind = 1;
      f.row = ho[p].first;
      continue;
    }
    const uint64_t cell = ho[p].first - kCopyKeyBase;
    const uint32_t to = hto[p];  // k_check_targets: the cell the constraint points to
    f.kind = 2;
    f.wire = (uint32_t)(cell / n);
    f.row = cell % n;
    f.wire2 = (uint32_t)(to / n);
    f.row2 = to % n;
  }
  return CAPGPU_OK;
}

// check_resident's layout of Context::stage_a; returns the bytes it takes (base == nullptr: sizes only)
size_t check_carve(void* base, uint32_t P, size_t pub_stride, bool coeffs, size_t n, void** small, fe** pub, fe** vals) {
  Carver k(base);
  *small = k.take<char>(check_small_bytes(P));
  *pub = k.take<fe>((size_t)P * (pub_stride ? pub_stride : 1));
  *vals = coeffs ? k.take<fe>((size_t)P * NW * n) : nullptr;
  return k.off + 256;
}

// The same for witnesses resident at d_wires in `form` with their public inputs still on the host (`pubs`: P rows of
// pub_stride elements).  Scratch: Context::stage_a.  Coefficient-form input is transformed to values out of place, into
// stage_a; d_wires is never written.
int check_resident(const ProvingKey& K, const std::vector<const ProvingKey*>* keys, uint32_t P, const fe* d_wires,
                   const uint64_t* pubs, size_t pub_stride, int form, capgpu_witness_fault* faults,
                   bool gates_only = false) {
  Context& c = ctx();
  hipStream_t s = c.stream;
  const size_t n = K.n;
  const bool coeffs = form == CAPGPU_INPUT_COEFFS;
  void* d_small = nullptr;
  fe *d_pub = nullptr, *d_vals = nullptr;
  int rc = scratch_reserve(c.stage_a, check_carve(nullptr, P, pub_stride, coeffs, n, &d_small, &d_pub, &d_vals));
  if (rc) return rc;
  (void)check_carve(c.stage_a.p, P, pub_stride, coeffs, n, &d_small, &d_pub, &d_vals);
  if (pub_stride) CAP_HIP(hipMemcpyAsync(d_pub, pubs, sizeof(fe) * P * pub_stride, hipMemcpyHostToDevice, s));
  if (coeffs) {
    if ((rc = run_ntt_from(s, K.log_n, d_wires, n, n, d_vals, n, P * NW, 0, 0))) return rc;
  } else {
    d_vals = const_cast<fe*>(d_wires);
  }
  return check_batch(K, keys, P, d_vals, d_pub, pub_stride, d_small, faults, gates_only);
}

std::string fault_text(uint32_t p, const capgpu_witness_fault& f) {
  char b[160];
  oc::fault_text(p, f, b, sizeof b);
  return b;
}
// CAPGPU_OK when every witness holds; else CAPGPU_ERR_PROOF with the number of bad proofs, the first one and its fault
int precheck_verdict(const capgpu_witness_fault* faults, uint32_t P) {
  uint32_t bad = 0, first = P;
  for (uint32_t p = 0; p < P; p++)
    if (faults[p].kind) {
      if (!bad) first = p;
      bad++;
    }
  if (!bad) return CAPGPU_OK;
  char b[320];
  oc::precheck_text(bad, P, first, faults[first], b, sizeof b);
  set_error("%s", b);
  return CAPGPU_ERR_PROOF;
}

// ---- capgpu_plonk_reserve: what prove_batch would ask of the context's scratch -----------------------------------
// The witness check is prove_batch's own step: its requests (check_resident's: stage_a, and the transform of
// coefficient-form input to values) ...
void precheck_needs(const ProvePlan& pl, const ProvingKey& K, ProveNeeds& nd) {
  if (!pl.precheck) return;
  void* a = nullptr;
  fe *b = nullptr, *v = nullptr;
  nd.stage_a = check_carve(nullptr, pl.P, K.num_inputs, pl.coeffs, K.n, &a, &b, &v);
  if (pl.coeffs) nd.ntt(ntt_scratch_from(K.log_n, (size_t)pl.P * NW));
}
// ... and with them the largest request a planned batch under K makes of every buffer (ProveRun::needs).  The device
// transcript's prefix is sized for an EMPTY init message - the caller's is not known to a reserve; it takes P * (length
// rounded up to 256) bytes of a workspace of megabytes per proof, well inside scratch_reserve's slack.
ProveNeeds prove_needs(const ProvePlan& pl, const ProvingKey& K) {
  ProveNeeds nd;
  precheck_needs(pl, K, nd);
  ProveRun::needs(pl, K, nd);
  return nd;
}

// The tail of prove_batch, behind the witness check: the workspace, the graph set of the call's signature, a driver.
int prove_planned(Context& c, const ProvingKey& K, uint32_t P, const ProveRequest& rq, const ProvePlan& pl, ProveRun& run) {
  const size_t num_inputs = rq.num_inputs;
  int rc;
  if (pl.five)  // the selector values the row test reads, once per key
    for (uint32_t p = 0; p < P && (rq.keys || p == 0); p++)
      if ((rc = key_gate_table(rq.keys ? *(*rq.keys)[p] : K))) return rc;
  // workspace
  if ((rc = scratch_reserve(c.prove_ws, carve(nullptr, K, P, num_inputs, pl.coeffs, pl.tr_stride).total))) return rc;
  run.w = carve(c.prove_ws.p, K, P, num_inputs, pl.coeffs, pl.tr_stride);
  // the check's device-side verdicts, for k_prove_outcomes: out of the check's scratch into the workspace (outside the
  // segments, like every per-call value; nothing has touched stage_a since the check)
  if (run.faults && pl.dev_tr)
    CAP_HIP(hipMemcpy2DAsync(run.w.chk_first, sizeof(unsigned long long), &check_out_at(c.stage_a.p, P)->first,
                             sizeof(CheckOut), sizeof(unsigned long long), P, hipMemcpyDeviceToDevice, c.stream));
  if (pl.graphs) {
    ProveGraphSig sig;
    sig.key_uid = K.uid;
    sig.srs = K.srs_handle;
    sig.P = P;
    sig.num_inputs = num_inputs;
    sig.form = rq.form;
    sig.multi = rq.keys != nullptr;
    sig.d_wires = rq.d_wires;
    sig.ws = c.prove_ws.p;
    sig.msm_ws = c.msm_ws.p;
    sig.ntt_scratch = c.ntt_scratch.p;
    sig.bases = pl.B->ext;
    sig.lagrange = pl.Lag ? pl.Lag->ext : nullptr;
    sig.stream = c.stream;
    sig.overlap = pl.overlap;
    sig.transcript = pl.dev_tr ? CAPGPU_TRANSCRIPT_DEVICE : CAPGPU_TRANSCRIPT_HOST;
    sig.tr_stride = pl.tr_stride;
    sig.outcomes = rq.outcomes ? (run.faults ? 2 : 1) : 0;
    sig.five = pl.five;
    run.gs = graph_set_for(c, sig);
  }
  return pl.dev_tr ? run.run_device_transcript() : run.run_host_transcript();
}

// ---- batch compaction (capgpu_plonk_set_compaction; the plan: compact.hpp, the kernel: compact_kernels.hpp) ------------
// An outcome call whose witnesses were checked knows, before the prover has reserved anything, which proofs will be blanked
// at the end.  With the mode on it proves the P' survivors as a batch of P' - the refused ones cost their check, not a proof.
std::atomic<int> g_compact{-1};  // -1: the process default (CAPGPU_COMPACT=1 turns it on)
std::atomic<uint64_t> g_compact_calls{0}, g_compact_dropped{0}, g_compact_rows{0};  // capgpu_plonk_compaction_stats
bool compaction_on() {
  static const int env_default = env_int("CAPGPU_COMPACT", 0) != 0 ? 1 : 0;
  const int m = g_compact.load(std::memory_order_relaxed);
  return (m < 0 ? env_default : m) != 0;
}
static_assert(sizeof(CheckKey) >= sizeof(uint2), "the move table takes the place of the check's key array");

// The survivors of an outcome call of P proofs of which the check refused `bad` (0 < bad < P), proved as a batch of their
// own.  *ran stays false - and nothing has been touched - when this call is one that runs uncompacted: `_dev` columns
// below the copy threshold.  The rows the prover reads are moved by ONE launch of k_move_rows, whose table is a per-call
// value: it is uploaded and the kernel launched here, outside the captured segments, so the segments of the smaller batch
// depend on the call's signature alone (P = P', an outcome call without verdicts of its own).
//   * columns in library staging (host-resident input, already copied for the check; gathered columns of the variable
//     form, whose value vectors are not read again): the plan's moves, in place;
//   * `_dev` evals / coeffs: the caller's buffer is never written - the survivors' rows are copied into Context::stage_b
//     (P' moves, dst = i) when cp::copy_route_pays.
int prove_compacted(Context& c, const ProvingKey& K, uint32_t P, const ProveRequest& rq,
                    const std::vector<capgpu_witness_fault>& faults, uint32_t bad, bool* ran) {
  *ran = false;
  const uint32_t S = P - bad;
  const size_t n = K.n, row16 = sizeof(fe) * NW * n / sizeof(uint4);
  const bool in_place = rq.d_wires == (const fe*)c.stage_b.p;
  if (!in_place && (!cp::copy_route_pays(bad, S) || ((uintptr_t)rq.d_wires & (sizeof(uint4) - 1)))) return CAPGPU_OK;
  std::vector<uint8_t> refused(P);
  for (uint32_t p = 0; p < P; p++) refused[p] = faults[p].kind != 0;
  const cp::Plan plan = cp::compact_plan(refused.data(), P);
  const std::vector<uint32_t>& orig = plan.orig;
  int rc;
  std::vector<uint2> table;
  fe* cols = const_cast<fe*>(rq.d_wires);
  if (in_place) {
    for (const cp::Move& mv : plan.moves) table.push_back(make_uint2(mv.src, mv.dst));
  } else {
    if ((rc = scratch_reserve(c.stage_b, wires_stage_bytes(S, n)))) return rc;
    cols = (fe*)c.stage_b.p;
    for (uint32_t i = 0; i < S; i++) table.push_back(make_uint2(orig[i], i));
  }
  if (!table.empty()) {
    // (the head of the check's scratch - its key array: the check has been waited for)
    uint2* d_table = (uint2*)c.stage_a.p;
    CAP_HIP(hipMemcpyAsync(d_table, table.data(), sizeof(uint2) * table.size(), hipMemcpyHostToDevice, c.stream));
    launch("k_move_rows", k_move_rows, dim3(cdiv(row16, kThreads), (uint32_t)std::min<size_t>(table.size(), 65535)),
           dim3(kThreads), 0, c.stream, (const uint4*)rq.d_wires, (uint4*)cols, row16, (const uint2*)d_table,
           (uint32_t)table.size());
  }
  // the compacted request: everything per proof reordered by `orig`, results into temporaries of P'
  std::vector<const ProvingKey*> keys2;
  size_t ni2 = rq.num_inputs;
  if (rq.keys) {
    ni2 = 0;
    for (uint32_t i = 0; i < S; i++) {
      keys2.push_back((*rq.keys)[orig[i]]);
      ni2 = std::max(ni2, keys2[i]->num_inputs);  // (rows of the survivors' largest count, as prove_batch wants them)
    }
  }
  const ProvingKey& K2 = rq.keys ? *keys2[0] : K;
  std::vector<uint64_t> pubs2((size_t)4 * ni2 * S + 4, 0), blind2((size_t)4 * 13 * S);
  std::vector<const uint8_t*> msgs2(S, nullptr);
  std::vector<size_t> lens2(S, 0);
  size_t longest = 0;
  for (uint32_t i = 0; i < S; i++) {
    const uint32_t p = orig[i];
    if (ni2) memcpy(&pubs2[(size_t)4 * ni2 * i], rq.pub_inputs + (size_t)4 * rq.num_inputs * p, 32 * ni2);
    memcpy(&blind2[(size_t)4 * 13 * i], rq.blinders + (size_t)4 * 13 * p, 32 * 13);
    if (rq.msgs) {
      msgs2[i] = rq.msgs[p];
      lens2[i] = rq.msg_lens[p];
    }
    const ProvingKey& Kp = rq.keys ? *keys2[i] : K;
    const size_t ml = rq.msgs ? (rq.msgs[p] ? rq.msg_lens[p] : 0) : (rq.ext_msg ? rq.ext_len : 0);
    longest = std::max(longest, ml + Kp.vk_bytes.size() + 32 * Kp.num_inputs);
  }
  std::vector<capgpu_proof> proofs2(S);
  std::vector<capgpu_prove_outcome> outcomes2(S);
  ProveRequest r2 = rq;
  r2.d_wires = cols;
  r2.h_wires = nullptr;  // resident since the check
  r2.pub_inputs = ni2 ? pubs2.data() : nullptr;
  r2.num_inputs = ni2;
  r2.blinders = blind2.data();
  r2.msgs = rq.msgs ? msgs2.data() : nullptr;
  r2.msg_lens = rq.msgs ? lens2.data() : nullptr;
  r2.keys = rq.keys ? &keys2 : nullptr;
  r2.proofs = proofs2.data();
  r2.outcomes = outcomes2.data();
  ProvePlan pl2;
  if ((rc = make_plan(c, K2, S, rq.form, false, longest, false, &pl2))) return rc;
  pl2.precheck = false;  // these witnesses have been checked
  ProveRun run2(c, pl2, K2, r2);
  if ((rc = prove_planned(c, K2, S, r2, pl2, run2))) return rc;
  for (uint32_t i = 0; i < S; i++) {
    rq.proofs[orig[i]] = proofs2[i];
    rq.outcomes[orig[i]] = outcomes2[i];
  }
  // a dropped proof was never proved: its fault, an all-ones record, no degree flags - as when every witness is refused
  for (uint32_t p = 0; p < P; p++)
    if (refused[p]) oc::finish_outcome(0, &faults[p], &rq.outcomes[p], &rq.proofs[p]);
  g_compact_calls.fetch_add(1, std::memory_order_relaxed);
  g_compact_dropped.fetch_add(bad, std::memory_order_relaxed);
  g_compact_rows.fetch_add(table.size(), std::memory_order_relaxed);
  *ran = true;
  return CAPGPU_OK;
}

// The rule for the keys of one batch, stated once: they share the domain size and - `same_srs` - the SRS; `no_recompute`
// refuses a key of the reference-schedule test mode (ProvingKey::recompute) as well.  Reports the common n and the row length
// of the batch's public inputs, the largest num_inputs among the keys.  `who` opens the message.
struct KeySet {
  size_t n = 0, max_inputs = 0;
};
int key_set(const char* who, const ProvingKey* const* keys, size_t count, bool same_srs, bool no_recompute, KeySet* out) {
  *out = KeySet{};
  for (size_t i = 0; i < count; i++) {
    const ProvingKey &K = *keys[0], &Kp = *keys[i];
    if (Kp.n != K.n || (same_srs && Kp.srs_handle != K.srs_handle) || (no_recompute && (Kp.recompute || K.recompute))) {
      set_error("%s: the keys of one batch must share the domain size and the SRS", who);
      return CAPGPU_ERR_INVALID_ARG;
    }
    out->n = K.n;
    out->max_inputs = std::max(out->max_inputs, Kp.num_inputs);
  }
  return CAPGPU_OK;
}

// One batch of P proofs under K (mixed keys: K = keys[0]) on the calling thread's context - see ProveRequest for the
// arguments, ProvePlan for the modes and ProveRun for the schedule.
int prove_batch(const ProvingKey& K, uint32_t P, const ProveRequest& rq) {
  Context& c = ctx();
  trace("pb_begin", c.slot, P);
  struct TraceEnd {
    int slot;
    ~TraceEnd() { trace("pb_end", slot); }
  } trace_end{c.slot};
  // host-resident witnesses are copied on the context's copy stream straight from the callers' buffers: no exit path -
  // an error return in particular - may leave such a copy in flight (the caller frees or reuses its buffer, and the
  // next call writes the same staging area)
  struct CopyDrain {
    Context& c;
    bool armed;
    ~CopyDrain() {
      if (armed && c.copy_stream) (void)hipStreamSynchronize(c.copy_stream);
    }
  } drain{c, rq.h_wires != nullptr};
  const std::vector<const ProvingKey*>* const keys = rq.keys;
  const size_t num_inputs = rq.num_inputs;
  auto key_of = [&](uint32_t p) -> const ProvingKey& { return keys ? *(*keys)[p] : K; };
  if (rq.form == CAPGPU_INPUT_VARS) {
    const VarsIn* const vin = rq.vin;
    for (uint32_t p = 0; p < P && (keys || p == 0); p++) {
      if (key_lacks_table(key_of(p))) return CAPGPU_ERR_INVALID_ARG;
      if (!vin || key_of(p).num_vars > vin->stride) {
        set_error("capgpu_plonk_prove: rows of %zu variables given, the key of proof %u has %zu", vin ? vin->stride : (size_t)0,
                  p, key_of(p).num_vars);
        return CAPGPU_ERR_INVALID_ARG;
      }
    }
  }
  if (keys) {
    KeySet ks;
    if (int rc = key_set("capgpu_plonk_prove_multi", keys->data(), P, true, true, &ks)) return rc;
    if (num_inputs != ks.max_inputs) {
      set_error("capgpu_plonk_prove_multi: rows of %zu public inputs given, the keys need %zu", num_inputs, ks.max_inputs);
      return CAPGPU_ERR_INVALID_ARG;
    }
  } else if (num_inputs != K.num_inputs) {
    set_error("capgpu_plonk_prove: %zu public inputs given, key expects %zu", num_inputs, K.num_inputs);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (const int ss = comm_shard_slot(); ss >= 0 && ss != c.slot) {
    set_error("capgpu_plonk_prove: commitment MSMs are sharded over the communicator of context %d (capgpu_plonk_shard_msm); "
              "this call runs on context %d and would prove unsharded while its peers wait", ss, c.slot);
    return CAPGPU_ERR_INVALID_ARG;
  }
  size_t longest = 0;  // the longest transcript prefix: init message || vk_bytes || public inputs
  for (uint32_t p = 0; p < P; p++) {
    const size_t ml = rq.msgs ? (rq.msgs[p] ? rq.msg_lens[p] : 0) : (rq.ext_msg ? rq.ext_len : 0);
    longest = std::max(longest, ml + key_of(p).vk_bytes.size() + 32 * key_of(p).num_inputs);
  }
  ProvePlan pl;
  int rc = make_plan(c, K, P, rq.form, rq.h_wires != nullptr, longest, false, &pl);
  if (rc) return rc;
  ProveRun run(c, pl, K, rq);
  // the witness check reads whole witnesses: host-resident ones are copied now, in one go
  if (pl.precheck && rq.h_wires && (rc = run.copy_input(0, P, c.stream))) return rc;
  // variable form with the values resident (a caller's device buffer, or copied a moment ago): all columns at once
  if (pl.vars && !pl.r1_copies) run.gather_vars(0, P);
  std::vector<capgpu_witness_fault> faults;
  if (pl.precheck) {
    // Ahead of everything the proof itself needs - the workspace, every MSM and NTT: a refused batch has cost the
    // check's launches.  (Coefficient-form input is first transformed to values, in scratch of the check's own.)
    faults.resize(P);
    // (gathered columns satisfy every copy constraint by construction: the gate pass only)
    if ((rc = check_resident(K, keys, P, rq.d_wires, rq.pub_inputs, num_inputs, pl.vars ? CAPGPU_INPUT_EVALS : rq.form,
                             faults.data(), pl.vars)))
      return rc;
    if (!rq.outcomes) {
      if ((rc = precheck_verdict(faults.data(), P))) return rc;
    } else {
      // an outcome call keeps the verdicts and goes on - unless EVERY witness was refused: then nothing is left to prove
      run.faults = faults.data();
      uint32_t bad = 0;
      for (uint32_t p = 0; p < P; p++) bad += faults[p].kind != 0;
      if (bad == P) {
        for (uint32_t p = 0; p < P; p++) oc::finish_outcome(0, &faults[p], &rq.outcomes[p], &rq.proofs[p]);
        return CAPGPU_OK;
      }
      // capgpu_plonk_set_compaction: the refused ones leave the batch here, before the prover reserves its workspace
      if (bad && compaction_on()) {
        bool ran = false;
        if ((rc = prove_compacted(c, K, P, rq, faults, bad, &ran)) || ran) return rc;
      }
    }
  }
  return prove_planned(c, K, P, rq, pl, run);
}

}  // namespace

// everything derived from the coefficient table: constants of the quotient kernel, 1 / (n (x - 1)) on the coset,
// and the cached coset evaluations of the 18 fixed polynomials
int key_finish_tables(hipStream_t s, ProvingKey& K) {
  const size_t n = K.n, m = K.m;
  int rc;
  const uint64_t five[4] = {5, 0, 0, 0};
  K.qc.g = Fr::to_mont(fe_from_words(five));
  for (int i = 0; i < NW; i++) K.qc.k[i] = Fr::to_mont(fe_from_words(K_CANON[i]));
  {
    uint32_t e_n[8] = {(uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0, 0, 0, 0, 0, 0};
    fe gn = Fr::pow(K.qc.g, e_n);
    const Ntt3Domain* dq = nullptr;
    if ((rc = get_domain3(K.log_m, &dq))) return rc;
    fe w6 = Fr::pow(dq->omega, e_n);  // omega_m^n: a primitive 6th root of unity (m = 6n)
    fe x = gn;
    for (int i = 0; i < 8; i++) K.qc.zh_inv[i] = Fr::zero();
    for (int i = 0; i < 6; i++) {
      K.qc.zh_inv[i] = Fr::inv(Fr::sub(x, Fr::one()));
      x = Fr::mul(x, w6);
    }
  }
  const Ntt3Domain* dom_m = nullptr;
  if ((rc = get_domain3(K.log_m, &dom_m))) return rc;
  launch("k_inv_nx1", k_inv_nx1, dim3(cdiv(m, kThreads)), dim3(kThreads), 0, s, K.inv_nx1, (const fe*)dom_m->xs_ext,
         fr_from_u64((uint64_t)n), m);
  ntt_table_to_internal(K.inv_nx1, K.inv_nx1, m, s);
  {
    auto conv = [](const fe& a) { return Fr29::pack(Fr29::canonical(Fr29::from_ext(a))); };
    K.qc29.g = conv(K.qc.g);
    for (int i = 0; i < NW; i++) K.qc29.k[i] = conv(K.qc.k[i]);
    for (int i = 0; i < 8; i++) K.qc29.zh_inv[i] = conv(K.qc.zh_inv[i]);
  }
  if (!K.recompute) {
    CAP_HIP(hipMalloc(&K.pk_coset, sizeof(fe) * kPkcCols * m));
    if ((rc = compute_pk_coset(s, K, K.pk_coset))) return rc;
    if ((rc = compute_pk_kx(s, K, K.pk_coset))) return rc;
  }
  return CAPGPU_OK;
}

namespace {

// ---- coalescing of concurrent single-proof calls ----------------------------------------------------------------
// The reference proves notes under rayon (`into_par_iter()`, src/utils/params_builder.rs:194-226): many host threads
// each calling prove() for ONE note.  Behind one device and one process lock those calls would run one after the
// other at single-proof latency (4 ms each, the chip mostly idle).  With coalescing switched on
// (capgpu_plonk_set_coalescing) the calls that arrive for the same proving key while the device is busy - or within a
// short window - are gathered and proved as ONE device batch; every caller gets its own proof and its own error code.
struct ProveReq {
  uint64_t pk;
  const uint64_t* wires;
  const uint64_t* pubs;
  size_t num_inputs;
  const uint8_t* msg;
  size_t msg_len;
  const uint64_t* blinders;
  capgpu_proof* out;
  int form = CAPGPU_INPUT_EVALS;  // the requests of one gathered batch share it (it is part of the group id)
  int rc = CAPGPU_OK;
  std::string err;
  bool done = false;
  // the caller's own copy of its witness on the device, started when the call arrived (StagePool); null: not staged
  const void* d_wires = nullptr;
  hipEvent_t staged = nullptr;  // recorded behind that copy
  // capgpu_plonk_prove_given_one / _io_one (kind != kWires): `wires` stays null, the values the circuit is given come in
  // its place; the requests of one gathered batch share the kind too (it is part of the group id)
  enum Kind { kWires = 0, kGiven, kGivenIo };
  Kind kind = kWires;
  const uint64_t* given = nullptr;
  size_t num_given = 0;
  capgpu_prove_outcome* outcome = nullptr;
  capgpu_solve_status* solved = nullptr;  // optional
  uint64_t* pub_out = nullptr;            // kGivenIo: the caller's row of computed public inputs
};

// OPTIONAL (CAPGPU_COALESCE_PRESTAGE=1; off by default): witnesses of coalesced single-proof calls copied to the device BY
// THEIR CALLERS, when the call arrives - into a slot of this pool, on the pool's streams - instead of by the leader once
// the batch has been gathered.  The copy of a 24 .. 40 proof batch (3 - 4.5 ms at 5.2 MB per proof) sits at the head of
// every batch with nothing of that batch running, a tenth of its lifetime; staged, the batch starts from device memory
// (one device-to-device copy per request into its contiguous input array) and a caller's latency drops by those
// milliseconds (50 -> 45 ms with 64 closed-loop callers).  THROUGHPUT does not move (profiles/phase_trace_r06.md: 0.875 of
// the resident rate either way): the link needs the same 4 ms for the batch's 200 MB wherever the copy is issued, the
// callers now come back spread over those milliseconds, and the batches that form are smaller.  One physical device only
// (the slot must live where the batch will run); slots are scratch for capgpu_trim / capgpu_set_memory_limit.
struct StageSlot {
  void* d = nullptr;
  hipEvent_t ev = nullptr;
  size_t bytes = 0;
  hipStream_t stream = nullptr;  // one of the pool's copy streams (callers copy concurrently: several, round-robin)
};
struct StagePool {
  std::mutex mu;
  static constexpr int kStreams = 4;
  hipStream_t streams[kStreams] = {};
  int device = -1;
  std::vector<StageSlot> idle;
  size_t live = 0, made = 0;
  static constexpr size_t kMaxSlots = 320;
  static bool enabled() {  // (read per call: a process may switch it)
    return env_int("CAPGPU_COALESCE_PRESTAGE", 0) != 0;
  }
  // a slot of `bytes` on `dev`, or an empty one (the caller's witness then travels with the batch, as before)
  StageSlot acquire(int dev, size_t bytes) {
    std::lock_guard<std::mutex> lk(mu);
    if (device >= 0 && device != dev) return {};
    if (!streams[0]) {
      for (int i = 0; i < kStreams; i++)
        if (hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking) != hipSuccess) {
          (void)hipGetLastError();
          for (int j = 0; j < i; j++) (void)hipStreamDestroy(streams[j]);
          for (int j = 0; j < kStreams; j++) streams[j] = nullptr;
          return {};
        }
      device = dev;
    }
    for (size_t i = 0; i < idle.size(); i++)
      if (idle[i].bytes == bytes) {
        StageSlot s = idle[i];
        idle.erase(idle.begin() + (long)i);
        return s;
      }
    if (live >= kMaxSlots || !scratch_room_for(dev, bytes)) return {};
    StageSlot s;
    if (hipMalloc(&s.d, bytes) != hipSuccess || hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) {
      if (s.d) (void)hipFree(s.d);
      (void)hipGetLastError();
      return {};
    }
    s.bytes = bytes;
    s.stream = streams[made++ % kStreams];
    live++;
    scratch_account(dev, bytes, 0);
    return s;
  }
  void release(const StageSlot& s) {
    if (!s.d) return;
    std::lock_guard<std::mutex> lk(mu);
    idle.push_back(s);
  }
  size_t trim() {  // frees the idle slots (the ones in use stay with their callers)
    std::lock_guard<std::mutex> lk(mu);
    size_t freed = 0;
    for (int i = 0; i < kStreams; i++)
      if (streams[i]) (void)hipStreamSynchronize(streams[i]);
    for (StageSlot& s : idle) {
      (void)hipFree(s.d);
      (void)hipEventDestroy(s.ev);
      freed += s.bytes;
      scratch_account(device, 0, s.bytes);
      live--;
    }
    idle.clear();
    (void)hipGetLastError();
    return freed;
  }
  void reset() {  // capgpu_shutdown: nothing is in flight any more
    (void)trim();
    std::lock_guard<std::mutex> lk(mu);
    for (int i = 0; i < kStreams; i++) {
      if (streams[i]) (void)hipStreamDestroy(streams[i]);
      streams[i] = nullptr;
    }
    device = -1;
    (void)hipGetLastError();
  }
};
StagePool& stage_pool() {
  static StagePool p;
  return p;
}
// (the gathering protocol - queues, leaders, windows, the cut over two contexts - is coalescer.hpp, which also builds for
// the host alone and runs under ThreadSanitizer there: tests/cpp/coalescer_tsan.cpp)
struct Coalescer : CoalescerCore<ProveReq> {
  // (proving-key handle, input form) -> (group id, domain size of the key); handles are never reused
  std::map<uint64_t, std::pair<uint64_t, size_t>> group_of;
};
Coalescer& coalescer() {
  static Coalescer c;
  return c;
}

}  // namespace

size_t plonk_trim_staging() { return stage_pool().trim(); }
void plonk_reset_staging() {
  stage_pool().reset();
  // (capgpu_shutdown: capgpu_plonk_input_stats counts since capgpu_init)
  g_witness_h2d.store(0);
  g_gather_launches.store(0);
  g_compact_calls.store(0);  // (capgpu_plonk_compaction_stats likewise)
  g_compact_dropped.store(0);
  g_compact_rows.store(0);
  solve_stats_reset();  // (capgpu_plonk_solve_stats)
}

}  // namespace cap

namespace cap {
// ---- the extended permutation from a wire -> variable table (vars_kernels.hpp) ---------------------------------------
// d_perm[c] = the cell after c among the cells of c's variable in ascending order, the first after the last: the unique keys
// (variable << 32) | cell are sorted - bitonic network, stages inside a tile of 2048 keys in LDS, the wider ones one launch
// each - and neighbours linked.  On stream s; waits for it (the key array is scratch of this call).
int vars_build_perm(hipStream_t s, const uint32_t* d_table, size_t n, uint32_t* d_perm) {
  const size_t cells = (size_t)NW * n;
  size_t padded = kSortTile;
  while (padded < cells) padded <<= 1;
  DevTmp<unsigned long long> keys;
  CAP_HIP(keys.alloc(padded));
  launch("k_vars_keys", k_vars_keys, dim3(cdiv(padded, kThreads)), dim3(kThreads), 0, s, d_table, cells, padded, keys.p);
  const dim3 tiles((unsigned)(padded / kSortTile));
  launch("k_vars_sort_tile", k_vars_sort_tile, tiles, dim3(kThreads), 0, s, keys.p, (size_t)2, (size_t)kSortTile);
  for (size_t k = 2 * (size_t)kSortTile; k <= padded; k <<= 1) {
    for (size_t j = k / 2; j >= kSortTile; j >>= 1)
      launch("k_vars_sort_step", k_vars_sort_step, dim3(cdiv(padded / 2, kThreads)), dim3(kThreads), 0, s, keys.p, padded / 2,
             k, j);
    launch("k_vars_sort_tile", k_vars_sort_tile, tiles, dim3(kThreads), 0, s, keys.p, k, k);
  }
  launch("k_vars_link", k_vars_link, dim3(cdiv(cells, kThreads)), dim3(kThreads), 0, s, (const unsigned long long*)keys.p,
         cells, d_perm);
  CAP_HIP(hipStreamSynchronize(s));
  return take_launch_error();
}
// index form -> sigma_i(omega^j) = k_i' omega^j' in arkworks' Montgomery form ([5 n]: what ProvingKey::sig_eval holds)
void vars_sigma_values(hipStream_t s, uint32_t log_n, const uint32_t* d_perm, fe* d_sigma) {
  SigmaConsts sc;
  memset(&sc, 0, sizeof sc);
  sc.log_n = log_n;
  for (int i = 0; i < NW; i++) sc.k[i] = Fr::to_mont(fe_from_words(K_CANON[i]));
  fe w = ntt_root_of_unity(log_n);
  for (uint32_t b = 0; b < log_n && b < 28; b++) {
    sc.wpow[b] = w;
    w = Fr::sqr(w);
  }
  const size_t cells = (size_t)NW << log_n;
  launch("k_vars_sigma", k_vars_sigma, dim3(cdiv(cells, kThreads)), dim3(kThreads), 0, s, d_perm, sc, cells, d_sigma);
}
// capgpu_plonk_key_set_vars: the table's permutation against the index form of the key's own sigma, cell for cell
void vars_first_difference(hipStream_t s, const uint32_t* d_perm, const uint32_t* d_key_perm, size_t cells,
                           unsigned long long* d_first) {
  launch("k_vars_differ", k_vars_differ, dim3(cdiv(cells, kThreads)), dim3(kThreads), 0, s, d_perm, d_key_perm, cells, d_first);
}
}  // namespace cap

using namespace cap;

extern "C" {

static bool bad_form(int form) {
  if (form == CAPGPU_INPUT_EVALS || form == CAPGPU_INPUT_COEFFS || form == CAPGPU_INPUT_VARS) return false;
  set_error("capgpu_plonk: input_form %d is none of CAPGPU_INPUT_EVALS (0), CAPGPU_INPUT_COEFFS (1), CAPGPU_INPUT_VARS (2)",
            form);
  return true;
}
// CAPGPU_INPUT_VARS asks for a key with a table: refused before the device is touched.  *stride_out: elements per proof of
// the input in `form` under the keys of one call - 5 n, or the largest num_vars among them.
static int input_stride(const uint64_t* pks, int count, int form, size_t n, size_t* stride_out) {
  *stride_out = (size_t)NW * n;
  if (form != CAPGPU_INPUT_VARS) return CAPGPU_OK;
  size_t stride = 0;
  for (int i = 0; i < count; i++) {
    std::shared_ptr<ProvingKey> K;
    int rc = home_key(pks[i], &K);
    if (rc) return rc;
    if (key_lacks_table(*K)) return CAPGPU_ERR_INVALID_ARG;
    stride = std::max(stride, K->num_vars);
  }
  *stride_out = stride;
  return CAPGPU_OK;
}

// ---- dealing host-buffer batches over the device contexts -------------------------------------------------------
// A batch that arrives with its witnesses in host memory names no device, so a process that drives several (capgpu_init
// with more than one id, or CAPGPU_CONTEXTS_PER_DEVICE) cuts it into contiguous parts, one per context, each proved
// from a thread of its own: proofs are independent, so the parts' proofs are bit for bit those of the undivided batch.
// A thread that bound itself to a device (capgpu_set_device) keeps its batches there.
static int deal_min() {  // proofs a part must hold at least (smaller batches stay on one context)
  return env_int("CAPGPU_DEAL_MIN", 8, 1);
}
// ... and at most two parts per DEVICE (CAPGPU_DEAL_PARTS_PER_DEVICE): two halves of a batch overlap on a GPU - one's
// copies, latency-bound launches and transcript steps under the other's issue-bound kernels - but four quarters are smaller
// launches for nothing (256 host-resident proofs on a device with four contexts: 1274 proofs/s as two parts, 1200 as four).
// The contexts beyond two are there for the coalescer's gathered batches (capgpu_init).
static size_t deal_max_parts(size_t contexts) {
  static const size_t per_device = (size_t)env_int("CAPGPU_DEAL_PARTS_PER_DEVICE", 2, 1);
  std::vector<int> seen;
  for (size_t i = 0; i < contexts; i++) {
    const int d = rt().ctxs[i]->device;
    if (std::find(seen.begin(), seen.end(), d) == seen.end()) seen.push_back(d);
  }
  const size_t devices = std::max<size_t>(seen.size(), 1);
  return devices * std::min<size_t>(per_device, std::max<size_t>(contexts / devices, 1));
}
// which contexts `parts` parts run on: the idle ones first, in slot order (a lone caller keeps to the same - warm - contexts
// call after call; concurrent callers find different ones), the round-robin cursor for the rest
static std::vector<size_t> deal_pick(size_t parts) {
  const size_t S = num_contexts();
  const uint32_t start = rt().rr.fetch_add((uint32_t)parts, std::memory_order_relaxed);
  std::vector<size_t> pick;
  for (size_t i = 0; i < S && pick.size() < parts; i++) {
    std::recursive_mutex& m = rt().ctxs[i]->mu;
    if (m.try_lock()) {
      m.unlock();
      pick.push_back(i);
    }
  }
  for (size_t k = 0; pick.size() < parts && k < S; k++) {
    const size_t i = (start + k) % S;
    if (std::find(pick.begin(), pick.end(), i) == pick.end()) pick.push_back(i);
  }
  return pick;
}
// whether a host-resident call stays whole on ONE context (pick_context's): mode A (capgpu_plonk_shard_msm: the ranks of the
// communicator prove the same batch in lock step), a thread that bound itself, a single context, an entry from inside the library
static bool deal_stays_whole(size_t S, size_t parts) {
  return comm_shard_slot() >= 0 || thread_bound_slot() >= 0 || S <= 1 || parts <= 1 || thread_entry_depth() > 0;
}
static int deal(int count, const std::function<int(int first, int cnt)>& part) {
  const size_t S = num_contexts();
  const size_t parts = std::min<size_t>(std::min<size_t>(S, deal_max_parts(S)), (size_t)std::max(count / deal_min(), 1));
  // Mode A (capgpu_plonk_shard_msm): the ranks of the communicator prove the same batch in lock step, so the batch stays
  // whole and on the communicator's context - cut over contexts, one part would run unsharded and which proofs meet in
  // an exchange would depend on a cursor the ranks do not share (pick_context sends it there)
  if (deal_stays_whole(S, parts)) {
    Context& c = pick_context();
    ScopedCtx sc(c);
    return part(0, count);
  }
  std::vector<int> rcs(parts, CAPGPU_OK);
  std::vector<std::string> errs(parts);
  const std::vector<size_t> pick = deal_pick(parts);
  H2dTurn turn;
  // (parts on different devices have a link each: only the parts of ONE device take turns)
  bool one_device = true;
  for (size_t i = 1; i < parts; i++) one_device = one_device && rt().ctxs[pick[i]]->device == rt().ctxs[pick[0]]->device;
  const bool ordered = h2d_in_part_order() && one_device && count >= 64;
  // Two parts whose copies go in part order do not start together: the first has the device to itself while the second's
  // witnesses arrive, stays ahead through every round and would end well before it, leaving the second part's last rounds
  // alone on the device (its host steps uncovered).  The first part is therefore the larger: CAPGPU_DEAL_FIRST_SIXTEENTHS
  // (default 9: 144 + 112 of 256; 8 = equal halves).
  static const uint64_t first16 = (uint64_t)env_int("CAPGPU_DEAL_FIRST_SIXTEENTHS", 9, 4, 12);
  auto cut = [&](size_t i) -> int {  // first proof of part i
    if (i == 0) return 0;
    if (i >= parts) return count;
    if (ordered && parts == 2) return (int)((uint64_t)count * first16 / 16);
    return (int)((uint64_t)count * i / parts);
  };
  auto body = [&](size_t i) {
    const int first = cut(i), last = cut(i + 1);
    ScopedCtx sc(*rt().ctxs[pick[i]]);
    if (ordered) {
      tl_h2d_turn = &turn;
      tl_h2d_index = (uint32_t)i;
    }
    rcs[i] = part(first, last - first);
    if (rcs[i]) errs[i] = last_error();
    tl_h2d_turn = nullptr;
    turn.pass((uint32_t)i);  // (whatever happened inside: a part that failed before its copies must not hold the others up)
  };
  std::vector<std::thread> th;
  for (size_t i = 1; i < parts; i++) th.emplace_back(body, i);
  body(0);
  for (auto& t : th) t.join();
  for (size_t i = 0; i < parts; i++)
    if (rcs[i]) {
      set_error("%s", errs[i].c_str());
      return rcs[i];
    }
  return CAPGPU_OK;
}

// ---- the prove entry points ------------------------------------------------------------------------------------------------
// Every form of the proving call - one key or one per proof, host or device buffers, all-or-nothing or per-proof outcomes,
// synchronous or by ticket - is described by one ProveCall.  The entry points differ in the ORDER of their checks (part of
// the ABI: tests/test_gpu_prove_args.py), so each states that order itself, out of the pieces below: bad_front / bad_rest
// (the pointers), host_part (proofs [first, first + cnt) of a host-resident call on one context - what deal() hands out and,
// whole, the body of a ticket and of a lone coalesced request), prove_resident (a device-resident call) and fill_job (a ticket).
struct ProveCall {
  const uint64_t* handles = nullptr;  // the key of proof i: handles[i], or - one_key - handles[0] for every proof
  bool one_key = false;               // (then ProveRequest::keys stays null: the single-key launches and graph signatures)
  int count = 0;
  const void* wires = nullptr;        // host memory, or - the _dev calls - a device address
  const uint64_t* pub_inputs = nullptr;
  size_t num_inputs = 0;
  const uint8_t* ext_msg = nullptr;   // one message for every proof ...
  size_t ext_msg_len = 0;
  const uint8_t* const* msgs = nullptr;  // ... or one per proof
  const size_t* msg_lens = nullptr;
  const uint64_t* blinders = nullptr;
  int form = CAPGPU_INPUT_EVALS;
  capgpu_proof* proofs = nullptr;
  capgpu_prove_outcome* outcomes = nullptr;  // capgpu_plonk_prove_each*: one record per proof
  // host-resident calls, once the first key is known:
  size_t n = 0;
  size_t stride = 0;  // elements per proof of `wires`: 5 n, or the largest num_vars among the keys of the WHOLE call
  const std::shared_ptr<ProvingKey>* homes = nullptr;  // tickets: the home of every handle, see part_key
  // capgpu_plonk_prove_given*: the input is the values each circuit is GIVEN - `wires` stays null, `form` is
  // CAPGPU_INPUT_VARS (what the solver's result is) and given_part takes the place of host_part / prove_resident
  const void* given = nullptr;            // host memory, or - given_dev - a device address
  bool given_dev = false;
  capgpu_solve_status* solved = nullptr;  // optional: the solver's verdict per proof
  size_t given_stride = 0;                // elements per proof of `given`: the largest num_given among the keys of the WHOLE call
  size_t given_own_bytes = 0;             // a gathered part (run_coalesced_given): what its callers brought - the rows are padded
                                          // by the library, capgpu_plonk_input_stats counts the callers' own bytes; 0: the rows'
  // capgpu_plonk_prove_given_io*: the public inputs are computed from the solved assignments into pub_out - which
  // pub_inputs then points at too: from the gather on, the call is a given-value call on that host buffer
  uint64_t* pub_out = nullptr;
  // capgpu_plonk_prove_notes*: host form - rows[i] is proof i's own witness block (`wires` stays null: one pointer per
  // note, no common stride); device form - dev_stride > 0 is the constant stride the blocks of a variable-form group lie at
  // in the caller's buffer, which may exceed the largest num_vars
  const uint64_t* const* rows = nullptr;
  size_t dev_stride = 0;
  size_t num_keys() const { return one_key ? 1 : (size_t)count; }
};
static const char kProve[] = "capgpu_plonk_prove", kProveMulti[] = "capgpu_plonk_prove_multi",
                  kCheckMulti[] = "capgpu_plonk_check_witness_multi";  // the names the refusals open with

// The pointer checks come in two stages: the host-buffer calls look their first key up BETWEEN them (an unknown handle
// together with a NULL `blinders` is CAPGPU_ERR_BAD_HANDLE there), every other call makes both at once.
static bool bad_front(const ProveCall& a) { return a.count < 0 || (a.count && (!a.wires || !a.handles)); }
static bool bad_rest(const ProveCall& a) {
  return a.count && (!a.blinders || !a.proofs || (a.num_inputs && !a.pub_inputs) || (a.msgs && !a.msg_lens));
}
static int bad_args(const char* who) {
  set_error("%s: bad argument", who);
  return CAPGPU_ERR_INVALID_ARG;
}

// The keys of proofs [first, first + cnt) of a call on the current context, held while the part runs.
struct PartKeys {
  std::vector<std::shared_ptr<ProvingKey>> hold;
  std::vector<const ProvingKey*> ptr;
};
static int part_keys(const ProveCall& b, int first, int cnt, PartKeys* out) {
  const size_t nk = b.one_key ? 1 : (size_t)cnt;
  out->hold.resize(nk);
  out->ptr.resize(nk);
  for (size_t i = 0; i < nk; i++) {
    const size_t at = b.one_key ? 0 : (size_t)first + i;
    if (int rc = part_key(b.handles[at], b.homes ? b.homes + at : nullptr, &out->hold[i])) return rc;
    out->ptr[i] = out->hold[i].get();
  }
  return CAPGPU_OK;
}
// `count` handles through `look` (home_key: the registry's copies, lookup_key: the current context's) and the rule over
// the keys found (key_set), as a loop over the handles meets the two: a key that breaks the rule is reported before an
// unknown handle behind it.
static int keys_in_rule(const char* who, int (*look)(uint64_t, std::shared_ptr<ProvingKey>*), const uint64_t* handles,
                        size_t count, bool same_srs, bool no_recompute, PartKeys* keys, KeySet* ks) {
  keys->hold.assign(count, nullptr);
  keys->ptr.clear();
  int rc = CAPGPU_OK;
  for (size_t i = 0; i < count && !(rc = look(handles[i], &keys->hold[i])); i++) keys->ptr.push_back(keys->hold[i].get());
  if (int rule = key_set(who, keys->ptr.data(), keys->ptr.size(), same_srs, no_recompute, ks)) return rule;
  return rc;
}
// what proofs [first, ...) of a call ask of prove_batch wherever their witnesses are; the caller adds d_wires / h_wires / vin
static ProveRequest request_of(const ProveCall& b, int first, const PartKeys& keys) {
  ProveRequest rq;
  rq.pub_inputs = b.pub_inputs ? b.pub_inputs + (size_t)4 * first * b.num_inputs : nullptr;
  rq.num_inputs = b.num_inputs;
  rq.blinders = b.blinders + (size_t)4 * 13 * first;
  rq.proofs = b.proofs + first;
  rq.ext_msg = b.ext_msg;
  rq.ext_len = b.ext_msg_len;
  rq.msgs = b.msgs ? b.msgs + first : nullptr;
  rq.msg_lens = b.msgs ? b.msg_lens + first : nullptr;
  rq.keys = b.one_key ? nullptr : &keys.ptr;
  rq.outcomes = b.outcomes ? b.outcomes + first : nullptr;
  rq.form = b.form;
  return rq;
}

// several keys: a part's rows carry `num_inputs` = the largest count among the keys of the WHOLE call; prove_batch wants
// the largest among its own keys: re-pack (into *pubs) when the part's maximum is smaller
static int part_pub_rows(const ProveCall& b, const PartKeys& keys, int cnt, ProveRequest* rq, std::vector<uint64_t>* pubs) {
  if (b.one_key) return CAPGPU_OK;
  size_t ni = 0;
  for (const ProvingKey* k : keys.ptr) ni = std::max(ni, k->num_inputs);
  if (ni > b.num_inputs) {
    set_error("capgpu_plonk_prove_multi: rows of %zu public inputs given, the keys need %zu", b.num_inputs, ni);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (ni < b.num_inputs) {
    pubs->assign((size_t)4 * ni * cnt + 4, 0);
    for (int i = 0; i < cnt; i++)
      if (ni) memcpy(&(*pubs)[(size_t)4 * ni * i], rq->pub_inputs + (size_t)4 * b.num_inputs * i, 32 * ni);
    rq->pub_inputs = pubs->data();
    rq->num_inputs = ni;
  }
  return CAPGPU_OK;
}

static int host_part(const ProveCall& b, int first, int cnt) {
  Context& c = ctx();
  Entry lk(c);
  const size_t n = b.n;
  PartKeys keys;
  int rc = part_keys(b, first, cnt, &keys);
  if (rc) return rc;
  ProveRequest rq = request_of(b, first, keys);
  std::vector<uint64_t> pubs;
  if ((rc = part_pub_rows(b, keys, cnt, &rq, &pubs))) return rc;
  const bool vars = b.form == CAPGPU_INPUT_VARS;
  rc = scratch_reserve(c.stage_b, vars ? vars_stage_bytes((size_t)cnt, n, b.stride, true) : wires_stage_bytes((size_t)cnt, n));
  if (rc) return rc;
  // the columns (variable form: the value vectors) are copied inside round 1, chunk by chunk, behind the commitments of
  // the chunk before
  std::vector<const uint64_t*> rows(cnt);
  for (int i = 0; i < cnt; i++) rows[i] = b.rows ? b.rows[first + i] : (const uint64_t*)b.wires + (size_t)4 * (first + i) * b.stride;
  const VarsIn vin{(const fe*)c.stage_b.p + (size_t)cnt * NW * n, b.stride};
  rq.d_wires = (const fe*)c.stage_b.p;
  rq.h_wires = rows.data();
  rq.vin = vars ? &vin : nullptr;
  return prove_batch(*keys.ptr[0], (uint32_t)cnt, rq);
}

// A device-resident call on the calling thread's context, whose lock the caller holds.
static int prove_resident(const ProveCall& a) {
  Context& c = ctx();
  PartKeys keys;
  int rc = part_keys(a, 0, a.count, &keys);
  if (rc) return rc;
  ProveRequest rq = request_of(a, 0, keys);
  rq.d_wires = (const fe*)a.wires;
  VarsIn vin{};
  if (a.form == CAPGPU_INPUT_VARS) {
    // the caller's buffer holds count * stride values and is only read: the columns are gathered into staging
    size_t stride = 0;
    if ((rc = input_stride(a.handles, (int)a.num_keys(), a.form, 0, &stride))) return rc;
    if (a.dev_stride) stride = a.dev_stride;
    if ((rc = scratch_reserve(c.stage_b, vars_stage_bytes((size_t)a.count, keys.ptr[0]->n, 0, false)))) return rc;
    vin = VarsIn{(const fe*)a.wires, stride};
    rq.d_wires = (const fe*)c.stage_b.p;
    rq.vin = &vin;
  }
  return prove_batch(*keys.ptr[0], (uint32_t)a.count, rq);
}

// ---- proving from given values (capgpu_plonk_prove_given*) -------------------------------------------------------------
static const char kProveGiven[] = "capgpu_plonk_prove_given";
// Context::stage_b of `cnt` proofs from given values: the columns and, behind them, the value vectors - the layout of the
// variable form in library staging (vars_stage_bytes), which the solver fills instead of a copy -, then the solver's status
// words, its witness lists (calls with several keys), - host-resident values only - the staged given rows and - the _io
// calls, pub_stride > 0 - the rows of computed public inputs.
struct GivenStage {
  fe *cols = nullptr, *vars = nullptr, *given = nullptr, *pub = nullptr, *side = nullptr;
  unsigned long long* status = nullptr;
  uint32_t* which = nullptr;
  size_t bytes = 0;
};
static GivenStage given_carve(void* base, size_t cnt, size_t n, size_t var_stride, size_t given_stride, bool host,
                              size_t pub_stride = 0, size_t side_elems = 0) {
  GivenStage g;
  Carver k(base);
  g.cols = k.take<fe>(cnt * NW * n + cnt * var_stride);  // (one piece: VarsIn of a staged call starts where the columns end)
  g.vars = base ? g.cols + cnt * NW * n : nullptr;
  g.status = k.take<unsigned long long>(cnt);
  g.which = k.take<uint32_t>(cnt);
  if (host) g.given = k.take<fe>(cnt * given_stride + 1);
  if (pub_stride) g.pub = k.take<fe>(cnt * pub_stride);
  if (side_elems) g.side = k.take<fe>(side_elems);  // (keys in the DEFERRED form: the solver's denominators)
  g.bytes = k.off + 256;
  return g;
}
// The pinned result area of such a part: the prover's own in either transcript home (its carving starts at the base),
// and behind it the status words, which come back with the proofs - no host wait is added for them.
static size_t given_pinned_offset(uint32_t P) {
  return (std::max(prove_pinned_bytes(P, true), prove_pinned_bytes(P, false)) + 255) / 256 * 256;
}
static size_t given_pinned_bytes(uint32_t P) { return given_pinned_offset(P) + sizeof(unsigned long long) * P + 256; }

static int no_solver(const char* who) {
  set_error("%s: the key has no solver (capgpu_plonk_key_set_given gives it one)", who);
  return CAPGPU_ERR_INVALID_ARG;
}

// Proofs [first, first + cnt) of a given-value call on the current context: stage the given rows (one copy), solve them
// on the proving stream into library scratch - one launch per distinct key, over that key's proofs -, and from there the
// variable-form outcome call on a library-owned buffer (prove_resident's request, columns and values in Context::stage_b).
static int given_part(const ProveCall& b, int first, int cnt) {
  Context& c = ctx();
  Entry lk(c);
  PartKeys keys;
  int rc = part_keys(b, first, cnt, &keys);
  if (rc) return rc;
  const sv29::Exps* ex = solve_exps();
  if (!ex) {
    set_error("%s: (r - 1) mod 5 != 1: the scalar field has no fifth-root exponent", kProveGiven);
    return CAPGPU_ERR_INVALID_ARG;
  }
  ProveRequest rq = request_of(b, first, keys);
  std::vector<uint64_t> pubs;
  const size_t io_stride = b.pub_out ? b.num_inputs : 0;  // (an _io call: the rows are not there yet - re-packed below)
  if (!b.pub_out && (rc = part_pub_rows(b, keys, cnt, &rq, &pubs))) return rc;
  // the distinct keys of the part, in order of first appearance, each with the proofs it proves
  struct KeyRun {
    const ProvingKey* K;
    SolveTables tab;
    std::shared_ptr<const SolveSched> hold;
    std::vector<uint32_t> which;
  };
  std::vector<KeyRun> runs;
  for (int i = 0; i < cnt; i++) {
    const ProvingKey* K = keys.ptr[b.one_key ? 0 : (size_t)i];
    size_t r = 0;
    while (r < runs.size() && runs[r].K != K) r++;
    if (r == runs.size()) {
      {
        std::lock_guard<std::mutex> klk(K->chk_mu);
        if (!K->solve || !K->wire_vars) return no_solver(kProveGiven);
      }
      runs.push_back(KeyRun{K, SolveTables{}, nullptr, {}});
      if ((rc = key_check_tables(*K))) return rc;
      if ((rc = solve_tables(*K, &runs[r].tab, &runs[r].hold))) return rc;
      if (runs[r].tab.num_given > b.given_stride || K->num_vars > b.stride) {
        set_error("%s: rows of %zu given values and %zu variables, the key of proof %d has %zu and %zu", kProveGiven,
                  b.given_stride, b.stride, first + i, runs[r].tab.num_given, K->num_vars);
        return CAPGPU_ERR_INVALID_ARG;
      }
    }
    runs[r].which.push_back((uint32_t)i);
  }
  const size_t n = keys.ptr[0]->n;
  const bool host = !b.given_dev;
  // (the launches of one part run one behind the other on one stream: the side buffer of the largest serves them all)
  size_t side_elems = 0;
  for (const KeyRun& r : runs) side_elems = std::max(side_elems, r.tab.side_elems(r.which.size()));
  if ((rc = scratch_reserve(c.stage_b,
                            given_carve(nullptr, (size_t)cnt, n, b.stride, b.given_stride, host, io_stride, side_elems).bytes)))
    return rc;
  if ((rc = pinned_reserve(c, given_pinned_bytes((uint32_t)cnt)))) return rc;
  const GivenStage g = given_carve(c.stage_b.p, (size_t)cnt, n, b.stride, b.given_stride, host, io_stride, side_elems);
  unsigned long long* const h_st = (unsigned long long*)((char*)c.pin_host + given_pinned_offset((uint32_t)cnt));
  hipStream_t s = c.stream;
  const fe* d_given = (const fe*)b.given + (size_t)first * b.given_stride;
  if (host) {
    const size_t bytes = sizeof(fe) * (size_t)cnt * b.given_stride;
    if (bytes) {
      CAP_HIP(hipMemcpyAsync(g.given, (const uint64_t*)b.given + (size_t)4 * first * b.given_stride, bytes,
                             hipMemcpyHostToDevice, s));
      count_witness_h2d(b.given_own_bytes ? b.given_own_bytes : bytes);
    }
    d_given = g.given;
  }
  CAP_HIP(hipMemsetAsync(g.status, 0xff, sizeof(unsigned long long) * cnt, s));
  const int setting = solve_pack_setting();
  size_t listed = 0;
  for (KeyRun& r : runs) {
    const uint32_t* d_which = nullptr;
    if (runs.size() > 1) {  // (one key: its proofs are 0 .. cnt - 1)
      uint32_t* at = g.which + listed;
      CAP_HIP(hipMemcpyAsync(at, r.which.data(), sizeof(uint32_t) * r.which.size(), hipMemcpyHostToDevice, s));
      d_which = at;
      listed += r.which.size();
    }
    const uint32_t k = (uint32_t)r.which.size();
    solve_launch_packed(s, spk::pack_for(setting, r.hold->auto_pack, k),
                        SolveLaunch{k, d_given, b.given_stride, g.vars, b.stride, g.status, d_which, g.side}, r.tab, *ex);
  }
  CAP_HIP(hipMemcpyAsync(h_st, g.status, sizeof(unsigned long long) * cnt, hipMemcpyDeviceToHost, s));
  if (io_stride) {
    // the public inputs of the solved assignments: gathered per key over its proofs (a key with fewer than the row: zeros
    // behind its own), brought to the caller's rows with the one stream wait this call adds, then the request's pub_inputs
    uint64_t* const out = b.pub_out + (size_t)4 * first * io_stride;
    const size_t bytes = sizeof(fe) * (size_t)cnt * io_stride;
    CAP_HIP(hipMemsetAsync(g.pub, 0, bytes, s));
    listed = 0;
    for (KeyRun& r : runs) {
      const uint32_t* d_which = runs.size() > 1 ? g.which + listed : nullptr;  // (the lists the solver's launches read)
      listed += r.which.size();
      pub_inputs_launch(s, (uint32_t)r.which.size(), g.vars, b.stride, r.K->wire_vars, r.K->chk_sel, n, (uint32_t)r.K->num_inputs,
                        d_which, g.pub, io_stride);
    }
    CAP_HIP(hipMemcpyAsync(out, g.pub, bytes, hipMemcpyDeviceToHost, s));
    CAP_HIP(hipStreamSynchronize(s));
    if ((rc = take_launch_error())) return rc;
    if ((rc = part_pub_rows(b, keys, cnt, &rq, &pubs))) return rc;
  }
  const VarsIn vin{g.vars, b.stride};
  rq.d_wires = g.cols;
  rq.vin = &vin;
  if ((rc = prove_batch(*keys.ptr[0], (uint32_t)cnt, rq))) return rc;
  // (the proofs are here: the stream has been waited for behind the copy above)
  if (b.solved)
    for (int i = 0; i < cnt; i++) {
      capgpu_solve_status& o = b.solved[first + i];
      memset(&o, 0, sizeof o);
      if (h_st[i] != kSolved) {
        o.kind = 1;
        o.row = h_st[i];
      }
    }
  return CAPGPU_OK;
}

// A host-resident call from its first key on: the remaining pointers, the stride, and the parts dealt over the contexts.
static int prove_dealt(const char* who, ProveCall& a) {
  std::shared_ptr<ProvingKey> K0;
  int rc = home_key(a.handles[0], &K0);
  if (rc) return rc;
  if (bad_rest(a)) return bad_args(who);
  if ((rc = input_stride(a.handles, (int)a.num_keys(), a.form, K0->n, &a.stride))) return rc;
  a.n = K0->n;
  return deal(a.count, [&](int first, int cnt) -> int { return host_part(a, first, cnt); });
}
// capgpu_plonk_prove_batch_ex / _multi_ex
static int prove_host(const char* who, ProveCall a) {
  CAP_CHECK_INIT();
  if (bad_form(a.form)) return CAPGPU_ERR_INVALID_ARG;
  if (bad_front(a)) return bad_args(who);
  if (a.count == 0) return CAPGPU_OK;
  return prove_dealt(who, a);
}
// capgpu_plonk_prove_batch_dev_ex / _multi_dev_ex
static int prove_dev(const char* who, const ProveCall& a) {
  CAP_CHECK_INIT();
  if (bad_form(a.form)) return CAPGPU_ERR_INVALID_ARG;
  Context& c = ctx();
  Entry lk(c);
  if (bad_front(a) || bad_rest(a)) return bad_args(who);
  if (a.count == 0) return CAPGPU_OK;
  return prove_resident(a);
}

int capgpu_plonk_prove_batch_ex(uint64_t pk_handle, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                                size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders,
                                int input_form, capgpu_proof* proofs_out) {
  return prove_host(kProve, ProveCall{&pk_handle, true, count, wires, pub_inputs, num_inputs, ext_msg, ext_msg_len, nullptr,
                                      nullptr, blinders, input_form, proofs_out});
}
int capgpu_plonk_prove_batch(uint64_t pk_handle, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                             size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders,
                             capgpu_proof* proofs_out) {
  return capgpu_plonk_prove_batch_ex(pk_handle, count, wires, pub_inputs, num_inputs, ext_msg, ext_msg_len, blinders,
                                     CAPGPU_INPUT_EVALS, proofs_out);
}
int capgpu_plonk_prove_batch_dev_ex(uint64_t pk_handle, int count, const void* d_wires, const uint64_t* pub_inputs,
                                    size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len,
                                    const uint64_t* blinders, int input_form, capgpu_proof* proofs_out) {
  return prove_dev(kProve, ProveCall{&pk_handle, true, count, d_wires, pub_inputs, num_inputs, ext_msg, ext_msg_len, nullptr,
                                     nullptr, blinders, input_form, proofs_out});
}
int capgpu_plonk_prove_batch_dev(uint64_t pk_handle, int count, const void* d_wires, const uint64_t* pub_inputs,
                                 size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len,
                                 const uint64_t* blinders, capgpu_proof* proofs_out) {
  return capgpu_plonk_prove_batch_dev_ex(pk_handle, count, d_wires, pub_inputs, num_inputs, ext_msg, ext_msg_len,
                                         blinders, CAPGPU_INPUT_EVALS, proofs_out);
}

// Proofs of several proving keys in one device batch (see prove_batch): pk_handles[i] is the key of proof i.
int capgpu_plonk_prove_multi_ex(const uint64_t* pk_handles, int count, const uint64_t* wires,
                                const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                capgpu_proof* proofs_out) {
  return prove_host(kProveMulti, ProveCall{pk_handles, false, count, wires, pub_inputs, num_inputs, nullptr, 0, ext_msgs,
                                           ext_msg_lens, blinders, input_form, proofs_out});
}
int capgpu_plonk_prove_multi(const uint64_t* pk_handles, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                             size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                             const uint64_t* blinders, capgpu_proof* proofs_out) {
  return capgpu_plonk_prove_multi_ex(pk_handles, count, wires, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders,
                                     CAPGPU_INPUT_EVALS, proofs_out);
}
int capgpu_plonk_prove_multi_dev_ex(const uint64_t* pk_handles, int count, const void* d_wires,
                                    const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                    const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                    capgpu_proof* proofs_out) {
  return prove_dev(kProveMulti, ProveCall{pk_handles, false, count, d_wires, pub_inputs, num_inputs, nullptr, 0, ext_msgs,
                                          ext_msg_lens, blinders, input_form, proofs_out});
}
int capgpu_plonk_prove_multi_dev(const uint64_t* pk_handles, int count, const void* d_wires, const uint64_t* pub_inputs,
                                 size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                 const uint64_t* blinders, capgpu_proof* proofs_out) {
  return capgpu_plonk_prove_multi_dev_ex(pk_handles, count, d_wires, pub_inputs, num_inputs, ext_msgs, ext_msg_lens,
                                         blinders, CAPGPU_INPUT_EVALS, proofs_out);
}

// ---- per-proof outcomes (capgpu_plonk_prove_each*) ---------------------------------------------------------------------
// The arguments of capgpu_plonk_prove_multi_ex plus one outcome record per proof; the pointer checks come before the
// device is looked for.  A call whose handles all name one key takes the single-key path with its messages per proof.
static ProveCall each_call(const uint64_t* pk_handles, int count, const void* wires, const uint64_t* pub_inputs,
                           size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                           const uint64_t* blinders, int input_form, capgpu_proof* proofs_out,
                           capgpu_prove_outcome* outcomes_out) {
  return ProveCall{pk_handles, false, count, wires, pub_inputs, num_inputs, nullptr, 0, ext_msgs, ext_msg_lens, blinders,
                   input_form, proofs_out, outcomes_out};
}
static int each_bad_args(const ProveCall& a) {
  if (bad_form(a.form)) return CAPGPU_ERR_INVALID_ARG;
  if (bad_front(a) || bad_rest(a) || (a.count && !a.outcomes)) return bad_args(kProveMulti);
  return CAPGPU_OK;
}
static bool each_one_key(const ProveCall& a) {
  for (int i = 1; i < a.count; i++)
    if (a.handles[i] != a.handles[0]) return false;
  return true;
}
// the ranks of a communicator prove in lock step (capgpu_plonk_shard_msm): there is no per-proof exit
static bool each_refused_by_sharding() {
  if (comm_shard_slot() < 0 && !comm_shard_prover()) return false;
  set_error("capgpu_plonk_prove_each: not available while capgpu_plonk_shard_msm is on (the ranks prove in lock step)");
  return true;
}

int capgpu_plonk_prove_each(const uint64_t* pk_handles, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                            size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                            const uint64_t* blinders, int input_form, capgpu_proof* proofs_out,
                            capgpu_prove_outcome* outcomes_out) {
  ProveCall a = each_call(pk_handles, count, wires, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders, input_form,
                          proofs_out, outcomes_out);
  if (int rc = each_bad_args(a)) return rc;
  CAP_CHECK_INIT();
  if (count == 0) return CAPGPU_OK;
  if (each_refused_by_sharding()) return CAPGPU_ERR_INVALID_ARG;
  a.one_key = each_one_key(a);
  return prove_dealt(kProveMulti, a);
}

int capgpu_plonk_prove_each_dev(const uint64_t* pk_handles, int count, const void* d_wires, const uint64_t* pub_inputs,
                                size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                const uint64_t* blinders, int input_form, capgpu_proof* proofs_out,
                                capgpu_prove_outcome* outcomes_out) {
  ProveCall a = each_call(pk_handles, count, d_wires, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders, input_form,
                          proofs_out, outcomes_out);
  if (int rc = each_bad_args(a)) return rc;
  CAP_CHECK_INIT();
  Context& c = ctx();
  Entry lk(c);
  if (count == 0) return CAPGPU_OK;
  if (each_refused_by_sharding()) return CAPGPU_ERR_INVALID_ARG;
  a.one_key = each_one_key(a);
  return prove_resident(a);
}


int capgpu_prove_outcome_text(const capgpu_prove_outcome* outcome, char* buf, size_t cap) {
  if (!outcome || (cap && !buf)) {
    set_error("capgpu_prove_outcome_text: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  (void)oc::outcome_text(*outcome, buf, cap);
  return CAPGPU_OK;
}

}  // extern "C"

// ---- asynchronous prove tickets ------------------------------------------------------------------------------------------
// The _async entry points check their arguments, copy what is small (messages, handles), take a reference to the key(s)
// and queue a ticket (tickets.hpp); a worker thread of the library then proves the whole batch on ONE context - the body is
// host_part with first = 0, cnt = count, not deal(): two tickets in flight are two bound callers (0.995 of the resident
// rate, profiles/phase_trace_r06.md), four quarter-parts are slower (deal_max_parts above).  Coalescing is not involved.
namespace cap {
namespace {
struct AsyncJob {
  // the call as it was submitted: wires, public inputs, blinders, proofs and outcomes are borrowed until the ticket is done;
  // handles, homes and messages are the submitter's no longer - run_ticket points them at the copies below
  ProveCall call;
  std::vector<uint64_t> pks;                       // one, or one per proof
  std::vector<std::shared_ptr<ProvingKey>> homes;  // shared ownership, as home_key gives it: [pks.size()]
  std::vector<std::vector<uint8_t>> msgs;          // call.msgs != NULL: one per proof, else [1]: the shared message
  int bound_slot = -1;                             // the submitting thread's capgpu_set_device, -1: none
  std::vector<const uint64_t*> rows;               // capgpu_plonk_prove_notes_async: the pointer per note (the blocks are borrowed)
};
// The ticket of a call whose pointers have been checked: every key is known and the set obeys the rule - what the
// synchronous call finds out on the device (prove_batch) is found out here, before anything is queued.  refuse_recompute:
// see key_set.
int fill_job(const ProveCall& a, bool refuse_recompute, AsyncJob* j) {
  const size_t nk = a.num_keys();
  PartKeys keys;
  KeySet ks;
  int rc = keys_in_rule(kProveMulti, home_key, a.handles, nk, true, refuse_recompute, &keys, &ks);
  if (rc) return rc;
  size_t given_stride = 0;
  if (a.given)  // every key needs its solver; the rows of `given` have the largest list's length
    for (const ProvingKey* K : keys.ptr) {
      std::lock_guard<std::mutex> klk(K->chk_mu);
      if (!K->solve || !K->wire_vars) return no_solver(kProveGiven);
      given_stride = std::max<size_t>(given_stride, K->solve->plan.num_given);
    }
  if (a.num_inputs != ks.max_inputs) {
    if (a.one_key) set_error("capgpu_plonk_prove: %zu public inputs given, key expects %zu", a.num_inputs, ks.max_inputs);
    else set_error("capgpu_plonk_prove_multi: rows of %zu public inputs given, the keys need %zu", a.num_inputs, ks.max_inputs);
    return CAPGPU_ERR_INVALID_ARG;
  }
  j->call = a;
  j->call.n = ks.n;
  j->call.given_stride = given_stride;
  if ((rc = input_stride(a.handles, (int)nk, a.form, ks.n, &j->call.stride))) return rc;
  j->pks.assign(a.handles, a.handles + nk);
  j->homes = std::move(keys.hold);
  j->msgs.resize(a.msgs ? (size_t)a.count : 1);
  for (size_t i = 0; i < j->msgs.size(); i++) {
    const uint8_t* m = a.msgs ? a.msgs[i] : a.ext_msg;
    const size_t len = a.msgs ? a.msg_lens[i] : a.ext_msg_len;
    if (m && len) j->msgs[i].assign(m, m + len);
  }
  j->bound_slot = thread_bound_slot();
  return CAPGPU_OK;
}
// the call of a job with its handles, homes and messages pointed at the job's own copies
struct JobCall {
  std::vector<const uint8_t*> mp;
  std::vector<size_t> ml;
  ProveCall b;
  explicit JobCall(const AsyncJob& j) : mp(j.msgs.size()), ml(j.msgs.size()), b(j.call) {
    for (size_t i = 0; i < j.msgs.size(); i++) {
      mp[i] = j.msgs[i].empty() ? nullptr : j.msgs[i].data();
      ml[i] = j.msgs[i].size();
    }
    b.handles = j.pks.data();
    b.homes = j.homes.data();
    if (b.rows) b.rows = j.rows.data();
    if (b.msgs) {
      b.msgs = mp.data();
      b.msg_lens = ml.data();
    } else {
      b.ext_msg = mp[0];
      b.ext_msg_len = ml[0];
    }
  }
};
using Tickets = TicketTable<AsyncJob>;

uint32_t async_inflight() {  // tickets of one physical device running at once (CAPGPU_ASYNC_INFLIGHT, default 2)
  static const uint32_t v = (uint32_t)env_int("CAPGPU_ASYNC_INFLIGHT", 2, 1, 16);
  return v;
}
// HIP devices behind the contexts, in slot order: a ticket's lane is the index of its device
std::vector<int> async_devices() {
  std::vector<int> seen;
  for (auto& c : rt().ctxs)
    if (std::find(seen.begin(), seen.end(), c->device) == seen.end()) seen.push_back(c->device);
  return seen;
}
// a context of `device` nobody is using right now (returned LOCKED), else nullptr
Context* try_acquire_context_on(int device) {
  Runtime& R = rt();
  const size_t n = R.ctxs.size();
  const uint32_t start = R.rr.load(std::memory_order_relaxed);
  for (size_t i = 0; i < n; i++) {
    Context* c = R.ctxs[(start + i) % n].get();
    if (c->device != device) continue;
    if (c->mu.try_lock()) {
      R.rr.store((uint32_t)((start + i + 1) % n), std::memory_order_relaxed);
      return c;
    }
  }
  return nullptr;
}

int notes_here(const ProveCall& a);  // capgpu_plonk_prove_notes_async: the groups of the call, one after the other, on this context

int run_ticket(AsyncJob& j, int lane, std::string* err) {
  Runtime& R = rt();
  const std::vector<int> devs = async_devices();
  if (!R.initialised.load(std::memory_order_acquire) || (size_t)lane >= devs.size()) {
    *err = "capgpu: not initialised (call capgpu_init first)";
    return CAPGPU_ERR_NOT_INITIALISED;
  }
  // the context: the submitter's bound slot, else a free one of the lane's device, else that device's round-robin pick
  Context* c = nullptr;
  bool locked = false;
  if (j.bound_slot >= 0 && (size_t)j.bound_slot < R.ctxs.size()) {
    c = R.ctxs[(size_t)j.bound_slot].get();
  } else if (devs.size() == 1 && (c = try_acquire_context()) != nullptr) {
    locked = true;
  } else if (devs.size() > 1 && (c = try_acquire_context_on(devs[(size_t)lane])) != nullptr) {
    locked = true;
  } else {
    std::vector<Context*> mine;
    for (auto& cp : R.ctxs)
      if (cp->device == devs[(size_t)lane]) mine.push_back(cp.get());
    c = mine[R.rr.fetch_add(1, std::memory_order_relaxed) % mine.size()];
  }
  trace("tk_run", c->slot, j.call.count);
  int rc;
  {
    ScopedCtx sc(*c);
    const JobCall jc(j);
    rc = jc.b.given ? given_part(jc.b, 0, jc.b.count) : jc.b.rows ? notes_here(jc.b) : host_part(jc.b, 0, jc.b.count);
    if (rc) *err = last_error();
  }
  if (locked) c->mu.unlock();
  return rc;
}

Tickets& tickets() {
  // (never destroyed: a process may exit without capgpu_shutdown while a worker sleeps on the table's condition variable)
  static Tickets* t = [] {
    Tickets* x = new Tickets;
    x->run = run_ticket;
    return x;
  }();
  return *t;
}
std::atomic<uint32_t> g_async_rr{0};  // lane of the next unbound ticket when several devices are bound

int submit_ticket(AsyncJob&& j, uint64_t* ticket_out) {
  const std::vector<int> devs = async_devices();
  int lane = 0;
  if (j.bound_slot >= 0) {
    const int d = rt().ctxs[(size_t)j.bound_slot]->device;
    lane = (int)(std::find(devs.begin(), devs.end(), d) - devs.begin());
  } else if (devs.size() > 1) {
    lane = (int)(g_async_rr.fetch_add(1, std::memory_order_relaxed) % devs.size());
  }
  Tickets& T = tickets();
  {
    std::lock_guard<std::mutex> lk(T.mu);
    T.limit = async_inflight();
  }
  switch (T.submit(std::move(j), lane, ticket_out)) {
    case Tickets::kOk:
      return CAPGPU_OK;
    case Tickets::kBusy:
      set_error("capgpu: %zu tickets outstanding; wait for one", Tickets::kMaxOutstanding);
      return CAPGPU_ERR_BUSY;
    default:
      set_error("capgpu: not initialised (call capgpu_init first)");
      return CAPGPU_ERR_NOT_INITIALISED;
  }
}
// the ranks of a communicator must prove in lock step (capgpu_plonk_shard_msm): no tickets then
bool async_refused_by_sharding() {
  if (comm_shard_slot() < 0 && !comm_shard_prover()) return false;
  set_error("capgpu_plonk_prove_async: not available while capgpu_plonk_shard_msm is on (the ranks prove in lock step)");
  return true;
}
}  // namespace

void plonk_async_shutdown() {
  Tickets& T = tickets();
  T.drain(CAPGPU_ERR_NOT_INITIALISED, "capgpu: shut down before this ticket ran");
  T.reset_stats();
}
}  // namespace cap

extern "C" {

// capgpu_plonk_prove_batch_async / _multi_async: the checks of the synchronous call, in its order, with its codes and
// messages (prove_host), and those it would meet on the device (fill_job)
static int prove_async(const char* who, const ProveCall& a, bool refuse_recompute, uint64_t* ticket_out) {
  CAP_CHECK_INIT();
  if (bad_form(a.form)) return CAPGPU_ERR_INVALID_ARG;
  if (bad_front(a) || !ticket_out) return bad_args(who);
  *ticket_out = 0;
  if (a.count == 0) return CAPGPU_OK;
  std::shared_ptr<ProvingKey> K0;
  int rc = home_key(a.handles[0], &K0);
  if (rc) return rc;
  if (bad_rest(a)) return bad_args(who);
  AsyncJob j;
  if ((rc = fill_job(a, refuse_recompute, &j))) return rc;
  if (async_refused_by_sharding()) return CAPGPU_ERR_INVALID_ARG;
  return submit_ticket(std::move(j), ticket_out);
}

int capgpu_plonk_prove_batch_async(uint64_t pk_handle, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                                   size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders,
                                   int input_form, capgpu_proof* proofs_out, uint64_t* ticket_out) {
  return prove_async(kProve, ProveCall{&pk_handle, true, count, wires, pub_inputs, num_inputs, ext_msg, ext_msg_len, nullptr,
                                       nullptr, blinders, input_form, proofs_out}, false, ticket_out);
}

int capgpu_plonk_prove_multi_async(const uint64_t* pk_handles, int count, const uint64_t* wires,
                                   const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                   const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                   capgpu_proof* proofs_out, uint64_t* ticket_out) {
  return prove_async(kProveMulti, ProveCall{pk_handles, false, count, wires, pub_inputs, num_inputs, nullptr, 0, ext_msgs,
                                            ext_msg_lens, blinders, input_form, proofs_out}, true, ticket_out);
}

int capgpu_plonk_prove_each_async(const uint64_t* pk_handles, int count, const uint64_t* wires,
                                  const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                  const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                  capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out, uint64_t* ticket_out) {
  ProveCall a = each_call(pk_handles, count, wires, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders, input_form,
                          proofs_out, outcomes_out);
  if (int rc = each_bad_args(a)) return rc;
  if (!ticket_out) return bad_args(kProveMulti);
  CAP_CHECK_INIT();
  *ticket_out = 0;
  if (count == 0) return CAPGPU_OK;
  if (each_refused_by_sharding()) return CAPGPU_ERR_INVALID_ARG;
  a.one_key = each_one_key(a);
  AsyncJob j;
  // (a recompute key is refused only among DIFFERENT keys: one key takes the single-key path)
  if (int rc = fill_job(a, !a.one_key, &j)) return rc;
  return submit_ticket(std::move(j), ticket_out);
}

// ---- capgpu_plonk_prove_given*: outcome calls whose input is the values each circuit is given ---------------------------
// Everything is refused before a device is touched: the pointers, then - through fill_job, the checks a ticket makes at
// submission - unknown handles, keys that break the batch's rule, a key without a solver, the row length of the public inputs.
static int given_checked(const uint64_t* pk_handles, int count, const void* given, bool given_dev, const uint64_t* pub_inputs,
                         size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                         const uint64_t* blinders, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                         capgpu_solve_status* solved_out, bool ticket, uint64_t* ticket_out, AsyncJob* j,
                         uint64_t* pub_out = nullptr, bool io = false) {
  if (io) pub_inputs = pub_out;  // (a NULL pub_inputs_out with num_inputs > 0 is refused as a NULL pub_inputs is)
  ProveCall a = each_call(pk_handles, count, nullptr, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders,
                          CAPGPU_INPUT_VARS, proofs_out, outcomes_out);
  a.given = given;
  a.given_dev = given_dev;
  a.solved = solved_out;
  a.pub_out = io ? pub_out : nullptr;
  if (count < 0 || (count && (!pk_handles || !given || !outcomes_out)) || bad_rest(a) || (ticket && !ticket_out))
    return bad_args(kProveGiven);
  CAP_CHECK_INIT();
  if (ticket) *ticket_out = 0;
  if (count == 0) return CAPGPU_OK;
  if (comm_shard_slot() >= 0 || comm_shard_prover()) {
    set_error("%s: not available while capgpu_plonk_shard_msm is on (the ranks prove in lock step)", kProveGiven);
    return CAPGPU_ERR_INVALID_ARG;
  }
  a.one_key = each_one_key(a);
  return fill_job(a, !a.one_key, j);
}

int capgpu_plonk_prove_given(const uint64_t* pk_handles, int count, const uint64_t* given, const uint64_t* pub_inputs,
                             size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                             const uint64_t* blinders, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                             capgpu_solve_status* solved_out) {
  AsyncJob j;
  if (int rc = given_checked(pk_handles, count, given, false, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders,
                             proofs_out, outcomes_out, solved_out, false, nullptr, &j))
    return rc;
  if (count == 0) return CAPGPU_OK;
  const JobCall jc(j);
  return deal(count, [&](int first, int cnt) -> int { return given_part(jc.b, first, cnt); });
}

int capgpu_plonk_prove_given_dev(const uint64_t* pk_handles, int count, const void* d_given, const uint64_t* pub_inputs,
                                 size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                 const uint64_t* blinders, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                                 capgpu_solve_status* solved_out) {
  AsyncJob j;
  if (int rc = given_checked(pk_handles, count, d_given, true, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders,
                             proofs_out, outcomes_out, solved_out, false, nullptr, &j))
    return rc;
  if (count == 0) return CAPGPU_OK;
  const JobCall jc(j);
  return given_part(jc.b, 0, count);  // on the calling thread's context, as every _dev call
}

int capgpu_plonk_prove_given_async(const uint64_t* pk_handles, int count, const uint64_t* given, const uint64_t* pub_inputs,
                                   size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                   const uint64_t* blinders, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                                   capgpu_solve_status* solved_out, uint64_t* ticket_out) {
  AsyncJob j;
  if (int rc = given_checked(pk_handles, count, given, false, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders,
                             proofs_out, outcomes_out, solved_out, true, ticket_out, &j))
    return rc;
  if (count == 0) return CAPGPU_OK;
  return submit_ticket(std::move(j), ticket_out);
}

// capgpu_plonk_prove_given_io*: one run function for the three forms - the given-value call with the public inputs computed
// (given_part's pub_out branch); the request goes through given_checked and fill_job like theirs
enum GivenIoForm { kIoHost, kIoDev, kIoAsync };
static int given_io_run(GivenIoForm form, const uint64_t* pk_handles, int count, const void* given, size_t num_inputs,
                        const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, const uint64_t* blinders,
                        uint64_t* pub_inputs_out, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                        capgpu_solve_status* solved_out, uint64_t* ticket_out) {
  AsyncJob j;
  if (int rc = given_checked(pk_handles, count, given, form == kIoDev, nullptr, num_inputs, ext_msgs, ext_msg_lens, blinders,
                             proofs_out, outcomes_out, solved_out, form == kIoAsync, ticket_out, &j, pub_inputs_out, true))
    return rc;
  if (count == 0) return CAPGPU_OK;
  if (form == kIoAsync) return submit_ticket(std::move(j), ticket_out);
  const JobCall jc(j);
  if (form == kIoDev) return given_part(jc.b, 0, count);  // on the calling thread's context, as every _dev call
  return deal(count, [&](int first, int cnt) -> int { return given_part(jc.b, first, cnt); });
}
int capgpu_plonk_prove_given_io(const uint64_t* pk_handles, int count, const uint64_t* given, size_t num_inputs,
                                const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, const uint64_t* blinders,
                                uint64_t* pub_inputs_out, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                                capgpu_solve_status* solved_out) {
  return given_io_run(kIoHost, pk_handles, count, given, num_inputs, ext_msgs, ext_msg_lens, blinders, pub_inputs_out, proofs_out,
                      outcomes_out, solved_out, nullptr);
}
int capgpu_plonk_prove_given_io_dev(const uint64_t* pk_handles, int count, const void* d_given, size_t num_inputs,
                                    const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, const uint64_t* blinders,
                                    uint64_t* pub_inputs_out, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                                    capgpu_solve_status* solved_out) {
  return given_io_run(kIoDev, pk_handles, count, d_given, num_inputs, ext_msgs, ext_msg_lens, blinders, pub_inputs_out,
                      proofs_out, outcomes_out, solved_out, nullptr);
}
int capgpu_plonk_prove_given_io_async(const uint64_t* pk_handles, int count, const uint64_t* given, size_t num_inputs,
                                      const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, const uint64_t* blinders,
                                      uint64_t* pub_inputs_out, capgpu_proof* proofs_out,
                                      capgpu_prove_outcome* outcomes_out, capgpu_solve_status* solved_out,
                                      uint64_t* ticket_out) {
  return given_io_run(kIoAsync, pk_handles, count, given, num_inputs, ext_msgs, ext_msg_lens, blinders, pub_inputs_out,
                      proofs_out, outcomes_out, solved_out, ticket_out);
}

int capgpu_wait(uint64_t ticket, uint32_t timeout_ms, int* done_out) {
  CAP_CHECK_INIT();
  if (!done_out) {
    set_error("capgpu_wait: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  *done_out = 0;
  if (ticket == 0) {  // the ticket of an empty batch
    *done_out = 1;
    return CAPGPU_OK;
  }
  int rc = CAPGPU_OK;
  std::string err;
  if (tickets().wait(ticket, timeout_ms, done_out, &rc, &err) == Tickets::kUnknown) {
    *done_out = 0;
    set_error("capgpu_wait: unknown ticket %llu (never issued, or its result was already taken)", (unsigned long long)ticket);
    return CAPGPU_ERR_BAD_HANDLE;
  }
  if (!*done_out) return CAPGPU_OK;
  if (rc) set_error("%s", err.c_str());
  return rc;
}

int capgpu_async_stats(uint64_t* submitted_out, uint64_t* completed_out, uint32_t* max_running_out) {
  CAP_CHECK_INIT();
  tickets().stats(submitted_out, completed_out, max_running_out);
  return CAPGPU_OK;
}

// Sizes, without proving anything, what a `count`-proof host-resident batch under this key would grow on context `slot`
// (-1: every context) - see prove_needs - and brings the key, the SRS and the Lagrange-form commit key there.
static int reserve_impl(uint64_t pk_handle, int count, int input_form, int slot, bool given);
int capgpu_plonk_reserve(uint64_t pk_handle, int count, int input_form, int slot) {
  return reserve_impl(pk_handle, count, input_form, slot, false);
}
// Everything capgpu_plonk_reserve(pk, count, CAPGPU_INPUT_VARS, slot) sizes, and what a given-value call adds: the staging
// of the given rows, the solved buffer and the status words (given_carve, given_pinned_bytes - the call's own
// expressions), the plan of a call whose values are resident (what the prover sees behind the solver), the key's tables.
int capgpu_plonk_reserve_given(uint64_t pk_handle, int count, int slot) {
  return reserve_impl(pk_handle, count, CAPGPU_INPUT_VARS, slot, true);
}
static int reserve_impl(uint64_t pk_handle, int count, int input_form, int slot, bool given) {
  const char* const who = given ? "capgpu_plonk_reserve_given" : "capgpu_plonk_reserve";
  CAP_CHECK_INIT();
  if (bad_form(input_form)) return CAPGPU_ERR_INVALID_ARG;
  if (count < 0 || slot < -1 || slot >= (int)num_contexts()) {
    set_error("%s: bad argument (count >= 0, slot -1 .. %zu)", who, num_contexts() - 1);
    return CAPGPU_ERR_INVALID_ARG;
  }
  std::shared_ptr<ProvingKey> K0;
  int rc = home_key(pk_handle, &K0);
  if (rc) return rc;
  if (given) {
    std::lock_guard<std::mutex> klk(K0->chk_mu);
    if (!K0->solve || !K0->wire_vars) return no_solver(who);
  }
  if (input_form == CAPGPU_INPUT_VARS && key_lacks_table(*K0)) return CAPGPU_ERR_INVALID_ARG;
  if (count == 0) return CAPGPU_OK;
  struct ScaleOne {  // exact sizes: a growth scale the thread carries (gathered batches) does not apply
    double saved = scratch_growth_scale();
    ScaleOne() { scratch_growth_scale() = 1.0; }
    ~ScaleOne() { scratch_growth_scale() = saved; }
  } scale_one;
  for (int sl = slot < 0 ? 0 : slot, end = slot < 0 ? (int)num_contexts() : slot + 1; sl < end; sl++) {
    Context& c = *rt().ctxs[(size_t)sl];
    ScopedCtx sc(c);
    Entry lk(c);
    std::shared_ptr<ProvingKey> K;
    if ((rc = lookup_key(pk_handle, &K))) return rc;
    // the plan of such a batch - it brings the SRS and the Lagrange-form commit key along; an empty init message
    ProvePlan pl;
    if ((rc = make_plan(c, *K, (uint32_t)count, input_form, true, K->vk_bytes.size() + 32 * K->num_inputs, true, &pl)))
      return rc;
    // the domain tables and the streams a first proof would create
    const NttDomain* dn = nullptr;
    const Ntt3Domain* d3 = nullptr;
    if ((rc = get_domain(K->log_n, &dn)) || (rc = quot_domains(K->log_m, &d3, &dn))) return rc;
    (void)h2d_stream();
    (void)side_stream(c);
    ProveNeeds nd = prove_needs(pl, *K);
    if (given) {
      ProvePlan pr;
      if ((rc = make_plan(c, *K, (uint32_t)count, input_form, false, K->vk_bytes.size() + 32 * K->num_inputs, true, &pr)))
        return rc;
      const ProveNeeds nr = prove_needs(pr, *K);
      nd.prove_ws = std::max(nd.prove_ws, nr.prove_ws);
      nd.msm_ws = std::max(nd.msm_ws, nr.msm_ws);
      nd.ntt_scratch = std::max(nd.ntt_scratch, nr.ntt_scratch);
      nd.stage_a = std::max(nd.stage_a, nr.stage_a);
      SolveTables tab;
      std::shared_ptr<const SolveSched> hold;
      if ((rc = key_check_tables(*K)) || (rc = solve_tables(*K, &tab, &hold))) return rc;
      // (a key whose solver derives its public inputs: the rows an _io call gathers them into, too)
      const size_t io_stride = hold->rules.flags & CAPGPU_SOLVER_DERIVE_PUBLIC ? K->num_inputs : 0;
      nd.stage_b = std::max(nd.stage_b, given_carve(nullptr, (size_t)count, K->n, K->num_vars, tab.num_given, true, io_stride,
                                                         tab.side_elems((size_t)count)).bytes);
      nd.pinned = std::max(nd.pinned, given_pinned_bytes((uint32_t)count));
    }
    if ((rc = scratch_reserve(c.stage_b, nd.stage_b))) return rc;
    if ((rc = scratch_reserve(c.stage_a, nd.stage_a))) return rc;
    if ((rc = scratch_reserve(c.prove_ws, nd.prove_ws))) return rc;
    if ((rc = scratch_reserve(c.msm_ws, nd.msm_ws))) return rc;
    if ((rc = scratch_reserve(c.ntt_scratch, nd.ntt_scratch))) return rc;
    if ((rc = pinned_reserve(c, nd.pinned))) return rc;
    CAP_HIP(hipStreamSynchronize(c.stream));
    trace("reserve", c.slot, count);
  }
  return CAPGPU_OK;
}

// ---- capgpu_plonk_prove_notes*: one call over keys of several domain sizes ---------------------------------------------
// The rule is notes_plan.hpp's: a GROUP is what one device batch may hold.  Every group becomes a ProveCall of its own
// (GroupCall: the per-proof arrays of its members, in member order) and goes down capgpu_plonk_prove_each's path - host_part
// or prove_resident - so the contract (group by group, the bytes of that call) holds by construction.
}  // extern "C"

namespace cap {
namespace {
const char kNotes[] = "capgpu_plonk_prove_notes";
std::atomic<uint64_t> g_notes_calls{0}, g_notes_groups{0}, g_notes_groups_dealt{0}, g_notes_contexts_dealt{0},
    g_notes_direct{0}, g_notes_gathered{0}, g_notes_rows{0};  // capgpu_plonk_notes_stats

// check (7): the home copy of every note's key
int notes_keys(const uint64_t* handles, int count, int form, std::vector<std::shared_ptr<ProvingKey>>* home) {
  home->assign((size_t)count, nullptr);
  std::map<uint64_t, std::shared_ptr<ProvingKey>> seen;
  for (int i = 0; i < count; i++) {
    auto it = seen.find(handles[i]);
    if (it != seen.end()) {
      (*home)[i] = it->second;
      continue;
    }
    if (int rc = home_key(handles[i], &(*home)[i])) return rc;
    const ProvingKey& K = *(*home)[i];
    if (K.recompute) {
      set_error("%s: the key of note %d re-transforms its columns for every proof (CAPGPU_RECOMPUTE_PK_COSET): such a key is "
                "proved alone", kNotes, i);
      return CAPGPU_ERR_INVALID_ARG;
    }
    if (form == CAPGPU_INPUT_VARS && key_lacks_table(K)) return CAPGPU_ERR_INVALID_ARG;
    seen.emplace(handles[i], (*home)[i]);
  }
  return CAPGPU_OK;
}
np::Plan notes_plan_of(const std::shared_ptr<ProvingKey>* home, int count, int form) {
  std::vector<np::Note> notes((size_t)count);
  for (int i = 0; i < count; i++) {
    const ProvingKey& K = *home[i];
    notes[i] = np::Note{K.n, K.srs_handle, K.num_inputs, form == CAPGPU_INPUT_VARS ? K.num_vars : (uint64_t)NW * K.n};
  }
  return np::notes_plan(notes.data(), notes.size());
}
// check (8)
int notes_rows_too_short(const ProveCall& a, const np::Plan& pl) {
  if (a.num_inputs >= pl.max_inputs) return CAPGPU_OK;
  set_error("%s: rows of %zu public inputs given, the keys need %zu", kNotes, a.num_inputs, (size_t)pl.max_inputs);
  return CAPGPU_ERR_INVALID_ARG;
}

// One group of a notes call `a` as a call of its own: everything per proof in member order - the public-input rows
// re-packed to the group's own largest count, as part_pub_rows re-packs a part's -, results into temporaries that scatter()
// hands to the caller's slots once the group has run.
struct GroupCall {
  const std::vector<uint32_t>& who;
  std::vector<uint64_t> handles, pubs, blind;
  std::vector<std::shared_ptr<ProvingKey>> homes;
  std::vector<const uint64_t*> rows;
  std::vector<const uint8_t*> msgs;
  std::vector<size_t> lens;
  std::vector<capgpu_proof> proofs;
  std::vector<capgpu_prove_outcome> outcomes;
  ProveCall b;
  GroupCall(const ProveCall& a, const std::shared_ptr<ProvingKey>* home, const np::Group& G) : who(G.members), b(a) {
    const size_t cnt = who.size(), ni = (size_t)G.max_inputs;
    handles.resize(cnt);
    homes.resize(cnt);
    pubs.assign((size_t)4 * ni * cnt + 4, 0);
    blind.resize((size_t)4 * 13 * cnt);
    proofs.resize(cnt);
    outcomes.resize(cnt);
    if (a.rows) rows.resize(cnt);
    if (a.msgs) {
      msgs.resize(cnt);
      lens.resize(cnt);
    }
    for (size_t k = 0; k < cnt; k++) {
      const size_t i = who[k];
      handles[k] = a.handles[i];
      homes[k] = home[i];
      if (ni) memcpy(&pubs[(size_t)4 * ni * k], a.pub_inputs + (size_t)4 * a.num_inputs * i, 32 * ni);
      memcpy(&blind[(size_t)4 * 13 * k], a.blinders + (size_t)4 * 13 * i, 32 * 13);
      if (a.rows) rows[k] = a.rows[i];
      if (a.msgs) {
        msgs[k] = a.msgs[i];
        lens[k] = a.msg_lens[i];
      }
    }
    b.handles = handles.data();
    b.homes = homes.data();
    b.count = (int)cnt;
    b.wires = nullptr;
    b.rows = a.rows ? rows.data() : nullptr;
    b.pub_inputs = ni ? pubs.data() : nullptr;
    b.num_inputs = ni;
    b.msgs = a.msgs ? msgs.data() : nullptr;
    b.msg_lens = a.msgs ? lens.data() : nullptr;
    b.blinders = blind.data();
    b.proofs = proofs.data();
    b.outcomes = outcomes.data();
    b.one_key = each_one_key(b);
    b.n = (size_t)G.n;
    b.stride = (size_t)G.max_row;
  }
  void scatter(const ProveCall& a) const {
    for (size_t k = 0; k < who.size(); k++) {
      a.proofs[who[k]] = proofs[k];
      a.outcomes[who[k]] = outcomes[k];
    }
  }
};

int notes_host_group(const ProveCall& a, const std::shared_ptr<ProvingKey>* home, const np::Group& G) {
  GroupCall gc(a, home, G);
  const int rc = host_part(gc.b, 0, gc.b.count);
  if (!rc) gc.scatter(a);
  return rc;
}
// the groups in run order, one after the other, on the calling thread's context; stops at the first that fails
int notes_in_turn(const ProveCall& a, const std::shared_ptr<ProvingKey>* home, const np::Plan& pl) {
  for (uint32_t g : pl.order)
    if (int rc = notes_host_group(a, home, pl.groups[g])) return rc;
  return CAPGPU_OK;
}
void notes_count_call(const np::Plan& pl) {
  g_notes_calls.fetch_add(1, std::memory_order_relaxed);
  g_notes_groups.fetch_add(pl.groups.size(), std::memory_order_relaxed);
}

// deal()'s sibling for whole groups: where deal() cuts ONE batch into contiguous parts, this hands out the groups of a
// notes call, each whole - in run order, a context that finishes taking the next -, on the contexts deal_pick names.  The
// parts of different groups take no H2D turns: their copies are of different sizes and start when their context is free.
int deal_groups(const ProveCall& a, const std::shared_ptr<ProvingKey>* home, const np::Plan& pl) {
  const size_t S = num_contexts(), G = pl.groups.size();
  const size_t parts = std::min<size_t>(std::min<size_t>(S, deal_max_parts(S)), G);
  if (deal_stays_whole(S, parts)) {
    Context& c = pick_context();
    ScopedCtx sc(c);
    return notes_in_turn(a, home, pl);
  }
  const std::vector<size_t> pick = deal_pick(parts);
  std::vector<int> rcs(G, CAPGPU_OK);
  std::vector<std::string> errs(G);
  std::atomic<size_t> next{0};
  std::atomic<bool> failed{false};  // (a failed group stops none that runs; it keeps the idle contexts from starting more)
  auto body = [&](size_t w) {
    ScopedCtx sc(*rt().ctxs[pick[w]]);
    for (size_t k; !failed.load(std::memory_order_relaxed) && (k = next.fetch_add(1)) < G;) {
      rcs[k] = notes_host_group(a, home, pl.groups[pl.order[k]]);
      if (rcs[k]) {
        errs[k] = last_error();
        failed.store(true, std::memory_order_relaxed);
      }
    }
  };
  std::vector<std::thread> th;
  for (size_t w = 1; w < parts; w++) th.emplace_back(body, w);
  body(0);
  for (auto& t : th) t.join();
  g_notes_groups_dealt.fetch_add(G, std::memory_order_relaxed);
  g_notes_contexts_dealt.fetch_add(parts, std::memory_order_relaxed);
  for (size_t k = 0; k < G; k++)
    if (rcs[k]) {
      set_error("%s", errs[k].c_str());
      return rcs[k];
    }
  return CAPGPU_OK;
}

// A checked host-form call.  One group: capgpu_plonk_prove_each's own path - the caller's arrays as they are, dealt in
// contiguous cuts - unless the rows of public inputs are longer than the group's (then through GroupCall's re-packed ones).
int notes_host(ProveCall a, const std::vector<std::shared_ptr<ProvingKey>>& home) {
  const np::Plan pl = notes_plan_of(home.data(), a.count, a.form);
  if (int rc = notes_rows_too_short(a, pl)) return rc;
  notes_count_call(pl);
  if (pl.groups.size() > 1) return deal_groups(a, home.data(), pl);
  const np::Group& G = pl.groups[0];
  a.homes = home.data();
  if (a.num_inputs == G.max_inputs) {
    a.one_key = each_one_key(a);
    a.n = (size_t)G.n;
    a.stride = (size_t)G.max_row;
    return deal(a.count, [&](int first, int cnt) -> int { return host_part(a, first, cnt); });
  }
  GroupCall gc(a, home.data(), G);
  const int rc = deal(a.count, [&](int first, int cnt) -> int { return host_part(gc.b, first, cnt); });
  if (!rc) gc.scatter(a);
  return rc;
}

// a ticket's body (run_ticket): the call whole on the worker's context, groups in run order
int notes_here(const ProveCall& a) {
  const np::Plan pl = notes_plan_of(a.homes, a.count, a.form);
  notes_count_call(pl);
  return notes_in_turn(a, a.homes, pl);
}

// Context::stage_b of a gathered group of the device form: the layout host-resident input has there (host_part) - the
// columns, which in the evals / coeffs forms ARE the gathered rows, and in the variable form the value vectors behind them
// -, then the move table of the gather's one launch.
size_t notes_stage_table_at(size_t cnt, size_t n, size_t row, bool vars) {
  return ((vars ? vars_stage_bytes(cnt, n, row, true) : wires_stage_bytes(cnt, n)) + 255) / 256 * 256;
}
size_t notes_stage_bytes(size_t cnt, size_t n, size_t row, bool vars) {
  return notes_stage_table_at(cnt, n, row, vars) + sizeof(np::MoveAt) * cnt + 256;
}

// One group of a device-form call on the calling thread's context, whose lock the caller holds.
int notes_dev_group(Context& c, const ProveCall& a, const uint64_t* offsets, const std::shared_ptr<ProvingKey>* home,
                    const np::Group& G) {
  GroupCall gc(a, home, G);
  const bool vars = a.form == CAPGPU_INPUT_VARS;
  const size_t cnt = G.members.size(), n = (size_t)G.n, cols = (size_t)NW * n, row = (size_t)G.max_row;
  uint64_t stride = 0;
  int rc;
  if (np::constant_stride(offsets, G.members.data(), cnt, vars ? 0 : cols, row, &stride)) {
    // where it lies: capgpu_plonk_prove_each_dev of the group (a `_dev` column for compaction's rule)
    gc.b.wires = (const fe*)a.wires + offsets[G.members[0]];
    gc.b.dev_stride = vars ? (size_t)stride : 0;
    g_notes_direct.fetch_add(1, std::memory_order_relaxed);
  } else {
    if ((rc = scratch_reserve(c.stage_b, notes_stage_bytes(cnt, n, row, vars)))) return rc;
    fe* const dst = (fe*)c.stage_b.p + (vars ? cnt * cols : 0);
    np::MoveAt* const d_moves = (np::MoveAt*)((char*)c.stage_b.p + notes_stage_table_at(cnt, n, row, vars));
    std::vector<np::MoveAt> moves(cnt);
    for (size_t k = 0; k < cnt; k++)
      moves[k] = np::MoveAt{offsets[G.members[k]], 2 * (uint64_t)(vars ? home[G.members[k]]->num_vars : cols)};
    CAP_HIP(hipMemcpyAsync(d_moves, moves.data(), sizeof(np::MoveAt) * cnt, hipMemcpyHostToDevice, c.stream));
    notes_move_rows(c.stream, a.wires, dst, 2 * (uint64_t)row, d_moves, (uint32_t)cnt);
    // from here the group is library staging: columns at the head of stage_b, or - variable form - gathered there
    // from the value vectors behind them (prove_resident's request with the library's buffer for the caller's)
    gc.b.wires = dst;
    gc.b.dev_stride = vars ? row : 0;
    g_notes_gathered.fetch_add(1, std::memory_order_relaxed);
    g_notes_rows.fetch_add(cnt, std::memory_order_relaxed);
  }
  if ((rc = prove_resident(gc.b))) return rc;
  gc.scatter(a);
  return CAPGPU_OK;
}
}  // namespace
}  // namespace cap

extern "C" {

static ProveCall notes_call(const uint64_t* pk_handles, int count, const uint64_t* const* wires, const void* d_wires,
                            const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                            const size_t* ext_msg_lens, const uint64_t* blinders, int input_form, capgpu_proof* proofs_out,
                            capgpu_prove_outcome* outcomes_out) {
  ProveCall a = each_call(pk_handles, count, d_wires, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders, input_form,
                          proofs_out, outcomes_out);
  a.rows = wires;
  return a;
}
// checks (1) - (3), before a device is looked for
static int notes_bad_args(const ProveCall& a, bool dev, const uint64_t* offsets, bool ticket, const uint64_t* ticket_out) {
  if (bad_form(a.form)) return CAPGPU_ERR_INVALID_ARG;
  if (a.count < 0 || (a.count && (!a.handles || (dev ? !a.wires || !offsets : !a.rows) || !a.outcomes)) || bad_rest(a) ||
      (ticket && !ticket_out))
    return bad_args(kNotes);
  for (int i = 0; !dev && i < a.count; i++)
    if (!a.rows[i]) {
      set_error("%s: wires[%d] is NULL", kNotes, i);
      return CAPGPU_ERR_INVALID_ARG;
    }
  if (dev && a.count && ((uintptr_t)a.wires & 15)) {
    set_error("%s: d_wires %p is not 16-byte aligned", kNotes, a.wires);
    return CAPGPU_ERR_INVALID_ARG;
  }
  return CAPGPU_OK;
}
static bool notes_refused_by_sharding() {
  if (comm_shard_slot() < 0 && !comm_shard_prover()) return false;
  set_error("%s: not available while capgpu_plonk_shard_msm is on (the ranks prove in lock step)", kNotes);
  return true;
}

int capgpu_plonk_prove_notes(const uint64_t* pk_handles, int count, const uint64_t* const* wires,
                             const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                             const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                             capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out) {
  const ProveCall a = notes_call(pk_handles, count, wires, nullptr, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders,
                                 input_form, proofs_out, outcomes_out);
  if (int rc = notes_bad_args(a, false, nullptr, false, nullptr)) return rc;
  CAP_CHECK_INIT();
  if (count == 0) return CAPGPU_OK;
  if (notes_refused_by_sharding()) return CAPGPU_ERR_INVALID_ARG;
  std::vector<std::shared_ptr<ProvingKey>> home;
  if (int rc = notes_keys(pk_handles, count, input_form, &home)) return rc;
  return notes_host(a, home);
}

int capgpu_plonk_prove_notes_dev(const uint64_t* pk_handles, int count, const void* d_wires, const uint64_t* wire_offsets,
                                 const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                 const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                 capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out) {
  const ProveCall a = notes_call(pk_handles, count, nullptr, d_wires, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders,
                                 input_form, proofs_out, outcomes_out);
  if (int rc = notes_bad_args(a, true, wire_offsets, false, nullptr)) return rc;
  CAP_CHECK_INIT();
  Context& c = ctx();
  Entry lk(c);
  if (count == 0) return CAPGPU_OK;
  if (notes_refused_by_sharding()) return CAPGPU_ERR_INVALID_ARG;
  std::vector<std::shared_ptr<ProvingKey>> home;
  if (int rc = notes_keys(pk_handles, count, input_form, &home)) return rc;
  const np::Plan pl = notes_plan_of(home.data(), count, input_form);
  if (int rc = notes_rows_too_short(a, pl)) return rc;
  notes_count_call(pl);
  for (uint32_t g : pl.order)
    if (int rc = notes_dev_group(c, a, wire_offsets, home.data(), pl.groups[g])) return rc;
  return CAPGPU_OK;
}

int capgpu_plonk_prove_notes_async(const uint64_t* pk_handles, int count, const uint64_t* const* wires,
                                   const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                   const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                   capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out, uint64_t* ticket_out) {
  const ProveCall a = notes_call(pk_handles, count, wires, nullptr, pub_inputs, num_inputs, ext_msgs, ext_msg_lens, blinders,
                                 input_form, proofs_out, outcomes_out);
  if (int rc = notes_bad_args(a, false, nullptr, true, ticket_out)) return rc;
  CAP_CHECK_INIT();
  *ticket_out = 0;
  if (count == 0) return CAPGPU_OK;
  if (notes_refused_by_sharding()) return CAPGPU_ERR_INVALID_ARG;
  AsyncJob j;
  if (int rc = notes_keys(pk_handles, count, input_form, &j.homes)) return rc;
  if (int rc = notes_rows_too_short(a, notes_plan_of(j.homes.data(), count, input_form))) return rc;
  // (fill_job's copies: the handles, the homes above, the messages, the pointer per note)
  j.call = a;
  j.pks.assign(pk_handles, pk_handles + count);
  j.rows.assign(wires, wires + count);
  j.msgs.resize(a.msgs ? (size_t)count : 1);
  for (size_t i = 0; a.msgs && i < j.msgs.size(); i++)
    if (a.msgs[i] && a.msg_lens[i]) j.msgs[i].assign(a.msgs[i], a.msgs[i] + a.msg_lens[i]);
  j.bound_slot = thread_bound_slot();
  return submit_ticket(std::move(j), ticket_out);
}

int capgpu_plonk_notes_plan(const uint64_t* pk_handles, int count, capgpu_notes_group* groups_out, size_t cap,
                            size_t* num_groups_out, uint32_t* group_of_out) {
  if (count < 0 || (count && !pk_handles) || (cap && !groups_out) || !num_groups_out) return bad_args("capgpu_plonk_notes_plan");
  if (!rt().initialised.load(std::memory_order_acquire)) {
    set_error("capgpu: not initialised (call capgpu_init first)");
    return CAPGPU_ERR_NOT_INITIALISED;
  }
  *num_groups_out = 0;
  if (count == 0) return CAPGPU_OK;
  std::vector<std::shared_ptr<ProvingKey>> home;
  if (int rc = notes_keys(pk_handles, count, CAPGPU_INPUT_EVALS, &home)) return rc;
  const np::Plan pl = notes_plan_of(home.data(), count, CAPGPU_INPUT_EVALS);
  *num_groups_out = pl.groups.size();
  for (size_t g = 0; g < pl.groups.size() && g < cap; g++) {
    const np::Group& G = pl.groups[g];
    groups_out[g] = capgpu_notes_group{G.srs, G.n, (uint32_t)G.members.size(), G.members[0], (uint32_t)G.max_inputs, G.run_order};
  }
  for (int i = 0; group_of_out && i < count; i++) group_of_out[i] = pl.group_of[i];
  return CAPGPU_OK;
}

int capgpu_plonk_notes_stats(capgpu_notes_stats* out) {
  if (!out) return bad_args("capgpu_plonk_notes_stats");
  *out = capgpu_notes_stats{g_notes_calls.load(),  g_notes_groups.load(),   g_notes_groups_dealt.load(), g_notes_contexts_dealt.load(),
                            g_notes_direct.load(), g_notes_gathered.load(), g_notes_rows.load()};
  return CAPGPU_OK;
}

// The largest need over the groups of such a call on context `slot` (-1: every one), host and device form: per group the
// sizes capgpu_plonk_reserve takes for its batch - the plan of host-resident and of resident input, with the group's
// largest num_vars behind the columns - and the gather's staging (notes_stage_bytes); every key is brought to the context.
int capgpu_plonk_reserve_notes(const uint64_t* pk_handles, int count, int input_form, int slot) {
  const char* const who = "capgpu_plonk_reserve_notes";
  if (bad_form(input_form)) return CAPGPU_ERR_INVALID_ARG;
  if (count < 0 || (count && !pk_handles)) return bad_args(who);
  CAP_CHECK_INIT();
  if (slot < -1 || slot >= (int)num_contexts()) {
    set_error("%s: bad argument (count >= 0, slot -1 .. %zu)", who, num_contexts() - 1);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (count == 0) return CAPGPU_OK;
  std::vector<std::shared_ptr<ProvingKey>> home;
  int rc = notes_keys(pk_handles, count, input_form, &home);
  if (rc) return rc;
  const np::Plan plan = notes_plan_of(home.data(), count, input_form);
  const bool vars = input_form == CAPGPU_INPUT_VARS;
  struct ScaleOne {  // exact sizes, as capgpu_plonk_reserve takes them
    double saved = scratch_growth_scale();
    ScaleOne() { scratch_growth_scale() = 1.0; }
    ~ScaleOne() { scratch_growth_scale() = saved; }
  } scale_one;
  for (int sl = slot < 0 ? 0 : slot, end = slot < 0 ? (int)num_contexts() : slot + 1; sl < end; sl++) {
    Context& c = *rt().ctxs[(size_t)sl];
    ScopedCtx sc(c);
    Entry lk(c);
    ProveNeeds nd;
    for (const np::Group& G : plan.groups) {
      const uint32_t cnt = (uint32_t)G.members.size();
      std::shared_ptr<ProvingKey> K0, K;
      size_t prefix = 0;
      for (uint32_t i : G.members) {
        if ((rc = part_key(pk_handles[i], &home[i], &K))) return rc;
        if (!K0) K0 = K;
        prefix = std::max(prefix, K->vk_bytes.size() + 32 * K->num_inputs);
      }
      const NttDomain* dn = nullptr;
      const Ntt3Domain* d3 = nullptr;
      if ((rc = get_domain(K0->log_n, &dn)) || (rc = quot_domains(K0->log_m, &d3, &dn))) return rc;
      for (int host = 0; host < 2; host++) {
        ProvePlan pl;
        if ((rc = make_plan(c, *K0, cnt, input_form, host != 0, prefix, true, &pl))) return rc;
        const ProveNeeds g = prove_needs(pl, *K0);
        nd.prove_ws = std::max(nd.prove_ws, g.prove_ws);
        nd.msm_ws = std::max(nd.msm_ws, g.msm_ws);
        nd.ntt_scratch = std::max(nd.ntt_scratch, g.ntt_scratch);
        nd.stage_a = std::max(nd.stage_a, g.stage_a);
        nd.stage_b = std::max(nd.stage_b, g.stage_b);
        nd.pinned = std::max(nd.pinned, g.pinned);
      }
      nd.stage_b = std::max(nd.stage_b, notes_stage_bytes(cnt, (size_t)G.n, (size_t)G.max_row, vars));
    }
    (void)h2d_stream();
    (void)side_stream(c);
    if ((rc = scratch_reserve(c.stage_b, nd.stage_b))) return rc;
    if ((rc = scratch_reserve(c.stage_a, nd.stage_a))) return rc;
    if ((rc = scratch_reserve(c.prove_ws, nd.prove_ws))) return rc;
    if ((rc = scratch_reserve(c.msm_ws, nd.msm_ws))) return rc;
    if ((rc = scratch_reserve(c.ntt_scratch, nd.ntt_scratch))) return rc;
    if ((rc = pinned_reserve(c, nd.pinned))) return rc;
    CAP_HIP(hipStreamSynchronize(c.stream));
    trace("reserve_notes", c.slot, count);
  }
  return CAPGPU_OK;
}

// gathered batches differ in size from one to the next: scratch that has to grow for one of `g` proofs grows to the next
// multiple of 32 proofs (64 at least) at once, while this object lives (see run_coalesced)
struct GatheredGrowth {
  double prev;
  explicit GatheredGrowth(size_t g) : prev(scratch_growth_scale()) {
    scratch_growth_scale() = (double)std::max<size_t>(64, (g + 31) / 32 * 32) / (double)g;
  }
  ~GatheredGrowth() { scratch_growth_scale() = prev; }
};

// one gathered batch: device staging of every request's wires, per-proof messages and keys.  Without the witness check
// the batch is proved in outcome mode (ProveRequest::outcomes): a request whose witness does not satisfy its circuit gets
// its own CAPGPU_ERR_PROOF with the message its lone call would set, the others get their proofs - nothing is proved twice.
// Runs on the calling thread's context (the leader took its lock).
static void run_coalesced(std::vector<ProveReq*>& reqs) {
  Context& c = ctx();
  Entry lk(c);
  auto fail_all = [&](int rc) {
    for (ProveReq* r : reqs) {
      if (r->rc != CAPGPU_OK) continue;
      r->rc = rc;
      r->err = capgpu_last_error();
    }
  };
  // one request on this context (the recursive lock is held)
  auto prove_one = [&](ProveReq* r) {
    std::shared_ptr<ProvingKey> K;
    int rc = lookup_key(r->pk, &K);
    const bool rv = r->form == CAPGPU_INPUT_VARS;
    if (rc == CAPGPU_OK && rv && key_lacks_table(*K)) rc = CAPGPU_ERR_INVALID_ARG;
    if (rc == CAPGPU_OK) {
      ProveCall one{&r->pk, true, 1, r->wires, r->pubs, r->num_inputs, r->msg, r->msg_len, nullptr, nullptr, r->blinders,
                    r->form, r->out};
      one.n = K->n;
      one.stride = rv ? K->num_vars : (size_t)NW * K->n;
      rc = host_part(one, 0, 1);
    }
    r->rc = rc;
    if (rc) r->err = capgpu_last_error();
  };
  std::vector<ProveReq*> good;
  std::vector<std::shared_ptr<ProvingKey>> hold;
  for (ProveReq* r : reqs) {
    std::shared_ptr<ProvingKey> K;
    int rc = lookup_key(r->pk, &K);
    if (rc == CAPGPU_OK && r->num_inputs != K->num_inputs) {
      set_error("capgpu_plonk_prove: %zu public inputs given, key expects %zu", r->num_inputs, K->num_inputs);
      rc = CAPGPU_ERR_INVALID_ARG;
    }
    if (rc == CAPGPU_OK && r->form == CAPGPU_INPUT_VARS && key_lacks_table(*K)) rc = CAPGPU_ERR_INVALID_ARG;
    if (rc != CAPGPU_OK) {
      r->rc = rc;
      r->err = capgpu_last_error();
      continue;
    }
    good.push_back(r);
    hold.push_back(K);
  }
  if (good.empty()) return;
  size_t g = good.size();
  const size_t n = hold[0]->n;
  size_t ni = 0;  // row length of the public inputs: the largest count among the batch's keys
  bool mixed = false;
  auto shape = [&] {
    ni = 0;
    mixed = false;
    for (size_t i = 0; i < g; i++) {
      ni = std::max(ni, hold[i]->num_inputs);
      mixed = mixed || hold[i].get() != hold[0].get();
    }
  };
  shape();
  bool recompute = false;
  for (size_t i = 0; i < g; i++) recompute = recompute || hold[i]->recompute;
  if (mixed && recompute) {  // the reference-schedule test mode keeps one key per batch: prove these one by one
    for (size_t i = 0; i < g; i++) prove_one(good[i]);
    coalescer().batches += g;
    coalescer().proofs += g;
    return;
  }
  // variable form: rows of the largest num_vars among the batch's keys, staged behind the columns they are gathered into
  const bool vars = good[0]->form == CAPGPU_INPUT_VARS;
  size_t vstride = 0;
  for (size_t i = 0; i < g && vars; i++) vstride = std::max(vstride, hold[i]->num_vars);
  const size_t per = vars ? sizeof(fe) * vstride : sizeof(fe) * NW * n;
  auto own_bytes = [&](size_t i) { return vars ? sizeof(fe) * hold[i]->num_vars : per; };  // what request i brings
  // gathered batches differ in size from one to the next: scratch that has to grow for one grows to the next multiple of
  // 32 proofs (64 at least) at once - a context otherwise re-allocates gigabytes (0.1 - 0.6 s each time) whenever a batch
  // is a few proofs larger than every batch it has seen (round 6: it cost the bench's coalesced leg a third)
  GatheredGrowth growth(g);
  int rc = scratch_reserve(c.stage_b, vars ? vars_stage_bytes(g, n, vstride, true) : per * g);
  if (rc) return fail_all(rc);
  char* const in_base = (char*)c.stage_b.p + (vars ? wires_stage_bytes(g, n) : 0);  // (g: the batch as it arrived)
  // capgpu_plonk_set_precheck: every witness of the gathered batch is checked where it will be proved from; a request
  // whose witness does not satisfy its circuit gets its own CAPGPU_ERR_PROOF and fault text, the others close ranks in
  // the input array and are proved as ONE batch - no request-by-request re-run, whoever shares the batch.
  // every request's witness into the batch's input array on the batch's stream: from the slot its caller staged it in
  // (StagePool; behind that copy), else from the caller's host buffer
  auto gather_all = [&]() -> hipError_t {
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < g && e == hipSuccess; i++) {
      char* dst = in_base + per * i;
      if (good[i]->d_wires) {
        e = hipStreamWaitEvent(c.stream, good[i]->staged, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(dst, good[i]->d_wires, own_bytes(i), hipMemcpyDeviceToDevice, c.stream);
      } else {
        e = hipMemcpyAsync(dst, good[i]->wires, own_bytes(i), hipMemcpyHostToDevice, c.stream);
        count_witness_h2d(own_bytes(i));
      }
    }
    return e;
  };
  bool prechecked = false;
  if (g_precheck.load(std::memory_order_relaxed) != 0) {
    hipError_t e = gather_all();
    if (e != hipSuccess) return fail_all(hip_fail(e, "gathering the witnesses"));
    std::vector<uint64_t> rows(4 * ni * g + 4, 0);
    std::vector<const ProvingKey*> ks(g);
    for (size_t i = 0; i < g; i++) {
      if (good[i]->num_inputs) memcpy(&rows[4 * ni * i], good[i]->pubs, 32 * good[i]->num_inputs);
      ks[i] = hold[i].get();
    }
    std::vector<capgpu_witness_fault> faults(g);
    if (vars)
      gather_vars(c.stream, *ks[0], mixed ? &ks : nullptr, 0, (uint32_t)g, VarsIn{(const fe*)in_base, vstride},
                  (fe*)c.stage_b.p);
    rc = check_resident(*ks[0], mixed ? &ks : nullptr, (uint32_t)g, (const fe*)c.stage_b.p, rows.data(), ni,
                        vars ? CAPGPU_INPUT_EVALS : good[0]->form, faults.data(), vars);
    if (rc) return fail_all(rc);
    size_t k = 0;
    for (size_t i = 0; i < g && e == hipSuccess; i++) {
      if (faults[i].kind) {
        (void)precheck_verdict(&faults[i], 1);
        good[i]->rc = CAPGPU_ERR_PROOF;
        good[i]->err = capgpu_last_error();
        continue;
      }
      if (k != i) {  // (row k < i has been read or dropped: the copies run in stream order)
        e = hipMemcpyAsync(in_base + per * k, in_base + per * i, per, hipMemcpyDeviceToDevice, c.stream);
        good[k] = good[i];
        hold[k] = hold[i];
      }
      k++;
    }
    good.resize(k);  // (the statistics count what is proved: the refused requests enter neither batches nor proofs)
    hold.resize(k);
    if (e != hipSuccess) return fail_all(hip_fail(e, "closing ranks in the gathered witnesses"));
    if (k == 0) return;
    g = k;
    shape();
    prechecked = true;
  }
  std::vector<uint64_t> pubs(4 * ni * g + 4, 0), blind(4 * 13 * g);
  std::vector<const uint8_t*> msgs(g);
  std::vector<size_t> lens(g);
  std::vector<capgpu_proof> out(g);
  std::vector<capgpu_prove_outcome> outs(prechecked ? 0 : g);  // (a checked batch has no bad witness left)
  std::vector<const ProvingKey*> keys(g);
  std::vector<const uint64_t*> rows(g);  // every caller's own buffer: copied inside round 1, chunk by chunk
  size_t staged = 0;
  for (size_t i = 0; i < g; i++) staged += good[i]->d_wires != nullptr;
  for (size_t i = 0; i < g; i++) {
    rows[i] = good[i]->wires;
    if (good[i]->num_inputs) memcpy(&pubs[4 * ni * i], good[i]->pubs, 32 * good[i]->num_inputs);
    memcpy(&blind[4 * 13 * i], good[i]->blinders, 32 * 13);
    msgs[i] = good[i]->msg;
    lens[i] = good[i]->msg_len;
    keys[i] = hold[i].get();
  }
  bool resident = prechecked;
  if (staged && !prechecked) {
    // the callers copied their witnesses when they arrived (StagePool): gather them into the batch's input array behind
    // their copies; a request that got no slot goes host -> device here, on the batch's stream
    trace("co_gather_staged", (int64_t)staged, (int64_t)g);
    const hipError_t e = gather_all();
    if (e != hipSuccess) return fail_all(hip_fail(e, "gathering the staged witnesses"));
    resident = true;
  }
  tl_prechecked = prechecked;
  const VarsIn vin{(const fe*)in_base, vstride};
  ProveRequest rq;
  rq.d_wires = (const fe*)c.stage_b.p;
  rq.pub_inputs = pubs.data();
  rq.num_inputs = ni;
  rq.blinders = blind.data();
  rq.proofs = out.data();
  rq.msgs = msgs.data();
  rq.msg_lens = lens.data();
  rq.keys = mixed ? &keys : nullptr;
  rq.h_wires = resident ? nullptr : rows.data();
  rq.form = good[0]->form;
  rq.vin = vars ? &vin : nullptr;
  rq.outcomes = prechecked ? nullptr : outs.data();
  rc = prove_batch(*keys[0], (uint32_t)g, rq);
  tl_prechecked = false;
  if (rc == CAPGPU_OK) rc = take_launch_error();
  if (rc == CAPGPU_OK) {
    for (size_t i = 0; i < g; i++) {
      if (prechecked || outs[i].status == CAPGPU_OK) {
        *good[i]->out = out[i];
        continue;
      }
      char text[320];  // what this request's own call would have set: proof 0, its flags
      oc::outcome_text(outs[i], text, sizeof text);
      good[i]->rc = outs[i].status;
      good[i]->err = text;
    }
  } else {
    for (ProveReq* r : good) {
      r->rc = rc;
      r->err = capgpu_last_error();
    }
  }
  coalescer().batches++;
  coalescer().proofs += g;
}

// ---- capgpu_plonk_prove_given_one / _io_one: single given-value calls, gathered ---------------------------------------------
static const char kProveGivenOne[] = "capgpu_plonk_prove_given_one";
// what the packing rule (given_gather.hpp) needs to know of one request: its key's home copy - no device is touched - and
// the two lengths on either side.  An unknown handle leaves home_key's code and message behind.
static int given_one_ask(uint64_t pk, size_t num_given, size_t num_inputs, std::shared_ptr<ProvingKey>* hold, gg::Ask* ask) {
  *ask = gg::Ask{};
  ask->num_given = num_given;
  ask->num_inputs = num_inputs;
  const int rc = home_key(pk, hold);
  if (rc) return rc;
  const ProvingKey& K = **hold;
  ask->key_found = true;
  ask->key_inputs = K.num_inputs;
  std::lock_guard<std::mutex> klk(K.chk_mu);
  ask->has_solver = K.solve && K.wire_vars;
  if (ask->has_solver) ask->key_given = K.solve->plan.num_given;
  return CAPGPU_OK;
}
// the code and message of a request that does not run
static int given_one_refusal(gg::Aside why, const gg::Ask& a, uint64_t pk) {
  switch (why) {
    case gg::kRuns:
      return CAPGPU_OK;
    case gg::kKeyGone: {
      std::shared_ptr<ProvingKey> none;
      const int rc = home_key(pk, &none);  // (its code and message; handles are never reused)
      return rc ? rc : CAPGPU_ERR_BAD_HANDLE;
    }
    case gg::kNoSolver:
      return no_solver(kProveGivenOne);
    default:
      set_error("%s: %zu given values and %zu public inputs passed, the key has %zu and %zu", kProveGivenOne, a.num_given,
                a.num_inputs, a.key_given, a.key_inputs);
      return CAPGPU_ERR_INVALID_ARG;
  }
}

// One gathered part of given-value requests (one kind: all plain or all _io) on the calling thread's context, whose lock the
// leader - or the helper thread of a cut batch - holds.  The requests that cannot run are set aside with their own code and
// message; the rows of the others are packed by given_gather.hpp's rule into ONE ProveCall with a key per proof, which
// given_part solves and proves: one staging copy, one solver launch per distinct key, the variable-form outcome call on
// library staging, witness check and compaction as that call applies them.  Then every caller gets what lies in its slot.
static void run_coalesced_given(std::vector<ProveReq*>& reqs) {
  Context& c = ctx();
  Entry lk(c);
  const bool io = reqs[0]->kind == ProveReq::kGivenIo;
  std::vector<gg::Ask> asks(reqs.size());
  std::vector<std::shared_ptr<ProvingKey>> homes_all(reqs.size());
  for (size_t i = 0; i < reqs.size(); i++)
    (void)given_one_ask(reqs[i]->pk, reqs[i]->num_given, reqs[i]->num_inputs, &homes_all[i], &asks[i]);
  const gg::Plan pl = gg::plan(asks.data(), asks.size());
  for (size_t i = 0; i < reqs.size(); i++)
    if (pl.why[i] != gg::kRuns) {
      reqs[i]->rc = given_one_refusal(pl.why[i], asks[i], reqs[i]->pk);
      reqs[i]->err = capgpu_last_error();
    }
  const size_t g = pl.slots();
  if (g == 0) return;
  // the slots [first, first + cnt) as one given-value call
  auto run = [&](size_t first, size_t cnt) {
    std::vector<uint64_t> handles(cnt);
    std::vector<std::shared_ptr<ProvingKey>> homes(cnt);
    std::vector<gg::Ask> part(cnt);
    for (size_t s = 0; s < cnt; s++) part[s] = asks[pl.req_of[first + s]];
    const gg::Plan pp = gg::plan(part.data(), cnt);  // (every one of them runs: the strides of THIS call)
    std::vector<uint64_t> given(pp.given_words(), 0), pubs(pp.pub_words(), 0), blind(pp.blind_words());
    std::vector<const uint8_t*> msgs(cnt);
    std::vector<size_t> lens(cnt);
    std::vector<capgpu_proof> out(cnt);
    std::vector<capgpu_prove_outcome> outs(cnt);
    std::vector<capgpu_solve_status> solved(cnt);
    size_t stride = 0, own = 0;
    for (size_t s = 0; s < cnt; s++) {
      const ProveReq& r = *reqs[pl.req_of[first + s]];
      handles[s] = r.pk;
      homes[s] = homes_all[pl.req_of[first + s]];
      stride = std::max(stride, homes[s]->num_vars);
      gg::pack_row(&given[pp.given_at(s)], pp.given_stride, r.given, r.num_given);
      if (!io) gg::pack_row(&pubs[pp.pub_at(s)], pp.pub_stride, r.pubs, r.num_inputs);
      memcpy(&blind[pp.blind_at(s)], r.blinders, sizeof(uint64_t) * gg::kWords * gg::kBlinders);
      msgs[s] = r.msg_len ? r.msg : nullptr;
      lens[s] = r.msg ? r.msg_len : 0;
      own += sizeof(fe) * r.num_given;
    }
    ProveCall b = each_call(handles.data(), (int)cnt, nullptr, pubs.data(), pp.pub_stride, msgs.data(), lens.data(),
                            blind.data(), CAPGPU_INPUT_VARS, out.data(), outs.data());
    b.one_key = each_one_key(b);
    b.homes = homes.data();
    b.n = homes[0]->n;
    b.stride = stride;
    b.given = given.data();
    b.given_stride = pp.given_stride;
    b.given_own_bytes = own;
    b.solved = solved.data();
    b.pub_out = io ? pubs.data() : nullptr;
    GatheredGrowth growth(cnt);
    trace("co_given_packed", (int64_t)cnt, (int64_t)own);
    int rc = given_part(b, 0, (int)cnt);
    if (rc == CAPGPU_OK) rc = take_launch_error();
    const std::string err = rc ? capgpu_last_error() : "";
    for (size_t s = 0; s < cnt; s++) {
      ProveReq& r = *reqs[pl.req_of[first + s]];
      r.rc = rc;
      if (rc) {  // a failure of the part is every caller's
        r.err = err;
        continue;
      }
      gg::normalise(&outs[s]);
      *r.out = out[s];
      *r.outcome = outs[s];
      if (r.solved) *r.solved = solved[s];
      if (io) gg::take_row(r.pub_out, &pubs[pp.pub_at(s)], r.num_inputs);
    }
  };
  bool mixed = false, recompute = false;
  for (size_t s = 0; s < g; s++) {
    const ProvingKey* K = homes_all[pl.req_of[s]].get();
    mixed = mixed || K != homes_all[pl.req_of[0]].get();
    recompute = recompute || K->recompute;
  }
  if (mixed && recompute) {  // the reference-schedule test mode keeps one key per batch: these go one by one
    for (size_t s = 0; s < g; s++) run(s, 1);
    coalescer().batches += g;
  } else {
    run(0, g);
    coalescer().batches++;
  }
  coalescer().proofs += g;
}

// what the gathering protocol (coalescer.hpp) needs from the runtime: free device contexts and the prover
struct CoalesceHooks {
  // a free device context: any of the process's (several batches are then in flight, one per context), or the one
  // this thread bound itself to; mode A of config 4: gathered batches go to the communicator's context, whole
  void* acquire() {
    const int ss = comm_shard_slot();
    const int bound = ss >= 0 && (size_t)ss < num_contexts() ? ss : thread_bound_slot();
    if (bound >= 0) {
      Context* b = rt().ctxs[(size_t)bound].get();
      return b->mu.try_lock() ? b : nullptr;
    }
    return try_acquire_context();
  }
  void* acquire_second() {
    if (thread_bound_slot() >= 0 || comm_shard_slot() >= 0 || num_contexts() <= 1) return nullptr;
    Context* c2 = try_acquire_context();
    if (c2) c2->mu.unlock();  // the helper thread locks it itself (the lock belongs to the thread that takes it)
    return c2;
  }
  // (the requests of one group are of one kind: wire-form, given-value, or given-value with computed public inputs)
  static void run_kind(std::vector<ProveReq*>& reqs) {
    if (reqs[0]->kind == ProveReq::kWires) run_coalesced(reqs);
    else run_coalesced_given(reqs);
  }
  void run(void* ctx, std::vector<ProveReq*>& reqs, bool on_helper) {
    Context& c = *static_cast<Context*>(ctx);
    ScopedCtx sc(c);
    if (on_helper) {
      Entry elk(c);
      run_kind(reqs);
    } else {
      run_kind(reqs);  // re-enters the (recursive) context lock this thread holds
    }
  }
  void release(void* ctx) { static_cast<Context*>(ctx)->mu.unlock(); }
  size_t deal_min() { return (size_t)::deal_min(); }
  size_t split_eighths() {  // CAPGPU_COALESCE_SPLIT = eighths of the first part
    static const size_t eighths = (size_t)env_int("CAPGPU_COALESCE_SPLIT", 3, 1, 4);
    return eighths;
  }
  // batch parts running at once before a leader keeps collecting instead of taking another free context:
  // CAPGPU_COALESCE_INFLIGHT (default 2) per bound DEVICE - two large batches fill a GPU, a third only fragments them
  size_t max_in_flight() {
    static const size_t per_device = (size_t)env_int("CAPGPU_COALESCE_INFLIGHT", 2, 1, 64);
    int devices = 1;
    (void)capgpu_physical_device_count(&devices);
    return per_device * (size_t)std::max(devices, 1);
  }
  bool early_release() {  // CAPGPU_COALESCE_EARLY=0: a cut batch's callers return when both parts are done, as before
    static const bool early = env_int("CAPGPU_COALESCE_EARLY", 1) != 0;
    return early;
  }
};

// The group of a key's requests: keys of one domain size under one SRS may share a device batch.  Bits 0-5 of the id are
// log2 of the domain size, bits 6-7 the form - the three input forms of the wire-form calls, and the value they leave free
// (3) for the given-value calls -, bit 63 tells the _io calls among those (a batch proves either against supplied or against
// computed public inputs), the SRS handle lies from bit 8 up.  *key_n: the key's domain size.  Called with `lk` (on co.mu)
// held; returns with it held, except with an error - an unknown handle -, which the caller returns at once.
static int coalesce_group(Coalescer& co, std::unique_lock<std::mutex>& lk, uint64_t pk_handle, unsigned form_bits, bool io,
                          uint64_t* group, size_t* key_n) {
  const uint64_t gkey = (pk_handle << 2) | (uint64_t)form_bits;
  auto it = co.group_of.find(gkey);
  if (it == co.group_of.end()) {
    // first call for this key: its domain size and SRS make the group
    lk.unlock();
    size_t kn = 0;
    uint64_t ksrs = 0;
    int rc = capgpu_plonk_key_info(pk_handle, &kn, nullptr, &ksrs);
    if (rc) return rc;
    lk.lock();
    it = co.group_of.emplace(gkey, std::make_pair((ksrs << 8) ^ (uint64_t)__builtin_ctzll(kn | (1ull << 63)) ^
                                                      ((uint64_t)form_bits << 6),
                                                  kn)).first;
  }
  *group = it->second.first ^ (io ? 1ull << 63 : 0);
  *key_n = it->second.second;
  return CAPGPU_OK;
}

int capgpu_plonk_prove_ex(uint64_t pk_handle, const uint64_t* wires, const uint64_t* pub_inputs, size_t num_inputs,
                          const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders, int input_form,
                          capgpu_proof* proof_out) {
  Coalescer& co = coalescer();
  const ProveCall a{&pk_handle, true, 1, wires, pub_inputs, num_inputs, ext_msg, ext_msg_len, nullptr, nullptr, blinders,
                    input_form, proof_out};
  if (co.window_us == 0) return prove_host(kProve, a);
  CAP_CHECK_INIT();
  if (bad_form(input_form)) return CAPGPU_ERR_INVALID_ARG;
  if (bad_front(a) || bad_rest(a)) return bad_args(kProve);
  size_t var_elems = 0;  // variable form: the values this call brings (and the refusal of a key without a table)
  if (input_form == CAPGPU_INPUT_VARS) {
    int rc = input_stride(&pk_handle, 1, input_form, 0, &var_elems);
    if (rc) return rc;
  }
  ProveReq req{pk_handle, wires, pub_inputs, num_inputs, ext_msg, ext_msg_len, blinders, proof_out, input_form};
  std::unique_lock<std::mutex> lk(co.mu);
  uint64_t group = 0;
  size_t key_n = 0;
  if (int rc = coalesce_group(co, lk, pk_handle, (unsigned)input_form, false, &group, &key_n)) return rc;
  // this caller's witness starts its way to the device now, on the staging pool's stream, while the batch it will be
  // part of is still being gathered (one bound device only: the slot must live where the batch runs)
  StageSlot slot;
  {
    int devices = 0;
    if (StagePool::enabled() && key_n && capgpu_physical_device_count(&devices) == CAPGPU_OK && devices == 1 &&
        comm_shard_slot() < 0) {
      co.arriving++;  // (a leader's window stays open for callers that are on their way)
      lk.unlock();
      const int dev = ctx().device;
      const size_t per = input_form == CAPGPU_INPUT_VARS ? sizeof(fe) * var_elems : sizeof(fe) * NW * key_n;
      slot = stage_pool().acquire(dev, per);
      if (slot.d) {
        hipError_t e = hipMemcpyAsync(slot.d, wires, per, hipMemcpyHostToDevice, slot.stream);
        if (e == hipSuccess) count_witness_h2d(per);
        if (e == hipSuccess) e = hipEventRecord(slot.ev, slot.stream);
        if (e != hipSuccess) {  // not fatal: the witness travels with the batch instead
          (void)hipGetLastError();
          (void)hipStreamSynchronize(slot.stream);
          stage_pool().release(slot);
          slot = StageSlot{};
        }
      }
      req.d_wires = slot.d;
      req.staged = slot.ev;
      trace("co_prestaged", slot.d != nullptr);
      lk.lock();
      co.arriving--;
    }
  }
  struct SlotReturn {  // (the batch that read the slot is done when submit returns; error paths included)
    StageSlot& s;
    ~SlotReturn() { stage_pool().release(s); }
  } slot_return{slot};
  CoalesceHooks hooks;
  co.submit(lk, req, group, hooks);
  if (req.rc != CAPGPU_OK) set_error("%s", req.err.c_str());
  return req.rc;
}

int capgpu_plonk_prove(uint64_t pk_handle, const uint64_t* wires, const uint64_t* pub_inputs, size_t num_inputs,
                       const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders, capgpu_proof* proof_out) {
  return capgpu_plonk_prove_ex(pk_handle, wires, pub_inputs, num_inputs, ext_msg, ext_msg_len, blinders,
                               CAPGPU_INPUT_EVALS, proof_out);
}

// capgpu_plonk_prove_given_one / _io_one: ONE proof from the values its circuit is given - what a rayon worker with one
// note's inputs calls.  Coalescing off: capgpu_plonk_prove_given[_io] with count = 1.  On: the request joins the group of its
// (domain size, SRS) and kind, and a leader proves the gathered part through run_coalesced_given.
static int given_one(ProveReq::Kind kind, uint64_t pk_handle, const uint64_t* given, size_t num_given,
                     const uint64_t* pub_inputs, uint64_t* pub_inputs_out, size_t num_inputs, const uint8_t* ext_msg,
                     size_t ext_msg_len, const uint64_t* blinders, capgpu_proof* proof_out,
                     capgpu_prove_outcome* outcome_out, capgpu_solve_status* solved_out) {
  const bool io = kind == ProveReq::kGivenIo;
  if (!given || !blinders || !proof_out || !outcome_out || (num_inputs && !(io ? (const void*)pub_inputs_out : pub_inputs)))
    return bad_args(kProveGivenOne);
  CAP_CHECK_INIT();
  if (comm_shard_slot() >= 0 || comm_shard_prover()) {
    set_error("%s: not available while capgpu_plonk_shard_msm is on (the ranks prove in lock step)", kProveGivenOne);
    return CAPGPU_ERR_INVALID_ARG;
  }
  Coalescer& co = coalescer();
  if (co.window_us == 0) {
    std::shared_ptr<ProvingKey> K;
    gg::Ask ask;
    (void)given_one_ask(pk_handle, num_given, num_inputs, &K, &ask);
    if (int rc = given_one_refusal(gg::set_aside(ask), ask, pk_handle)) return rc;
    const int rc = io ? capgpu_plonk_prove_given_io(&pk_handle, 1, given, num_inputs, &ext_msg, &ext_msg_len, blinders,
                                                    pub_inputs_out, proof_out, outcome_out, solved_out)
                      : capgpu_plonk_prove_given(&pk_handle, 1, given, pub_inputs, num_inputs, &ext_msg, &ext_msg_len,
                                                 blinders, proof_out, outcome_out, solved_out);
    if (rc == CAPGPU_OK) gg::normalise(outcome_out);
    return rc;
  }
  ProveReq req{pk_handle, nullptr, pub_inputs, num_inputs, ext_msg, ext_msg_len, blinders, proof_out, CAPGPU_INPUT_VARS};
  req.kind = kind;
  req.given = given;
  req.num_given = num_given;
  req.outcome = outcome_out;
  req.solved = solved_out;
  req.pub_out = pub_inputs_out;
  std::unique_lock<std::mutex> lk(co.mu);
  uint64_t group = 0;
  size_t key_n = 0;
  if (int rc = coalesce_group(co, lk, pk_handle, 3u, io, &group, &key_n)) return rc;
  // (no pre-staging: a row is a few KB and travels with the part's one copy)
  CoalesceHooks hooks;
  co.submit(lk, req, group, hooks);
  if (req.rc != CAPGPU_OK) set_error("%s", req.err.c_str());
  return req.rc;
}

int capgpu_plonk_prove_given_one(uint64_t pk_handle, const uint64_t* given, size_t num_given, const uint64_t* pub_inputs,
                                 size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders,
                                 capgpu_proof* proof_out, capgpu_prove_outcome* outcome_out,
                                 capgpu_solve_status* solved_out) {
  return given_one(ProveReq::kGiven, pk_handle, given, num_given, pub_inputs, nullptr, num_inputs, ext_msg, ext_msg_len,
                   blinders, proof_out, outcome_out, solved_out);
}
int capgpu_plonk_prove_given_io_one(uint64_t pk_handle, const uint64_t* given, size_t num_given, size_t num_inputs,
                                    const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders,
                                    uint64_t* pub_inputs_out, capgpu_proof* proof_out, capgpu_prove_outcome* outcome_out,
                                    capgpu_solve_status* solved_out) {
  return given_one(ProveReq::kGivenIo, pk_handle, given, num_given, nullptr, pub_inputs_out, num_inputs, ext_msg, ext_msg_len,
                   blinders, proof_out, outcome_out, solved_out);
}

// ---- witness check (see check_batch) -------------------------------------------------------------------------------
// One part of a check call on the calling thread's context: `cnt` witnesses from host memory (h_wires) or resident
// (d_wires), keys per proof (pk_handles) or one for all.
static int check_part(const uint64_t* pk_handles, uint64_t pk_handle, uint32_t cnt, const uint64_t* h_wires,
                      const void* d_wires, const uint64_t* pubs, size_t num_inputs, int form,
                      capgpu_witness_fault* faults, size_t stride) {
  Context& c = ctx();
  Entry lk(c);
  PartKeys held;
  KeySet ks;
  int rc = keys_in_rule(kCheckMulti, lookup_key, pk_handles ? pk_handles : &pk_handle, pk_handles ? cnt : 1, true, false,
                        &held, &ks);
  if (rc) return rc;
  const std::vector<const ProvingKey*>& keys = held.ptr;
  const size_t n = ks.n;
  if (form == CAPGPU_INPUT_VARS) {
    // rows of `stride` values per witness -> the five columns, in staging; then the gate pass alone: gathered columns
    // satisfy every copy constraint
    for (const ProvingKey* k : keys)
      if (key_lacks_table(*k)) return CAPGPU_ERR_INVALID_ARG;
    if ((rc = scratch_reserve(c.stage_b, vars_stage_bytes((size_t)cnt, n, stride, h_wires != nullptr)))) return rc;
    if (h_wires) {
      fe* d_vars = (fe*)c.stage_b.p + (size_t)cnt * NW * n;
      CAP_HIP(hipMemcpyAsync(d_vars, h_wires, sizeof(fe) * (size_t)cnt * stride, hipMemcpyHostToDevice, c.stream));
      count_witness_h2d(sizeof(fe) * (size_t)cnt * stride);
      d_wires = d_vars;
    }
    gather_vars(c.stream, *keys[0], pk_handles ? &keys : nullptr, 0, cnt, VarsIn{(const fe*)d_wires, stride},
                (fe*)c.stage_b.p);
    return check_resident(*keys[0], pk_handles ? &keys : nullptr, cnt, (const fe*)c.stage_b.p, pubs, num_inputs,
                          CAPGPU_INPUT_EVALS, faults, true);
  }
  if (h_wires) {
    if ((rc = scratch_reserve(c.stage_b, wires_stage_bytes((size_t)cnt, n)))) return rc;
    CAP_HIP(hipMemcpyAsync(c.stage_b.p, h_wires, sizeof(fe) * (size_t)cnt * NW * n, hipMemcpyHostToDevice, c.stream));
    count_witness_h2d(sizeof(fe) * (size_t)cnt * NW * n);
    d_wires = c.stage_b.p;
  }
  return check_resident(*keys[0], pk_handles ? &keys : nullptr, cnt, (const fe*)d_wires, pubs, num_inputs, form, faults);
}

// capgpu_plonk_check_witness_batch (h_wires: dealt over the contexts) and _batch_dev (d_wires: on the caller's context)
static int check_one_key(uint64_t pk_handle, int count, const uint64_t* h_wires, const void* d_wires,
                         const uint64_t* pub_inputs, size_t num_inputs, int input_form, capgpu_witness_fault* faults_out) {
  CAP_CHECK_INIT();
  if (bad_form(input_form)) return CAPGPU_ERR_INVALID_ARG;
  if (count < 0 || (count && ((!h_wires && !d_wires) || !faults_out || (num_inputs && !pub_inputs))))
    return bad_args("capgpu_plonk_check_witness");
  if (count == 0) return CAPGPU_OK;
  std::shared_ptr<ProvingKey> K0;
  int rc = home_key(pk_handle, &K0);
  if (rc) return rc;
  if (num_inputs != K0->num_inputs) {
    set_error("capgpu_plonk_check_witness: %zu public inputs given, key expects %zu", num_inputs, K0->num_inputs);
    return CAPGPU_ERR_INVALID_ARG;
  }
  size_t stride = 0;
  if ((rc = input_stride(&pk_handle, 1, input_form, K0->n, &stride))) return rc;
  if (d_wires)
    return check_part(nullptr, pk_handle, (uint32_t)count, nullptr, d_wires, pub_inputs, num_inputs, input_form, faults_out,
                      stride);
  return deal(count, [&](int first, int cnt) -> int {
    return check_part(nullptr, pk_handle, (uint32_t)cnt, h_wires + (size_t)4 * first * stride, nullptr,
                      pub_inputs ? pub_inputs + (size_t)4 * first * num_inputs : nullptr, num_inputs, input_form,
                      faults_out + first, stride);
  });
}
int capgpu_plonk_check_witness_batch_dev(uint64_t pk_handle, int count, const void* d_wires, const uint64_t* pub_inputs,
                                         size_t num_inputs, int input_form, capgpu_witness_fault* faults_out) {
  return check_one_key(pk_handle, count, nullptr, d_wires, pub_inputs, num_inputs, input_form, faults_out);
}
int capgpu_plonk_check_witness_batch(uint64_t pk_handle, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                                     size_t num_inputs, int input_form, capgpu_witness_fault* faults_out) {
  return check_one_key(pk_handle, count, wires, nullptr, pub_inputs, num_inputs, input_form, faults_out);
}

int capgpu_plonk_check_witness(uint64_t pk_handle, const uint64_t* wires, const uint64_t* pub_inputs, size_t num_inputs,
                               int input_form, capgpu_witness_fault* fault_out) {
  return capgpu_plonk_check_witness_batch(pk_handle, 1, wires, pub_inputs, num_inputs, input_form, fault_out);
}

int capgpu_plonk_check_witness_multi(const uint64_t* pk_handles, int count, const uint64_t* wires,
                                     const uint64_t* pub_inputs, size_t num_inputs, int input_form,
                                     capgpu_witness_fault* faults_out) {
  CAP_CHECK_INIT();
  if (bad_form(input_form)) return CAPGPU_ERR_INVALID_ARG;
  if (count < 0 || (count && (!pk_handles || !wires || !faults_out || (num_inputs && !pub_inputs))))
    return bad_args(kCheckMulti);
  if (count == 0) return CAPGPU_OK;
  // (the domain size alone: the parts compare the SRS where the keys are resident, check_part)
  PartKeys homes;
  KeySet ks;
  if (int rc = keys_in_rule(kCheckMulti, home_key, pk_handles, (size_t)count, false, false, &homes, &ks)) return rc;
  if (num_inputs != ks.max_inputs) {
    set_error("capgpu_plonk_check_witness_multi: rows of %zu public inputs given, the keys need %zu", num_inputs,
              ks.max_inputs);
    return CAPGPU_ERR_INVALID_ARG;
  }
  size_t stride = 0;
  if (int rc = input_stride(pk_handles, count, input_form, ks.n, &stride)) return rc;
  return deal(count, [&](int first, int cnt) -> int {
    return check_part(pk_handles + first, 0, (uint32_t)cnt, wires + (size_t)4 * first * stride, nullptr,
                      pub_inputs ? pub_inputs + (size_t)4 * first * num_inputs : nullptr, num_inputs, input_form,
                      faults_out + first, stride);
  });
}


int capgpu_plonk_set_precheck(int on) {
  g_precheck.store(on != 0);
  return CAPGPU_OK;
}

int capgpu_plonk_set_compaction(int on) {
  g_compact.store(on != 0);
  return CAPGPU_OK;
}

int capgpu_plonk_get_compaction(int* on_out) {
  if (!on_out) {
    set_error("capgpu_plonk_get_compaction: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  *on_out = compaction_on() ? 1 : 0;
  return CAPGPU_OK;
}

int capgpu_plonk_compaction_stats(uint64_t* calls_out, uint64_t* proofs_dropped_out, uint64_t* rows_moved_out) {
  if (calls_out) *calls_out = g_compact_calls.load();
  if (proofs_dropped_out) *proofs_dropped_out = g_compact_dropped.load();
  if (rows_moved_out) *rows_moved_out = g_compact_rows.load();
  return CAPGPU_OK;
}

int capgpu_plonk_set_coalescing(uint32_t window_us, uint32_t max_batch) {
  Coalescer& co = coalescer();
  std::lock_guard<std::mutex> lk(co.mu);
  co.window_us = window_us;
  co.max_batch = max_batch ? max_batch : 256;
  return CAPGPU_OK;
}

int capgpu_plonk_set_wire_commit(int mode) {
  if (mode < -1 || mode > 1) {
    set_error("capgpu_plonk_set_wire_commit: mode must be -1 (default), 0 (coefficients) or 1 (evaluations)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  g_wire_commit.store(mode);
  return CAPGPU_OK;
}

int capgpu_plonk_set_transcript(int mode) {
  if (mode != CAPGPU_TRANSCRIPT_HOST && mode != CAPGPU_TRANSCRIPT_DEVICE) {
    set_error("capgpu_plonk_set_transcript: mode must be CAPGPU_TRANSCRIPT_HOST (0) or CAPGPU_TRANSCRIPT_DEVICE (1)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  g_transcript.store(mode);
  return CAPGPU_OK;
}

int capgpu_plonk_get_transcript(int* mode_out) {
  if (!mode_out) {
    set_error("capgpu_plonk_get_transcript: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  *mode_out = transcript_mode();
  return CAPGPU_OK;
}

int capgpu_plonk_sync_stats(uint64_t* prove_calls_out, uint64_t* stream_waits_out) {
  if (prove_calls_out) *prove_calls_out = g_prove_calls.load();
  if (stream_waits_out) *stream_waits_out = g_stream_waits.load();
  return CAPGPU_OK;
}

int capgpu_keccak256_batch_dev(const uint8_t* data, const uint64_t* offsets, int count, uint8_t* digests_out) {
  CAP_CHECK_INIT();
  Context& c = ctx();
  Entry lk(c);
  if (count < 0 || (count && (!offsets || !digests_out))) {
    set_error("capgpu_keccak256_batch_dev: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (count == 0) return CAPGPU_OK;
  for (int i = 0; i < count; i++)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] >= (1ull << 31)) {
      set_error("capgpu_keccak256_batch_dev: offsets must not decrease, and a message must be shorter than 2^31 bytes");
      return CAPGPU_ERR_INVALID_ARG;
    }
  const uint64_t lo = offsets[0], total = offsets[count] - lo;
  if (total && !data) {
    set_error("capgpu_keccak256_batch_dev: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  hipStream_t s = c.stream;
  DevTmp<uint8_t> d_data, d_out;
  DevTmp<uint64_t> d_off;
  CAP_HIP(d_data.alloc(total));
  CAP_HIP(d_out.alloc((size_t)count * 32));
  CAP_HIP(d_off.alloc((size_t)count + 1));
  std::vector<uint64_t> rel(offsets, offsets + count + 1);
  for (auto& o : rel) o -= lo;
  if (total) CAP_HIP(hipMemcpyAsync(d_data, data + lo, total, hipMemcpyHostToDevice, s));
  CAP_HIP(hipMemcpyAsync(d_off, rel.data(), sizeof(uint64_t) * rel.size(), hipMemcpyHostToDevice, s));
  launch("k_keccak_batch", td::k_keccak_batch, dim3((uint32_t)count), dim3(64), 0, s, (const uint8_t*)d_data.p,
         (const uint64_t*)d_off.p, (uint32_t)count, d_out.p);
  CAP_HIP(hipMemcpyAsync(digests_out, d_out, (size_t)count * 32, hipMemcpyDeviceToHost, s));
  CAP_HIP(hipStreamSynchronize(s));
  return take_launch_error();
}

int capgpu_plonk_graph_stats(uint64_t* segments_captured_out, uint64_t* segments_replayed_out) {
  if (segments_captured_out) *segments_captured_out = g_graph_captured.load();
  if (segments_replayed_out) *segments_replayed_out = g_graph_replayed.load();
  return CAPGPU_OK;
}

int capgpu_plonk_coalescing_stats(uint64_t* batches_out, uint64_t* proofs_out) {
  Coalescer& co = coalescer();
  if (batches_out) *batches_out = co.batches.load();
  if (proofs_out) *proofs_out = co.proofs.load();
  return CAPGPU_OK;
}

}  // extern "C"
