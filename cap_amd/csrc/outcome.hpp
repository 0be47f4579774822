// Per-proof outcomes of capgpu_plonk_prove_each* - the ONE rule, host+device like proof_codec.hpp and verify_front.hpp:
//   * a proof failed exactly when k_check_degree left a non-zero flags word for it or the witness check (capgpu_plonk_
//     set_precheck) found a fault: prove_status;
//   * the record of a failed proof is all-ones words - the convention k_proof_decode_finish uses for a refused record,
//     which k_verify_front rejects by its range checks: blank_record, lane by lane (the host is lane 0 of 1);
//   * the message of a failed proof is the one capgpu_plonk_prove_ex of that witness ALONE sets (`proof 0`, `1 of 1`):
//     outcome_text, host only.  degree_text / fault_text are also what the all-or-nothing entry points say.
// k_prove_outcomes (prove_run.hpp) runs the first two on the device, behind k_tr_open; the host transcript and
// capgpu_prove_outcome_text run all three on the host.  tests/cpp/prove_outcome_check.cpp runs everything here on the
// host, under the sanitizers too.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/capgpu.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CAP_OC_HD __host__ __device__ __forceinline__
#else
#define CAP_OC_HD inline
#endif

namespace cap {
namespace oc {

constexpr uint32_t kRecordWords = (uint32_t)(sizeof(capgpu_proof) / sizeof(uint64_t));
static_assert(sizeof(capgpu_proof) % sizeof(uint64_t) == 0, "a record is blanked in 64-bit words");
static_assert(sizeof(capgpu_prove_outcome) == 56, "capgpu_prove_outcome is part of the ABI");

CAP_OC_HD int32_t prove_status(uint32_t degree_flags, uint32_t fault_kind) {
  return (degree_flags != 0 || fault_kind != 0) ? CAPGPU_ERR_PROOF : CAPGPU_OK;
}
// words lane, lane + lanes, ... of the record at `rec` (8-byte aligned, as a capgpu_proof is) to all ones
CAP_OC_HD void blank_record(void* rec, uint32_t lane, uint32_t lanes) {
  uint64_t* w = (uint64_t*)rec;
  for (uint32_t k = lane; k < kRecordWords; k += lanes) w[k] = ~0ull;
}

// the witness check's device-side verdict of a satisfied witness (check_kernels.hpp: CheckOut::first == kNoFault)
constexpr unsigned long long kCheckNoFault = ~0ull;

#if defined(__HIPCC__)
// One wavefront per proof, as k_proof_decode_finish: reads the proof's degree flags and - when the witness check ran
// (chk_first != nullptr) - the check's verdict, writes the status word, and overwrites the record of a failed proof
// with all-ones words before the call's one device-to-host copy takes it.  Every branch is on values the whole
// wavefront shares (blockIdx.x, two words loaded by all lanes from one address): no divergence, no field arithmetic.
__global__ __launch_bounds__(64) void k_prove_outcomes(uint32_t count, const uint32_t* __restrict__ flags,
                                                       const unsigned long long* __restrict__ chk_first,
                                                       int32_t* __restrict__ status, uint8_t* __restrict__ proofs) {
  const uint32_t p = blockIdx.x, t = threadIdx.x;
  if (p >= count) return;
  const uint32_t kind = (chk_first && chk_first[p] != kCheckNoFault) ? 1u : 0u;
  const int32_t st = prove_status(flags[p], kind);
  if (t == 0) status[p] = st;
  if (st != CAPGPU_OK) blank_record(proofs + (size_t)p * sizeof(capgpu_proof), t, 64);
}
#endif

// ---- host only ----
// "proof 3: gate 1234 not satisfied" / "proof 3: copy constraint (2,40) -> (0,7) violated"; returns snprintf's count
inline int fault_text(uint32_t p, const capgpu_witness_fault& f, char* buf, size_t cap) {
  if (f.kind == 1) return snprintf(buf, cap, "proof %u: gate %llu not satisfied", p, (unsigned long long)f.row);
  return snprintf(buf, cap, "proof %u: copy constraint (%u,%llu) -> (%u,%llu) violated", p, f.wire,
                  (unsigned long long)f.row, f.wire2, (unsigned long long)f.row2);
}
// the witness check's refusal of a batch of `total` with `bad` faults, the first of them proof `first`
inline int precheck_text(uint32_t bad, uint32_t total, uint32_t first, const capgpu_witness_fault& f, char* buf, size_t cap) {
  char ft[160];
  fault_text(first, f, ft, sizeof ft);
  return snprintf(buf, cap, "capgpu_plonk_prove: %u of %u witnesses do not satisfy their circuit; first: %s", bad, total, ft);
}
// the degree check's refusal of proof p
inline int degree_text(uint32_t p, uint32_t flags, char* buf, size_t cap) {
  return snprintf(buf, cap,
                  "capgpu_plonk_prove: proof %u: quotient polynomial has the wrong degree (flags %u): "
                  "the circuit is not satisfied by this witness",
                  p, flags);
}
// The message capgpu_plonk_prove_ex of this witness alone sets: the check's wording when the check found a fault, else
// the degree wording, else nothing.  At most cap - 1 characters and a NUL (cap 0: nothing is written); returns the length
// of the whole message.
inline int outcome_text(const capgpu_prove_outcome& o, char* buf, size_t cap) {
  char none[1];
  if (cap == 0) buf = none;  // (snprintf with a size of 0 writes nothing)
  if (o.fault.kind) return precheck_text(1, 1, 0, o.fault, buf, cap);
  if (o.degree_flags) return degree_text(0, o.degree_flags, buf, cap);
  if (cap) buf[0] = 0;
  return 0;
}
// the whole outcome of one proof on the host: status from (flags, fault), the record blanked when it failed
inline void finish_outcome(uint32_t degree_flags, const capgpu_witness_fault* fault, capgpu_prove_outcome* o, capgpu_proof* rec) {
  memset(o, 0, sizeof *o);
  o->degree_flags = degree_flags;
  if (fault) o->fault = *fault;
  o->status = prove_status(degree_flags, o->fault.kind);
  if (o->status != CAPGPU_OK && rec) blank_record(rec, 0, 1);
}

}  // namespace oc
}  // namespace cap
