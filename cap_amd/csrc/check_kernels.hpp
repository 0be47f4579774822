// Kernels of the witness check (capgpu_plonk_check_witness*): gates and copy constraints of P witnesses against their
// circuits, the counterpart of the `check_circuit_satisfiability` the reference runs before it proves
// (src/proof/transfer.rs:167-177).  The arithmetic is gatecheck29.hpp (host + device).
//   k_check_gates     one lane per (proof, row): the gate constraint with the key's selector VALUES on the domain
//   k_check_copies    one lane per (proof, wire, row): w[i][j] == w[i'][j'] through the key's index table
//   k_check_targets   one lane per proof: the cell its first violated copy constraint points to (for the message)
//   k_perm_index      once per key: sigma_i(omega^j) = k_i' omega^j'  ->  i' n + j'  (a discrete logarithm per lane)
// A proof's verdict is (first failing key, number of failing gates, number of failing copies): the key is the row for a
// gate and 2^40 + i n + j for a copy constraint, so ONE unsigned minimum gives the first failing gate in row order or,
// when every gate holds, the first violated copy constraint in (wire, row) order.  Minimum and integer sums do not depend
// on the order the blocks arrive in: the verdict is the same on every run.
// Measured (profiles/check_witness_r08.json; 256 transfer witnesses, n = 2^15, one MI355X): k_check_gates 1.79 ms, 162
// VGPRs, no scratch, 3 waves per SIMD; k_check_copies 0.42 ms, 40 VGPRs, 8 waves; the whole check 2.3 ms = 1.2 % of the
// batch's prove step (the 1.34 GB of wires at 6.3 TB/s would be 0.21 ms: the gate kernel is bound by its 23 products per
// row, not by memory); k_perm_index 60 VGPRs, no scratch, 8 waves.
#pragma once
#include <hip/hip_runtime.h>

#include "gatecheck29.hpp"
#include "plonk_kernels.hpp"

namespace cap {
namespace pk {

constexpr unsigned long long kCopyKeyBase = 1ull << 40;
constexpr unsigned long long kNoFault = ~0ull;

// what proof p is checked against (a batch may mix keys of one domain)
struct CheckKey {
  const fe* sel;         // [13][n] selector values, internal form, canonical
  const uint32_t* perm;  // [5 n] index form of the extended permutation
  uint32_t num_inputs;
  uint32_t pad;
};
struct CheckOut {
  unsigned long long first;  // smallest failing key, kNoFault when the witness satisfies the circuit
  unsigned long long gates, copies;
};

// wave -> block -> one pair of atomics per block that saw a failure (most blocks see none)
__device__ __forceinline__ void check_report(unsigned long long key, unsigned long long* first,
                                             unsigned long long* count) {
  __shared__ unsigned long long s_min[kThreads / 64];
  __shared__ uint32_t s_cnt[kThreads / 64];
  const uint32_t cnt = (uint32_t)__popcll(__ballot(key != kNoFault));
  uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t olo = __shfl_xor(lo, d), ohi = __shfl_xor(hi, d);
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo, m = ((unsigned long long)hi << 32) | lo;
    if (o < m) {
      lo = olo;
      hi = ohi;
    }
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_min[wave] = ((unsigned long long)hi << 32) | lo;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = s_min[0];
    uint32_t c = s_cnt[0];
#pragma unroll
    for (int k = 1; k < kThreads / 64; k++) {
      m = s_min[k] < m ? s_min[k] : m;
      c += s_cnt[k];
    }
    if (c) {
      atomicMin(first, m);
      atomicAdd(count, (unsigned long long)c);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_check_gates(const fe* __restrict__ wires /*[P][5][n]*/,
                                                          const fe* __restrict__ pub /*[P][pub_stride]*/,
                                                          size_t pub_stride, const CheckKey* __restrict__ keys, size_t n,
                                                          CheckOut* __restrict__ out) {
  using C = wc29::Check<>;
  using F = C::F;
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t p = blockIdx.y;
  unsigned long long key = kNoFault;
  if (j < n) {
    const CheckKey k = keys[p];
    fl w[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) w[i] = F::from_ext(wires[((size_t)p * NW + i) * n + j]);
    const fl pi = j < k.num_inputs ? F::from_ext(pub[(size_t)p * pub_stride + j]) : F::zero();
    const fe* sel = k.sel + j;
    if (!C::gate_holds([&](int s) { return F::load(sel[(size_t)s * n]); }, w, pi)) key = j;
  }
  check_report(key, &out[p].first, &out[p].gates);
}

__global__ __launch_bounds__(kThreads) void k_check_copies(const fe* __restrict__ wires /*[P][5 n]*/,
                                                           const CheckKey* __restrict__ keys, size_t n,
                                                           CheckOut* __restrict__ out) {
  using C = wc29::Check<>;
  const size_t cells = (size_t)NW * n;
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t p = blockIdx.y;
  unsigned long long key = kNoFault;
  if (c < cells) {
    const uint32_t to = keys[p].perm[c];
    // A cell that maps to itself needs no gather.  (`to < cells` guards the load only: key_check_tables refuses a key whose
    // sigma holds a value outside the five cosets for good, so a table with an unindexed cell never reaches this kernel -
    // a bad sigma is CAPGPU_ERR_INVALID_ARG, never "satisfied".)
    if (to != c && to < cells) {
      const fe* w = wires + (size_t)p * cells;
      if (!C::same_value(w[c], w[to])) key = kCopyKeyBase + c;
    }
  }
  check_report(key, &out[p].first, &out[p].copies);
}

// The prover's own test on the rows, where the quotient is interpolated from five n-cosets and carries no redundancy: a
// numerator that is not divisible by Z_H no longer shows as coefficients above degree 5n + 7 (k_check_degree's bit 1).
// Divisible means: zero on every row of the domain, where the blinders vanish - the gate constraint holds on every row
// (k_check_gates: out[p].first), z(omega x) den = z(x) num holds on every row by the way z is made, and z closes:
// prod num == prod den, from the scans' ends.  flags[p] |= 1 otherwise: the same bit for the same witnesses.
__global__ void k_rows_verdict(const CheckOut* __restrict__ out, const fe* __restrict__ pre, const fe* __restrict__ num,
                               const fe* __restrict__ sfx, const fe* __restrict__ den, size_t n,
                               uint32_t* __restrict__ flags, uint32_t count) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  const size_t o = (size_t)p * n;
  const fe total_num = Fr::mul(pre[o + n - 1], num[o + n - 1]), total_den = Fr::mul(sfx[o], den[o]);
  if (out[p].first != kNoFault || !Fr::eq(total_num, total_den)) atomicOr(&flags[p], 1u);
}

// After both checks: the cell a proof's first violated copy constraint points to (what the message names), one lane per
// proof - so that the host fetches P words in one copy instead of one word per faulty witness.
__global__ void k_check_targets(const CheckKey* __restrict__ keys, const CheckOut* __restrict__ out, uint32_t P,
                                size_t cells, uint32_t* __restrict__ to) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const unsigned long long first = out[p].first;
  uint32_t t = 0;
  if (first != kNoFault && first >= kCopyKeyBase && first - kCopyKeyBase < cells) t = keys[p].perm[first - kCopyKeyBase];
  to[p] = t;
}

// perm[i n + j] = index of sigma_i(omega^j); *bad != 0 afterwards: a value outside the five cosets
__global__ __launch_bounds__(kThreads) void k_perm_index(const fe* __restrict__ sig_eval /*[5 n], arkworks form*/,
                                                         wc29::PermConsts pc, size_t cells, uint32_t* __restrict__ perm,
                                                         uint32_t* __restrict__ bad) {
  using C = wc29::Check<>;
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cells) return;
  const uint32_t idx = C::perm_index(C::F::from_ext(sig_eval[c]), pc);
  perm[c] = idx;
  if (idx == wc29::kNoIndex) atomicOr(bad, 1u);
}

}  // namespace pk
}  // namespace cap
