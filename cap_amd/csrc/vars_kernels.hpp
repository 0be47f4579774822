// Kernels of the variable-form input (CAPGPU_INPUT_VARS): a circuit's wire -> variable table (jf-relation's
// `wire_variables`, 5 columns of n ids) is all a key needs to know its copy constraints, and a witness is one value per
// variable (`witness: Vec<F>`) - the five wire columns are that vector gathered through the table.
//   k_vars_keys        one lane per cell: the sort key (variable << 32) | cell; the tail of the power-of-two array is ~0
//   k_vars_sort_tile   bitonic stages whose partners lie inside one tile of 2048 keys, in LDS
//   k_vars_sort_step   one bitonic stage whose partners lie in different tiles
//   k_vars_link        sorted keys -> index form of the extended permutation: every cell points to the next cell of its
//                      variable in ascending cell order, the last one to the first (bench_utils._permutation,
//                      jf-relation's compute_wire_permutation)
//   k_vars_sigma       index form -> field form, sigma(cell) = k_wire' omega^row' (what ProvingKey::sig_eval holds)
//   k_vars_differ      first cell at which two index tables differ (capgpu_plonk_key_set_vars)
//   k_gather_vars      w[p][i][j] = vars[p][table[i][j]] for a chunk of proofs: two lanes per cell, 16 bytes each
// The keys are unique, so the sorted order - and with it the permutation - is a function of the table alone: nothing here
// is ordered by an atomic.  A variable's cells are one run of the sorted array however many they are (the padding
// variable of a CAP circuit holds more than half of all cells) and a run may span any number of tiles: k_vars_link looks
// one key ahead for the next cell and, at the end of a run, finds the run's head by a binary search for (variable << 32).
#pragma once
#include <hip/hip_runtime.h>

#include "plonk_kernels.hpp"

namespace cap {
namespace pk {

constexpr uint32_t kSortTile = 2048;  // keys per workgroup in k_vars_sort_tile: 8 per lane, 16 KB of LDS
constexpr unsigned long long kVarsPad = ~0ull;

// constants of k_vars_sigma for one domain, arkworks form: the coset representatives and omega^(2^b), b < log_n
struct SigmaConsts {
  fe k[NW];
  fe wpow[28];
  uint32_t log_n;
};

__global__ __launch_bounds__(kThreads) void k_vars_keys(const uint32_t* __restrict__ table /*[5 n]*/, size_t cells,
                                                        size_t padded, unsigned long long* __restrict__ keys) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= padded) return;
  keys[c] = c < cells ? ((unsigned long long)table[c] << 32) | (unsigned long long)c : kVarsPad;
}

// element i of the pair lane t handles in a stage of distance j (a power of two): the t-th index with bit j clear
__device__ __forceinline__ size_t bitonic_low(size_t t, size_t j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// Stages (k, j) of the bitonic network for k = k_lo, 2 k_lo, .. k_hi and j = min(k / 2, kSortTile / 2) .. 1 on the tile of
// kSortTile keys this workgroup owns.  (k_lo = 2, k_hi = kSortTile sorts every tile; k_lo = k_hi = k > kSortTile finishes
// merge step k after its cross-tile stages.)  `padded` is a multiple of kSortTile.
__global__ __launch_bounds__(kThreads) void k_vars_sort_tile(unsigned long long* __restrict__ keys, size_t k_lo,
                                                             size_t k_hi) {
  __shared__ unsigned long long sh[kSortTile];
  const size_t base = (size_t)blockIdx.x * kSortTile;
  for (uint32_t i = threadIdx.x; i < kSortTile; i += kThreads) sh[i] = keys[base + i];
  __syncthreads();
  for (size_t k = k_lo; k <= k_hi; k <<= 1) {
    for (uint32_t j = (uint32_t)(k / 2 < kSortTile / 2 ? k / 2 : kSortTile / 2); j >= 1; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < kSortTile / 2; t += kThreads) {
        const uint32_t i = (uint32_t)bitonic_low(t, j), q = i + j;
        const bool up = ((base + i) & k) == 0;
        const unsigned long long a = sh[i], b = sh[q];
        if ((a > b) == up) {
          sh[i] = b;
          sh[q] = a;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = threadIdx.x; i < kSortTile; i += kThreads) keys[base + i] = sh[i];
}

// stage (k, j), j >= kSortTile: one lane per pair, padded / 2 lanes
__global__ __launch_bounds__(kThreads) void k_vars_sort_step(unsigned long long* __restrict__ keys, size_t pairs, size_t k,
                                                             size_t j) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= pairs) return;
  const size_t i = bitonic_low(t, j), q = i + j;
  const bool up = (i & k) == 0;
  const unsigned long long a = keys[i], b = keys[q];
  if ((a > b) == up) {
    keys[i] = b;
    keys[q] = a;
  }
}

__global__ __launch_bounds__(kThreads) void k_vars_link(const unsigned long long* __restrict__ keys /*sorted*/,
                                                        size_t cells, uint32_t* __restrict__ perm /*[5 n]*/) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cells) return;
  const unsigned long long key = keys[t];
  const unsigned long long run = key >> 32 << 32;
  uint32_t next;
  if (t + 1 < cells && (keys[t + 1] >> 32 << 32) == run) {
    next = (uint32_t)keys[t + 1];
  } else {  // the last cell of its variable points to the first: the smallest key that is not below (variable << 32)
    size_t lo = 0, hi = t;
    while (lo < hi) {
      const size_t mid = lo + (hi - lo) / 2;
      if (keys[mid] < run) lo = mid + 1;
      else hi = mid;
    }
    next = (uint32_t)keys[lo];
  }
  perm[(uint32_t)key] = next;
}

__global__ __launch_bounds__(kThreads) void k_vars_sigma(const uint32_t* __restrict__ perm /*[5 n]*/, SigmaConsts sc,
                                                         size_t cells, fe* __restrict__ sig_eval /*[5 n], arkworks form*/) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cells) return;
  const uint32_t to = perm[c];
  const uint32_t wire = to >> sc.log_n, row = to & ((1u << sc.log_n) - 1);
  fe v = sc.k[wire < NW ? wire : 0];
#pragma unroll 1
  for (uint32_t b = 0; b < sc.log_n; b++)
    if ((row >> b) & 1) v = Fr::mul(v, sc.wpow[b]);
  sig_eval[c] = v;
}

// *first = the smallest c with a[c] != b[c] (stays ~0 when there is none); a minimum: the same on every run
__global__ __launch_bounds__(kThreads) void k_vars_differ(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                          size_t cells, unsigned long long* __restrict__ first) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cells) return;
  if (a[c] != b[c]) atomicMin(first, (unsigned long long)c);
}

// Proofs blockIdx.y, blockIdx.y + gridDim.y, .. < cnt of a chunk.  Lane t moves half (t & 1) of cell t >> 1: the table is
// read once per cell and kept in a register over the lane's proofs, a wavefront's stores are 1 KB without a gap, and each
// 32-byte value arrives as the two 16-byte loads of a lane pair.  Every table entry is below `stride` (checked when the
// key took the table), so no load leaves a proof's row.
__global__ __launch_bounds__(kThreads) void k_gather_vars(const uint4* __restrict__ vars /*[cnt][stride] x 2*/, size_t stride,
                                                          const uint32_t* __restrict__ table /*[5 n]*/, size_t cells,
                                                          uint32_t cnt, uint4* __restrict__ out /*[cnt][5 n] x 2*/) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * cells) return;
  const size_t src = (size_t)table[t >> 1] * 2 + (t & 1);
#pragma unroll 4
  for (uint32_t p = blockIdx.y; p < cnt; p += gridDim.y) out[(size_t)p * cells * 2 + t] = vars[(size_t)p * stride * 2 + src];
}

}  // namespace pk
}  // namespace cap
