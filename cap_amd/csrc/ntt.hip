// K2: multi-pass NTT over BN254 Fr with LDS-staged sub-transforms (see ntt.hpp).
//
// Decomposition (decimation in frequency, mixed radix 2^a x 2^b [x 2^c]):
//   n = N1*N2*N3, input index i = (i1*N2 + i2)*N3 + i3, output index k = k1 + N1*k2 + N1*N2*k3.
//   "column" passes transform one digit at a stride, multiply by the inter-pass
//   twiddle omega_M^(col*k) and store in place (to scratch); the final "row"
//   pass transforms contiguous rows and stores digit-reversed, C adjacent k1 per
//   workgroup so the scattered stores are C*32 B contiguous.
// Each workgroup stages a tile of len x C elements in LDS (<= 64 KiB) and runs
// log2(len) radix-2 stages there; HBM sees one read + one write of the array per
// pass.  All arithmetic is 254-bit modular integer work (no MFMA).
// (The column-wise multiplication schedule was measured here too: column pass 19.6 -> 19.4 ms, row pass 18.1 -> 19.0 ms
// per step.  The butterflies keep several independent multiplications in flight; the row-wise schedule stays.)
#include "ntt.hpp"
#include "field29.hpp"
#include "ntt_elem29.hpp"
#include "launch.hpp"

#include <stdlib.h>

#include <vector>

namespace cap {

namespace {

constexpr int kThreads = 256;
// Elements per thread whose global loads are issued together.  Measured in round 4 (round-4 same-box A/B `ntt_io`, profiles/LOG.md, same box,
// col + row pass per step): 1 (the old element-by-element loop) 37.2-37.6 ms, 2: 36.7 ms, 4: 38.1-38.4 ms (135 VGPRs: three
// waves per SIMD instead of four; held to 128 VGPRs with 52 B of scratch: 37.9 ms).  The passes are not waiting for
// memory - they are issue-bound butterflies with a barrier per radix-4 round - so 2 stays, for what it is worth.
#ifndef CAP_NTT_IO_BATCH
#define CAP_NTT_IO_BATCH 2
#endif
constexpr int kIoBatch = CAP_NTT_IO_BATCH;
#ifdef CAP_NTT_WAVES4  // experiment: hold the passes to the 128 VGPRs of four waves per SIMD (the LDS tile allows no more)
#define CAP_NTT_ATTR __attribute__((amdgpu_waves_per_eu(4, 4)))
#else
#define CAP_NTT_ATTR
#endif  // elements per thread whose global loads are issued together (a 1024-element tile: all 4)
constexpr uint32_t kMaxTileLogDefault = 10;  // 1024 elements * 36 B = 36 KiB of LDS (4 workgroups per CU)
uint32_t max_tile_log() {
  static uint32_t v = [] {
    const char* e = getenv("CAPGPU_NTT_TILE_LOG");
    int x = e ? atoi(e) : (int)kMaxTileLogDefault;
    return (uint32_t)(x >= 8 && x <= 11 ? x : (int)kMaxTileLogDefault);
  }();
  return v;
}

// A launch of a few transforms (a single proof's: 1 .. 15 arrays of 2^15 .. 2^16 elements) makes fewer 1024-element tiles
// than the chip has CUs, and a pass then lasts as long as ONE workgroup takes for its tile: such launches get tiles of 512
// or 256 elements - twice / four times the workgroups, each half / a quarter as long.  (For launches that fill the chip the
// smaller tiles are slower - narrower column tiles, more twiddle traffic: round-4 log - and are never chosen.)
uint32_t tile_log_for(uint32_t log_n, uint32_t count) {
  static const bool adapt = [] {
    const char* e = getenv("CAPGPU_NTT_TILE_ADAPT");
    return !e || atoi(e) != 0;
  }();
  uint32_t tl = max_tile_log();
  if (!adapt) return tl;
  while (tl > 8 && (((uint64_t)count << log_n) >> tl) < 256) tl--;
  return tl;
}

struct PassParams {
  const fe* in;
  fe* out;
  // array q of the batch starts at (q / group) * outer + (q % group) * inner elements; input elements at or beyond
  // in_len read as zero (a polynomial shorter than the transform: no padded copy has to exist in memory)
  size_t in_outer, in_inner, in_len;
  uint32_t in_group;
  uint32_t in_es;            // element stride of the first-pass input (decimated transforms); 1 = contiguous
  size_t in_fold;            // folded first-pass input (NttIo::src_fold; contiguous input with a pre-scale table); 0 = none
  // second grouping level of the input (decimated transforms of grouped polynomials): array q = (q2, a) with
  // a = q % in_group the decimation phase and q2 = q / in_group placed at (q2 / in_group2) * in_outer + (q2 % in_group2) * in_inner2
  size_t in_inner2;
  uint32_t in_group2;
  size_t out_outer, out_inner;
  uint32_t out_group;
  size_t out_inner2;         // second grouping level of the output, like in_group2 / in_inner2
  uint32_t out_group2;
  size_t pre_inner;          // the pre-scale table of array q starts at (q % in_group) * pre_inner
  const fl* tw_small;        // omega_len^i, i < len/2, unpacked limbs
  const fe* tw_full;         // omega_N^e, e < N (col pass twiddles); may be null for row pass
  const fe* pre_scale;       // indexed by global input index, or null
  const fe* post_scale;      // indexed by global output index, or null
  fe post_scalar;            // used when use_post_scalar
  uint32_t use_post_scalar;
  uint32_t tw_scaled;        // col pass: tw_full is the 1/n-scaled inverse table - entry 0 is 1/n, not 1: no product is skipped
  uint32_t lazy_out;         // row pass: leave results weakly reduced (< 2r) instead of canonical
  uint32_t log_n;
  uint32_t log_len;          // sub-transform size
  uint32_t log_c;            // tile width
  uint32_t log_m;            // col pass: segment size
  uint32_t log_n1, log_n2;   // row pass: digit sizes of the leading digits
  // persistent launch: tiles_x * tiles_y tiles are handed out by *tile_counter to a fixed number of workgroups (null:
  // one workgroup per tile, blockIdx = tile)
  uint32_t* tile_counter;
  uint32_t tiles_x, tiles_y;
};

// the tile a workgroup works on next: (blockIdx.x, blockIdx.y) once, or the next one from the counter; false: none left
__device__ __forceinline__ bool next_tile(const PassParams& p, uint32_t round, uint32_t& bx, uint32_t& by) {
  if (!p.tile_counter) {
    bx = blockIdx.x;
    by = blockIdx.y;
    return round == 0;
  }
  __shared__ uint32_t tile_s;
  __syncthreads();  // (everybody is done with the LDS tile and with tile_s of the round before)
  if (threadIdx.x == 0) tile_s = atomicAdd(p.tile_counter, 1u);
  __syncthreads();
  const uint32_t t = tile_s;
  if (t >= p.tiles_x * p.tiles_y) return false;
  bx = t % p.tiles_x;
  by = t / p.tiles_x;
  return true;
}

__device__ __forceinline__ uint32_t bitrev32(uint32_t x, uint32_t bits) { return __brev(x) >> (32 - bits); }

// DIT stages on sh[len][C] (rows were written bit-reversed): natural order out.
// Lazy 29-bit field: per butterfly  t = v * w (one Montgomery product, < 1.2p),  (u + t, u + 2p - t); values
// grow by at most 2p per stage (<= 2p * 11 stages + input), far below the 169p capacity of 9 x 29-bit limbs.
// Twiddles are stored in the internal Montgomery form (w * 2^261), so data keeps whatever form it came in.
//
// Stage plan: one radix-2 stage when the stage count is odd, then radix-4 rounds (stages s, s + 1 on four rows held in
// registers: the same multiplications as two radix-2 stages at half the LDS traffic, index arithmetic and barriers -
// 147 instead of 216 instructions per element and stage).  The first round of an even-length transform (s = 0) has
// trivial twiddles - 1, 1 and omega_4 - and, for the prover's zero-padded inputs (a polynomial of n + 2 coefficients on a
// 2n-point coset: rows len/2.. are zero), two zero operands: ONE multiplication for its four elements instead of four.
// Round 6 (round-5 VERDICT item 4): the butterflies' twiddle products are constant-multiplicand products (Fl::mul_shoup,
// independent column accumulators: 143 multiply-adds and no serial digit chain against the Montgomery product's 171).
// tw_small holds PAIRS - entry i at [2i] the plain canonical twiddle, at [2i + 1] its quotient floor(w 2^261 / p) - and a
// product is below 5p instead of 1.2p: the subtractions add 8p instead of 2p, and values grow by at most 16p per radix-4
// round (row 3 leaves as a + 8p - t + 8p - t', and zero padding makes both products zero), 10p in the s = 0 round, 2p
// in the lone radix-2 stage: at most 87.3p behind the last of five rounds for inputs below 2^256, against the 169p the
// limbs hold (tests/golden/lazy_envelope.json has the bound at every store).  Everything outside the radix-4 rounds - coset
// pre-scale, inter-pass twiddle, post-scale: factors from 32-byte tables - stays a Montgomery product.  Measured on one
// box (profiles/ntt_shoup_ab_r06.txt): 768 x 2^16 coset transforms 4.17 -> 4.03 ms, column + row pass per headline step
// 35.7 -> 34.3 ms, 1373 -> 1387 proofs/s; the microbenchmark behind the decision: profiles/ubench_shoup29_r06.txt.
// -DCAP_NTT_NO_SHOUP builds the Montgomery rounds of rounds 1-5.
// The stage bodies are the templates of ntt_elem29.hpp (shared with the host twin and the bound run); the stage loop
// and the barriers stay here.
#ifndef CAP_NTT_NO_SHOUP
constexpr bool kNttShoup = true;
#else
constexpr bool kNttShoup = false;
#endif
constexpr int kTwStride = NttTw<Fr29, fl, kNttShoup>::kStride;
__device__ __forceinline__ void lds_ntt(fl* sh, const fl* __restrict__ tw_small, uint32_t log_len, uint32_t log_c) {
  const uint32_t s0 = log_len & 1;
  if (s0) {
    ntt_stage_radix2<Fr29, fl>(sh, log_len, log_c, threadIdx.x, kThreads);
    __syncthreads();
  }
  for (uint32_t s = s0; s + 1 < log_len; s += 2) {
    ntt_stage_radix4<Fr29, fl, kNttShoup>(sh, tw_small, log_len, log_c, s, threadIdx.x, kThreads);
    __syncthreads();
  }
}

// column pass: len rows at stride S = M/len, C adjacent columns per tile
__device__ __forceinline__ void col_tile(const PassParams& p, fl* sh, const uint32_t bx, const uint32_t by) {
  {
  const uint32_t log_s = p.log_m - p.log_len;           // columns per segment (log)
  const uint32_t tiles_per_seg_log = log_s - p.log_c;
  const uint32_t t = bx;
  const size_t seg = t >> tiles_per_seg_log;
  const uint32_t col0 = (t & ((1u << tiles_per_seg_log) - 1)) << p.log_c;
  const uint32_t q2 = by / p.in_group;
  const fe* in = p.in + (size_t)(q2 / p.in_group2) * p.in_outer + (size_t)(q2 % p.in_group2) * p.in_inner2 +
                 (size_t)(by % p.in_group) * p.in_inner;
  const uint32_t o2 = by / p.out_group;
  fe* out = p.out + (size_t)(o2 / p.out_group2) * p.out_outer + (size_t)(o2 % p.out_group2) * p.out_inner2 +
            (size_t)(by % p.out_group) * p.out_inner;
  const size_t base = (seg << p.log_m) + col0;
  const uint32_t tile = 1u << (p.log_len + p.log_c);
  const uint32_t cmask = (1u << p.log_c) - 1;
  // kIoBatch elements per thread and round, their global loads (and the loads of their coset factors) issued together
  // before any of them is used (the loop used to be load - wait - multiply - store, one element at a time)
  for (uint32_t e0 = threadIdx.x; e0 < tile; e0 += kIoBatch * kThreads) {
    fe raw[kIoBatch], pre[kIoBatch];
    uint32_t any[kIoBatch];
    size_t sgs[kIoBatch];
#pragma unroll
    for (int u = 0; u < kIoBatch; u++) {
      const uint32_t e = e0 + u * kThreads;
      const uint32_t c = e & cmask, j = e >> p.log_c;
      const size_t g = base + ((size_t)j << log_s) + c;
      // position inside the source array (decimated input: every in_es-th element, starting at the group offset)
      const size_t sg = p.in_es == 1 ? g : g * p.in_es + (size_t)(by % p.in_group) * p.in_inner;
      sgs[u] = sg;
      any[u] = 0;
      if (e < tile && sg < p.in_len) {
        raw[u] = p.in_es == 1 ? in[g] : in[g * p.in_es];
        any[u] = 1;
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) raw[u].v[k] = 0;
      }
    }
    if (p.pre_scale) {
#pragma unroll
      for (int u = 0; u < kIoBatch; u++)
        if (any[u]) pre[u] = p.pre_scale[sgs[u] + (size_t)(by % p.in_group) * p.pre_inner];
    }
#pragma unroll
    for (int u = 0; u < kIoBatch; u++) {
      const uint32_t e = e0 + u * kThreads;
      if (e >= tile) break;
      const uint32_t c = e & cmask, j = e >> p.log_c;
      // zero padding needs no coset scaling; in_fold: the few coefficients beyond the transform's length, folded in
      const fl v = ntt_in_elem<Fr29, fl, fe>(raw[u], p.pre_scale && any[u], pre[u],
                                             p.in_fold && sgs[u] + p.in_fold < p.in_len, in, sgs[u] + p.in_fold, p.pre_scale,
                                             sgs[u] + p.in_fold + (size_t)(by % p.in_group) * p.pre_inner);
      sh[(bitrev32(j, p.log_len) << p.log_c) + c] = v;
    }
  }
  __syncthreads();
  lds_ntt(sh, p.tw_small, p.log_len, p.log_c);
  const uint32_t tw_shift = p.log_n - p.log_m;  // omega_M^x = omega_N^(x << tw_shift)
  for (uint32_t e0 = threadIdx.x; e0 < tile; e0 += kIoBatch * kThreads) {
    fe tw[kIoBatch];
    size_t exs[kIoBatch];
#pragma unroll
    for (int u = 0; u < kIoBatch; u++) {  // the inter-pass twiddles of the batch: gathers from a 2 MB table, in flight together
      const uint32_t e = e0 + u * kThreads;
      const uint32_t c = e & cmask, k = e >> p.log_c;
      exs[u] = e < tile ? ((size_t)(col0 + c) * k) << tw_shift : 0;
      if (exs[u] || p.tw_scaled) tw[u] = p.tw_full[exs[u]];
    }
#pragma unroll
    for (int u = 0; u < kIoBatch; u++) {
      const uint32_t e = e0 + u * kThreads;
      if (e >= tile) break;
      const uint32_t c = e & cmask, k = e >> p.log_c;
      out[base + ((size_t)k << log_s) + c] = ntt_out_col<Fr29, fl, fe>(sh[e], exs[u] || p.tw_scaled, tw[u]);   // < 2p: fits the 32-byte image
    }
  }
  }
}
// PERSIST: a fixed number of workgroups take tile after tile from a counter (next_tile); otherwise one tile per workgroup.
// Two instantiations, because the loop around the tile costs the one-shot form 55 VGPRs (93 -> 148: three waves per SIMD).
template <bool PERSIST>
__global__ __launch_bounds__(kThreads) CAP_NTT_ATTR void ntt_col_pass(PassParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  fl* sh = reinterpret_cast<fl*>(smem);
  if constexpr (!PERSIST) {
    col_tile(p, sh, blockIdx.x, blockIdx.y);
  } else {
    uint32_t bx, by;
    for (uint32_t round = 0; next_tile(p, round, bx, by); round++) col_tile(p, sh, bx, by);
  }
}

// row pass: contiguous rows of len elements; C rows with adjacent k1 per tile; digit-reversed store
__device__ __forceinline__ void row_tile(const PassParams& p, fl* sh, const uint32_t bx, const uint32_t by) {
  {
  const uint32_t t = bx;
  const uint32_t k2 = t & ((1u << p.log_n2) - 1);
  const uint32_t r0 = (t >> p.log_n2) << p.log_c;
  const uint32_t q2 = by / p.in_group;
  const fe* in = p.in + (size_t)(q2 / p.in_group2) * p.in_outer + (size_t)(q2 % p.in_group2) * p.in_inner2 +
                 (size_t)(by % p.in_group) * p.in_inner;
  const uint32_t o2 = by / p.out_group;
  fe* out = p.out + (size_t)(o2 / p.out_group2) * p.out_outer + (size_t)(o2 % p.out_group2) * p.out_inner2 +
            (size_t)(by % p.out_group) * p.out_inner;
  const uint32_t tile = 1u << (p.log_len + p.log_c);
  const uint32_t lmask = (1u << p.log_len) - 1;
  const uint32_t cmask = (1u << p.log_c) - 1;
  for (uint32_t e0 = threadIdx.x; e0 < tile; e0 += kIoBatch * kThreads) {  // batched loads: see ntt_col_pass
    fe raw[kIoBatch], pre[kIoBatch];
    uint32_t any[kIoBatch];
    size_t sgs[kIoBatch];
#pragma unroll
    for (int u = 0; u < kIoBatch; u++) {
      const uint32_t e = e0 + u * kThreads;
      const uint32_t j = e & lmask, c = e >> p.log_len;
      const size_t g = ((((size_t)(r0 + c) << p.log_n2) + k2) << p.log_len) + j;
      const size_t sg = p.in_es == 1 ? g : g * p.in_es + (size_t)(by % p.in_group) * p.in_inner;
      sgs[u] = sg;
      any[u] = 0;
      if (e < tile && sg < p.in_len) {
        raw[u] = p.in_es == 1 ? in[g] : in[g * p.in_es];
        any[u] = 1;
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) raw[u].v[k] = 0;
      }
    }
    if (p.pre_scale) {
#pragma unroll
      for (int u = 0; u < kIoBatch; u++)
        if (any[u]) pre[u] = p.pre_scale[sgs[u] + (size_t)(by % p.in_group) * p.pre_inner];
    }
#pragma unroll
    for (int u = 0; u < kIoBatch; u++) {
      const uint32_t e = e0 + u * kThreads;
      if (e >= tile) break;
      const uint32_t j = e & lmask, c = e >> p.log_len;
      // zero padding needs no coset scaling; in_fold: the few coefficients beyond the transform's length, folded in
      const fl v = ntt_in_elem<Fr29, fl, fe>(raw[u], p.pre_scale && any[u], pre[u],
                                             p.in_fold && sgs[u] + p.in_fold < p.in_len, in, sgs[u] + p.in_fold, p.pre_scale,
                                             sgs[u] + p.in_fold + (size_t)(by % p.in_group) * p.pre_inner);
      sh[(bitrev32(j, p.log_len) << p.log_c) + c] = v;
    }
  }
  __syncthreads();
  lds_ntt(sh, p.tw_small, p.log_len, p.log_c);
  for (uint32_t e = threadIdx.x; e < tile; e += kThreads) {
    uint32_t c = e & cmask, k = e >> p.log_c;
    fl v = sh[e];
    size_t g = (size_t)(r0 + c) + ((size_t)k2 << p.log_n1) + ((size_t)k << (p.log_n1 + p.log_n2));
    if (p.post_scale) v = ntt_scale_elem<Fr29, fl, fe>(v, p.post_scale[g]);
    else if (p.use_post_scalar) v = ntt_scale_elem<Fr29, fl, fe>(v, p.post_scalar);
    // (a plain inverse transform of two or more passes took its 1/n with the inter-pass twiddles - ntt_run - and, like
    // a forward transform, arrives here straight from the butterflies: normalized limbs, far below the 169p that store
    // and canonical take)
    // results leave the transform canonical (< r), as arkworks stores them - except the internal-form coset
    // evaluations, whose only reader (k_quotient) takes any representative below 2^256
    out[g] = ntt_out_row<Fr29, fl, fe>(v, p.lazy_out);
  }
  }
}
template <bool PERSIST>
__global__ __launch_bounds__(kThreads) CAP_NTT_ATTR void ntt_row_pass(PassParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  fl* sh = reinterpret_cast<fl*>(smem);
  if constexpr (!PERSIST) {
    row_tile(p, sh, blockIdx.x, blockIdx.y);
  } else {
    uint32_t bx, by;
    for (uint32_t round = 0; next_tile(p, round, bx, by); round++) row_tile(p, sh, bx, by);
  }
}

// tw_small: the internal-form table `in` (x * 2^261, canonical) as the limbs the butterflies multiply by - kTwStride = 1:
// the same values unpacked; kTwStride = 2 (CAP_NTT_SHOUP): pairs (plain canonical x, floor(x 2^261 / p))
__global__ void table_unpack(fl* __restrict__ out, const fe* __restrict__ in, size_t n) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if constexpr (kTwStride == 1) {
    out[e] = Fr29::load(in[e]);
  } else {
    const fl t = Fr29::load(in[e]);
    out[2 * e] = Fr29::load(Fr29::from_mont(t));
    out[2 * e + 1] = Fr29::shoup_quotient(t);
  }
}

// internal-form table: out[e] = pack(canonical(in_ext[e] * 2^5))  (x * 2^256 -> x * 2^261)
__global__ void table_to_internal(fe* __restrict__ out, const fe* __restrict__ in, size_t n) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  out[e] = Fr29::pack(Fr29::canonical(Fr29::from_ext(in[e])));
}

// out[e] = base^e * scale for e < n; pw[b] = base^(2^b)
__global__ void powers_table(fe* out, size_t n, const fe* __restrict__ pw, fe scale, int has_scale) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  fe r = has_scale ? scale : Fr::one();
  bool started = has_scale;
  for (int b = 0; (e >> b) != 0; b++) {
    if ((e >> b) & 1) {
      r = started ? Fr::mul(r, pw[b]) : pw[b];
      started = true;
    }
  }
  out[e] = r;
}

// ---- radix-3 stage of the N = 3 M transforms -------------------------------------------------------------------
// y: [count][3][M] sub-transform outputs (lazy, internal form).  out: array q at (q / group) * outer + (q % group) * inner.
//   X[k + M b] = Y0 + w3^b T1 + w3^(2b) T2,  T1 = omega_N^k Y1[k], T2 = omega_N^(2k) Y2[k];  with w3^2 = -1 - w3:
//   X[k] = Y0 + T1 + T2,  X[k + M] = Y0 - T2 + D,  X[k + 2M] = Y0 - T1 - D,  D = w3 (T1 - T2)     (3 multiplications)
// post != null (inverse transform): every output is multiplied by post[index] (an arkworks-form integer table, which
// takes internal-form data to arkworks' form) and leaves canonical; otherwise outputs leave weakly reduced.
// add != null (with post only): [count][M / 2] arkworks-form values (< r); output k + M b of array q takes
// add[q][k mod M / 2] after the post product - one load serves the thread's three outputs.
__global__ __launch_bounds__(kThreads) void ntt3_combine(const fe* __restrict__ y, fe* __restrict__ out, size_t out_outer,
                                                         size_t out_inner, uint32_t out_group, size_t m_len,
                                                         const fe* __restrict__ tw, fe w3, const fe* __restrict__ post,
                                                         const fe* __restrict__ add) {
  using F = Fr29;
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m_len) return;
  const uint32_t q = blockIdx.y;
  const fe* yq = y + (size_t)q * 3 * m_len;
  fe* o = out + (size_t)(q / out_group) * out_outer + (size_t)(q % out_group) * out_inner;
  fl x0, x1, x2;
  ntt3_combine_elem<F, fl, fe>(yq[k], yq[m_len + k], tw[k], yq[2 * m_len + k], tw[2 * k], w3, x0, x1, x2);
  if (post) {
    // products < 2p plus a value < p: normalized and well inside what canonical takes
    const size_t half = m_len >> 1;
    const fl a = add ? F::load(add[(size_t)q * half + (k & (half - 1))]) : F::zero();
    auto finish = [&](const fl& x, const fe& ps) { return ntt3_finish_elem<F, fl, fe>(x, ps, add != nullptr, a); };
    o[k] = finish(x0, post[k]);
    o[m_len + k] = finish(x1, post[m_len + k]);
    o[2 * m_len + k] = finish(x2, post[2 * m_len + k]);
  } else {
    o[k] = F::store(x0);
    o[m_len + k] = F::store(x1);
    o[2 * m_len + k] = F::store(x2);
  }
}

// ---- the solve of the five-coset inverse (ntt.hpp: Quot5Const) ----------------------------------------------------
// y01: [count][2][M] outputs of the inverse M-point transforms of blocks 0 and 1, y2: [count][M / 2] of the inverse
// M / 2-point transform of the compact block 2 (lazy, internal form).  out: array q at q * 3 M, all 3 M coefficients.
// One thread per i < n = M / 2 writes coefficients i, n + i, .. 5n + i:  un-scaling (the table changes the form as
// well: arkworks' from here on), the fixed 2 x 2 and 3 x 5 products, d_j add[q][i], and for i < 8 mt_j top[q][i];
// coefficient 5n + i is top[q][i] for i < 8 and zero beyond.  Canonical outputs.
__global__ __launch_bounds__(kThreads) void ntt3_combine5(const fe* __restrict__ y01, const fe* __restrict__ y2,
                                                          fe* __restrict__ out, size_t n_len,
                                                          const fe* __restrict__ unscale, Quot5Const qc,
                                                          const fe* __restrict__ top, const fe* __restrict__ add) {
  using F = Fr29;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_len) return;
  const uint32_t q = blockIdx.y;
  const size_t m_len = 2 * n_len;
  const fe* ya = y01 + (size_t)q * 2 * m_len;
  fe* o = out + (size_t)q * 3 * m_len;
  const fl e0 = ntt_scale_elem<F, fl, fe>(F::load(ya[i]), unscale[i]);
  const fl o0 = ntt_scale_elem<F, fl, fe>(F::load(ya[n_len + i]), unscale[n_len + i]);
  const fl e1 = ntt_scale_elem<F, fl, fe>(F::load(ya[m_len + i]), unscale[m_len + i]);
  const fl o1 = ntt_scale_elem<F, fl, fe>(F::load(ya[m_len + n_len + i]), unscale[m_len + n_len + i]);
  const fl r = ntt_scale_elem<F, fl, fe>(F::load(y2[(size_t)q * n_len + i]), unscale[2 * m_len + i]);
  const bool has_top = i < 8;
  fl pi = F::zero(), h = F::zero();
  if (add) pi = F::load(add[(size_t)q * n_len + i]);
  if (has_top) h = F::load(top[(size_t)q * 8 + i]);
  // sums of at most four reduced values (< 2p each, normalized): limbs < 2^31, well inside what normalize and canonical take
  using E = Ntt5Elem<F, fl, fe, Quot5Const>;
  for (int jj = 0; jj < 2; jj++)
    o[(size_t)(2 * jj + 1) * n_len + i] = E::odd(jj, o0, o1, add != nullptr, pi, has_top, h, qc);
  for (int jj = 0; jj < 3; jj++)
    o[(size_t)(2 * jj) * n_len + i] = E::even(jj, e0, o0, e1, o1, r, add != nullptr, pi, has_top, h, qc);
  fe t5 = Fr::zero();
  if (has_top) t5 = top[(size_t)q * 8 + i];
  o[5 * n_len + i] = t5;
}

fe host_root_of_unity(uint32_t log_n) {
  // omega_28 = 5^((r-1)/2^28), canonical little-endian limbs
  fe w;
  const uint32_t root28[8] = {0x725b19f0u, 0x9bd61b6eu, 0x41112ed4u, 0x402d111eu,
                              0x8ef62abcu, 0x00e0a7ebu, 0xa58a7e85u, 0x2a3c09f0u};
  for (int i = 0; i < 8; i++) w.v[i] = root28[i];
  w = Fr::to_mont(w);
  for (uint32_t i = log_n; i < 28; i++) w = Fr::sqr(w);
  return w;
}

fe host_from_u64(uint64_t v) {
  fe t = Fr::zero();
  t.v[0] = (uint32_t)v;
  t.v[1] = (uint32_t)(v >> 32);
  return Fr::to_mont(t);
}

int build_powers(fe* d_out, size_t n, fe base, const fe* scale, hipStream_t stream) {
  std::vector<fe> pw(40);
  fe x = base;
  for (int b = 0; b < 40; b++) {
    pw[b] = x;
    x = Fr::sqr(x);
  }
  fe* d_pw = nullptr;
  hipError_t e = hipMalloc(&d_pw, sizeof(fe) * pw.size());
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyAsync(d_pw, pw.data(), sizeof(fe) * pw.size(), hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return (int)e;
  fe sc = scale ? *scale : Fr::one();
  size_t blocks = (n + 255) / 256;
  launch("powers_table", powers_table, dim3((unsigned)blocks), dim3(256), 0, stream, d_out, n, d_pw, sc, scale ? 1 : 0);
  e = hipStreamSynchronize(stream);
  hipFree(d_pw);
  return (int)e;
}

}  // namespace

fe ntt_root_of_unity(uint32_t log_n) { return host_root_of_unity(log_n); }

int ntt_build_small_tables(NttSmallTables* t, hipStream_t stream) {
  if (!t->pass_counters) {
    hipError_t ec = hipMalloc(&t->pass_counters, sizeof(uint32_t) * kNttPassCounters);
    if (ec != hipSuccess) return (int)ec;
  }
  for (int s = 1; s <= kMaxLogTile; s++) {
    size_t n = (size_t)1 << (s - 1);
    hipError_t e = hipMalloc(&t->fwd[s], sizeof(fe) * n);
    if (e != hipSuccess) return (int)e;
    e = hipMalloc(&t->inv[s], sizeof(fe) * n);
    if (e != hipSuccess) return (int)e;
    fe w = host_root_of_unity(s);
    int rc = build_powers(t->fwd[s], n, w, nullptr, stream);
    if (rc) return rc;
    rc = build_powers(t->inv[s], n, Fr::inv(w), nullptr, stream);
    if (rc) return rc;
    launch("table_to_internal", table_to_internal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, t->fwd[s],
           (const fe*)t->fwd[s], n);
    launch("table_to_internal", table_to_internal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, t->inv[s],
           (const fe*)t->inv[s], n);
    for (int d = 0; d < 2; d++) {
      uint32_t** dst = d ? &t->inv_u[s] : &t->fwd_u[s];
      e = hipMalloc(dst, sizeof(fl) * n * kTwStride);
      if (e != hipSuccess) return (int)e;
      launch("table_unpack", table_unpack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
             reinterpret_cast<fl*>(*dst), (const fe*)(d ? t->inv[s] : t->fwd[s]), n);
    }
    hipError_t es = hipStreamSynchronize(stream);
    if (es != hipSuccess) return (int)es;
  }
  return 0;
}

void ntt_free_small_tables(NttSmallTables* t) {
  if (t->pass_counters) hipFree(t->pass_counters);
  t->pass_counters = nullptr;
  for (int s = 0; s <= kMaxLogTile; s++) {
    if (t->fwd[s]) hipFree(t->fwd[s]);
    if (t->inv[s]) hipFree(t->inv[s]);
    if (t->fwd_u[s]) hipFree(t->fwd_u[s]);
    if (t->inv_u[s]) hipFree(t->inv_u[s]);
    t->fwd[s] = t->inv[s] = nullptr;
    t->fwd_u[s] = t->inv_u[s] = nullptr;
  }
}

int ntt_build_domain(NttDomain* d, uint32_t log_n, hipStream_t stream) {
  d->log_n = log_n;
  size_t n = (size_t)1 << log_n;
  hipError_t e;
  if ((e = hipMalloc(&d->tw_fwd, sizeof(fe) * n)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d->tw_inv, sizeof(fe) * n)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d->coset_fwd, sizeof(fe) * n)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d->coset_inv, sizeof(fe) * n)) != hipSuccess) return (int)e;
  fe w = host_root_of_unity(log_n);
  fe g = host_from_u64(5);
  d->n_inv = Fr::inv(host_from_u64((uint64_t)n));
  int rc;
  if ((rc = build_powers(d->tw_fwd, n, w, nullptr, stream))) return rc;
  if ((rc = build_powers(d->tw_inv, n, Fr::inv(w), nullptr, stream))) return rc;
  if ((rc = build_powers(d->coset_fwd, n, g, nullptr, stream))) return rc;
  if ((rc = build_powers(d->coset_inv, n, Fr::inv(g), &d->n_inv, stream))) return rc;
  fe* src[4] = {d->tw_fwd, d->tw_inv, d->coset_fwd, d->coset_inv};
  fe** dst[4] = {&d->tw29_fwd, &d->tw29_inv, &d->coset29_fwd, &d->coset29_inv};
#ifndef CAP_NTT_NO_INV_FOLD
  // omega^-e / n: the inter-pass twiddles of a plain inverse transform, its 1/n folded in (ntt_run)
  if ((e = hipMalloc(&d->tw29_inv_n, sizeof(fe) * n)) != hipSuccess) return (int)e;
  if ((rc = build_powers(d->tw29_inv_n, n, Fr::inv(w), &d->n_inv, stream))) return rc;
  launch("table_to_internal", table_to_internal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d->tw29_inv_n,
         (const fe*)d->tw29_inv_n, n);
#endif
  for (int k = 0; k < 4; k++) {
    if ((e = hipMalloc(dst[k], sizeof(fe) * n)) != hipSuccess) return (int)e;
    launch("table_to_internal", table_to_internal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *dst[k],
           (const fe*)src[k], n);
  }
  d->n_inv29 = Fr29::pack(Fr29::canonical(Fr29::from_ext(d->n_inv)));
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return (int)e;
  // only omega^j (tw_fwd) is still read in arkworks' form (by the prover's elementwise kernels)
  hipFree(d->tw_inv);
  hipFree(d->coset_fwd);
  hipFree(d->coset_inv);
  d->tw_inv = d->coset_fwd = d->coset_inv = nullptr;
  return 0;
}

void ntt_free_domain(NttDomain* d) {
  if (d->tw_fwd) hipFree(d->tw_fwd);
  if (d->tw_inv) hipFree(d->tw_inv);
  if (d->coset_fwd) hipFree(d->coset_fwd);
  if (d->coset_inv) hipFree(d->coset_inv);
  for (fe* t : {d->tw29_fwd, d->tw29_inv, d->tw29_inv_n, d->coset29_fwd, d->coset29_inv})
    if (t) hipFree(t);
  d->tw_fwd = d->tw_inv = d->coset_fwd = d->coset_inv = nullptr;
  d->tw29_fwd = d->tw29_inv = d->tw29_inv_n = d->coset29_fwd = d->coset29_inv = nullptr;
}

void ntt_table_to_internal(fe* out, const fe* in, size_t n, hipStream_t stream) {
  if (n == 0) return;
  launch("table_to_internal", table_to_internal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out, in, n);
}

namespace {
// Workgroups per CU of a persistent pass launch (CAPGPU_NTT_PERSISTENT; 0 = one workgroup per tile)
unsigned ntt_persistent() {
  static const unsigned v = [] {
    const char* e = getenv("CAPGPU_NTT_PERSISTENT");
    const long x = e ? atol(e) : 0;
    return (unsigned)(x >= 1 && x <= 16 ? x : 0);
  }();
  return v;
}
template <class K>
void launch_pass(const char* name, K kernel, K kernel_persistent, PassParams& p, const NttSmallTables& small, size_t tiles,
                 uint32_t count, size_t lds, bool persistent, hipStream_t stream) {
  p.tile_counter = nullptr;
  p.tiles_x = (uint32_t)tiles;
  p.tiles_y = count;
  if (persistent) {
    // the plan says persistent, and capgpu_ntt_plan reports it: a pass that cannot get its tile counter is an error of
    // the call (latched like a failed launch), not a quiet one-shot launch
    uint32_t* ctr = small.pass_counters ? small.pass_counters + (small.next_counter++ % kNttPassCounters) : nullptr;
    const hipError_t e = ctr ? hipMemsetAsync(ctr, 0, sizeof(uint32_t), stream) : hipErrorInvalidValue;
    if (e != hipSuccess) {
      (void)hipGetLastError();
      LaunchError& le = launch_error();
      if (le.code == hipSuccess) {
        le.code = e;
        le.kernel = name;
      }
      return;
    }
    p.tile_counter = ctr;
    launch(name, kernel_persistent, dim3(256u * ntt_persistent()), dim3(kThreads), lds, stream, p);
    return;
  }
  launch(name, kernel, dim3((unsigned)tiles, count), dim3(kThreads), lds, stream, p);
}
}  // namespace

int ntt_plan(uint32_t log_n, uint32_t count, NttPlan* out) {
  NttPlan pl{};
  if (log_n == 0 || count == 0) {  // n = 1 is the identity in every mode: nothing is launched
    *out = pl;
    return 0;
  }
  pl.tile_log = tile_log_for(log_n, count);
  // digit split
  uint32_t lg[3] = {0, 0, 0};
  if (log_n <= 10) {
    pl.passes = 1;
    lg[2] = log_n;
  } else if (log_n <= 20) {
    pl.passes = 2;
    lg[0] = (log_n + 1) / 2;
    lg[2] = log_n / 2;
  } else {
    pl.passes = 3;
    lg[0] = (log_n + 2) / 3;
    lg[1] = (log_n - lg[0] + 1) / 2;
    lg[2] = log_n - lg[0] - lg[1];
  }
  if (lg[0] > 10 || lg[1] > 10 || lg[2] > 10) return (int)hipErrorInvalidValue;
  const unsigned per_cu = ntt_persistent();
  auto finish = [&](uint32_t i, uint32_t log_len, uint32_t log_c) {
    pl.digits[i] = log_len;
    pl.log_c[i] = log_c;
    pl.tiles[i] = (uint64_t)1 << (log_n - log_len - log_c);
    const uint64_t total = pl.tiles[i] * count;
    pl.persistent[i] = per_cu && total > 4ull * 256 * per_cu && total < (1ull << 32);
  };
  // column passes: the tile is C adjacent columns of a segment of 2^log_m elements
  uint32_t log_m = log_n;
  for (uint32_t d = 0; d + 1 < pl.passes; d++) {
    const uint32_t log_len = lg[d];
    const uint32_t log_s = log_m - log_len;
    uint32_t log_c = pl.tile_log > log_len ? pl.tile_log - log_len : 0;
    if (log_c > log_s) log_c = log_s;
    if (log_c > 4) log_c = 4;
    finish(d, log_len, log_c);
    log_m -= log_len;
  }
  // row pass: the tile is C rows with adjacent leading digit
  {
    const uint32_t log_len = lg[2];
    const uint32_t log_n1 = pl.passes >= 2 ? lg[0] : 0;
    uint32_t log_c = pl.tile_log > log_len ? pl.tile_log - log_len : 0;
    if (log_c > log_n1) log_c = log_n1;
    if (log_c > 4) log_c = 4;
    finish(pl.passes - 1, log_len, log_c);
  }
  *out = pl;
  return 0;
}

int ntt_run(const NttDomain& dom, const NttSmallTables& small, fe* data, fe* scratch, size_t stride_elems,
            uint32_t count, int dir, int coset, hipStream_t stream, const NttIo* io) {
  const uint32_t log_n = dom.log_n;
  if (count == 0) return 0;
  if (log_n == 0) {
    // n = 1: forward is the identity (5^0 = 1); inverse multiplies by 1^-1 = 1.
    return 0;
  }
  NttPlan plan;
  if (int rc = ntt_plan(log_n, count, &plan)) return rc;
  const int passes = (int)plan.passes;
  uint32_t* const* tws = dir ? small.inv_u : small.fwd_u;
  const fe* tw_full = dir ? dom.tw29_inv : dom.tw29_fwd;

  PassParams p{};
  // first-pass input and last-pass output addressing; the passes in between go through the scratch buffer
  const size_t scratch_stride = io ? ((size_t)1 << log_n) : stride_elems;
  struct Addr {
    size_t outer, inner;
    uint32_t group;
  };
  const Addr a_src = io ? Addr{io->src_outer, io->src_inner, io->src_group ? io->src_group : 1u} : Addr{stride_elems, 0, 1};
  const Addr a_dst = io ? Addr{io->dst_outer, io->dst_inner, io->dst_group ? io->dst_group : 1u} : Addr{stride_elems, 0, 1};
  const Addr a_tmp = Addr{scratch_stride, 0, 1};
  const size_t src_len = io ? io->src_len : ~(size_t)0;
  const size_t src_fold = io ? io->src_fold : 0;
  if (src_fold && (!io->pre_scale || (io->src_elem_stride > 1) || src_fold + ((size_t)1 << log_n) < io->src_len))
    return (int)hipErrorInvalidValue;  // one fold only, of contiguous pre-scaled input
  auto set_in = [&](const Addr& a, size_t len, uint32_t es) {
    p.in_fold = &a == &a_src ? src_fold : 0;
    p.in_outer = a.outer;
    p.in_inner = a.inner;
    p.in_group = a.group;
    p.in_len = len;
    p.in_es = es;
    p.in_group2 = 1;
    p.in_inner2 = 0;
    if (&a == &a_src && io && io->src_group2 > 1) {
      p.in_group2 = io->src_group2;
      p.in_inner2 = io->src_inner2;
    }
  };
  const uint32_t src_es = io && io->src_elem_stride ? io->src_elem_stride : 1;
  auto set_out = [&](const Addr& a) {
    p.out_outer = a.outer;
    p.out_inner = a.inner;
    p.out_group = a.group;
    p.out_group2 = 1;
    p.out_inner2 = 0;
    if (&a == &a_dst && io && io->dst_group2 > 1) {
      p.out_group2 = io->dst_group2;
      p.out_inner2 = io->dst_inner2;
    }
  };
  p.pre_inner = io ? io->pre_inner : 0;
  p.log_n = log_n;
  p.tw_full = tw_full;
  p.use_post_scalar = 0;
  // A plain inverse transform of two or more passes that ends in the domain's own 1/n takes it with the inter-pass
  // twiddles of its first column pass (tw29_inv_n[e] = omega^-e / n: the product is there anyway) and its row pass
  // multiplies by nothing.  One-pass transforms have no column pass, coset inverses carry 1/n in coset29_inv, and a
  // caller's own post_scalar (the public-input fold's kappa / n) stays a product of the row pass.
#ifndef CAP_NTT_NO_INV_FOLD
  const bool inv_fold = dir && !coset && passes >= 2 && !(io && io->has_post_scalar) && dom.tw29_inv_n;
#else
  const bool inv_fold = false;
#endif

  const fe* pre = (!dir && coset) ? dom.coset29_fwd : nullptr;
  if (io && io->pre_scale) pre = io->pre_scale;
  bool first = true;
  const fe* cur_in = io ? io->src : data;
  // column passes
  uint32_t log_m = log_n;
  for (int d = 0; d < passes - 1; d++) {
    const uint32_t log_len = plan.digits[d], log_c = plan.log_c[d];
    p.in = cur_in;
    p.out = scratch;
    set_in(first ? a_src : a_tmp, first ? src_len : ~(size_t)0, first ? src_es : 1);
    set_out(a_tmp);
    p.tw_small = reinterpret_cast<const fl*>(tws[log_len]);
    p.pre_scale = first ? pre : nullptr;
    p.post_scale = nullptr;
    p.log_len = log_len;
    p.log_c = log_c;
    p.log_m = log_m;
    p.tw_full = (inv_fold && d == 0) ? dom.tw29_inv_n : tw_full;
    p.tw_scaled = (inv_fold && d == 0) ? 1 : 0;
    size_t lds = sizeof(fl) << (log_len + log_c);
    launch_pass("ntt_col_pass", ntt_col_pass<false>, ntt_col_pass<true>, p, small, (size_t)plan.tiles[d], count, lds,
                plan.persistent[d] != 0, stream);
    cur_in = scratch;
    first = false;
    log_m -= log_len;
  }
  // row pass
  {
    const int last = passes - 1;
    const uint32_t log_len = plan.digits[last], log_c = plan.log_c[last];
    const uint32_t log_n1 = passes >= 2 ? plan.digits[0] : 0;
    const uint32_t log_n2 = passes == 3 ? plan.digits[1] : 0;
    p.in = cur_in;
    p.out = data;
    set_in(first ? a_src : a_tmp, first ? src_len : ~(size_t)0, first ? src_es : 1);
    set_out(a_dst);
    p.tw_small = reinterpret_cast<const fl*>(tws[log_len]);
    p.pre_scale = first ? pre : nullptr;
    p.post_scale = (dir && coset) ? dom.coset29_inv : nullptr;
    p.use_post_scalar = (dir && !coset && !inv_fold) ? 1 : 0;
    p.post_scalar = (io && io->has_post_scalar) ? io->post_scalar : dom.n_inv29;
    p.lazy_out = (io && io->lazy_out) ? 1 : 0;
    p.log_len = log_len;
    p.log_c = log_c;
    p.log_n1 = log_n1;
    p.log_n2 = log_n2;
    size_t lds = sizeof(fl) << (log_len + log_c);
    launch_pass("ntt_row_pass", ntt_row_pass<false>, ntt_row_pass<true>, p, small, (size_t)plan.tiles[last], count, lds,
                plan.persistent[last] != 0, stream);
  }
  return 0;  // launch failures are latched by launch() and reported by take_launch_error()
}

// ---- N = 3 * 2^k ------------------------------------------------------------------------------------------------
namespace {
// (r - 1) / 3, little-endian 32-bit words
void exponent_third(uint32_t e[8]) {
  uint32_t t[8];
  for (int i = 0; i < 8; i++) t[i] = FrP::MOD[i];
  t[0] -= 1;  // r is odd and r - 1 is divisible by 3 (r - 1 = 2^28 * 3^2 * ...)
  uint64_t rem = 0;
  for (int i = 7; i >= 0; i--) {
    uint64_t cur = (rem << 32) | t[i];
    e[i] = (uint32_t)(cur / 3);
    rem = cur % 3;
  }
}

// the tables and constants of the five-coset transforms (ntt.hpp: Ntt3Domain::unscale5, Quot5Const); g = 5, wN = omega_N
template <class ToInternal>
int build_quot5(Ntt3Domain* d, const fe& g, const fe& wN, ToInternal to_internal, hipStream_t stream) {
  const size_t M = (size_t)1 << d->log_m, nh = M / 2;
  hipError_t e;
  if ((e = hipMalloc(&d->unscale5, sizeof(fe) * (2 * M + nh))) != hipSuccess) return (int)e;
  const uint32_t en[8] = {(uint32_t)nh, (uint32_t)((uint64_t)nh >> 32), 0, 0, 0, 0, 0, 0};
  fe c[5];  // c_k = s_k^n for k < 3, c_(k+3) = -c_k
  fe s_a = g;
  int rc;
  for (int a = 0; a < 3; a++) {
    c[a] = Fr::pow(s_a, en);
    if ((rc = build_powers(d->unscale5 + (size_t)a * M, a < 2 ? M : nh, Fr::inv(s_a), nullptr, stream))) return rc;
    s_a = Fr::mul(s_a, wN);
  }
  c[3] = Fr::neg(c[0]);
  c[4] = Fr::neg(c[1]);
  // rows E_0, O_0, E_1, O_1, R of the system in (u_0 .. u_4), inverted by Gauss-Jordan elimination
  fe A[5][10];
  for (int r = 0; r < 5; r++)
    for (int j = 0; j < 10; j++) A[r][j] = j == 5 + r ? Fr::one() : Fr::zero();
  for (int a = 0; a < 2; a++) {
    const fe c2 = Fr::sqr(c[a]);
    A[2 * a][0] = Fr::one();
    A[2 * a][2] = c2;
    A[2 * a][4] = Fr::sqr(c2);
    A[2 * a + 1][1] = Fr::one();
    A[2 * a + 1][3] = c2;
  }
  A[4][0] = Fr::one();
  for (int j = 1; j < 5; j++) A[4][j] = Fr::mul(A[4][j - 1], c[2]);
  for (int col = 0; col < 5; col++) {
    int piv = col;
    while (piv < 5 && Fr::is_zero(A[piv][col])) piv++;
    if (piv == 5) return (int)hipErrorInvalidValue;  // the c_k are distinct: cannot happen
    for (int j = 0; j < 10; j++) std::swap(A[piv][j], A[col][j]);
    const fe inv = Fr::inv(A[col][col]);
    for (int j = 0; j < 10; j++) A[col][j] = Fr::mul(A[col][j], inv);
    for (int r = 0; r < 5; r++) {
      if (r == col) continue;
      const fe f = A[r][col];
      for (int j = 0; j < 10; j++) A[r][j] = Fr::sub(A[r][j], Fr::mul(f, A[col][j]));
    }
  }
  Quot5Const& q = d->q5;
  for (int jj = 0; jj < 2; jj++)
    for (int a = 0; a < 2; a++) q.odd[jj][a] = to_internal(A[2 * jj + 1][5 + 2 * a + 1]);
  for (int jj = 0; jj < 3; jj++)
    for (int r = 0; r < 5; r++) q.even[jj][r] = to_internal(A[2 * jj][5 + r]);
  // Mt(Y) = prod_k (Y - c_k)
  fe mt[6];
  mt[0] = Fr::one();
  for (int k = 0; k < 5; k++) {
    mt[k + 1] = mt[k];
    for (int j = k; j >= 1; j--) mt[j] = Fr::sub(mt[j - 1], Fr::mul(mt[j], c[k]));
    mt[0] = Fr::neg(Fr::mul(mt[0], c[k]));
  }
  for (int j = 0; j < 5; j++) {
    q.mt[j] = to_internal(mt[j]);
    q.d[j] = to_internal(Fr::sub(Fr::one(), mt[j]));
  }
  return 0;
}
}  // namespace

int ntt3_build_domain(Ntt3Domain* d, uint32_t log_m, hipStream_t stream) {
  d->log_m = log_m;
  const size_t M = (size_t)1 << log_m, N = 3 * M;
  // omega_N = omega_3 * omega_M^c, 3c = 1 mod M
  uint32_t e3[8];
  exponent_third(e3);
  const fe g = host_from_u64(5);
  const fe w3gen = Fr::pow(g, e3);  // a primitive cube root of unity
  size_t c = (M % 3 == 2) ? (M + 1) / 3 : (2 * M + 1) / 3;
  if (M == 1) c = 1;
  uint32_t ec[8] = {(uint32_t)c, (uint32_t)((uint64_t)c >> 32), 0, 0, 0, 0, 0, 0};
  const fe wM = host_root_of_unity(log_m);
  const fe wN = Fr::mul(w3gen, Fr::pow(wM, ec));
  d->omega = wN;
  uint32_t eM[8] = {(uint32_t)M, (uint32_t)((uint64_t)M >> 32), 0, 0, 0, 0, 0, 0};
  const fe w3 = Fr::pow(wN, eM);
  auto to_internal = [](const fe& a) { return Fr29::pack(Fr29::canonical(Fr29::from_ext(a))); };
  d->w3inv_29 = to_internal(Fr::inv(w3));
  hipError_t e;
  if ((e = hipMalloc(&d->xs_ext, sizeof(fe) * N)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d->xs29, sizeof(fe) * N)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d->pre3, sizeof(fe) * N)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d->tw29_inv, sizeof(fe) * 2 * M)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d->coset_inv_ext, sizeof(fe) * N)) != hipSuccess) return (int)e;
  int rc;
  const fe k32 = host_from_u64(32);
  fe s_a = g;  // 5 * omega_N^a
  for (int a = 0; a < 3; a++) {
    if ((rc = build_powers(d->xs_ext + (size_t)a * M, M, wM, &s_a, stream))) return rc;   // s_a * omega_M^k
    if ((rc = build_powers(d->pre3 + (size_t)a * M, M, s_a, &k32, stream))) return rc;     // 32 * s_a^i
    s_a = Fr::mul(s_a, wN);
  }
  if ((rc = build_powers(d->tw29_inv, 2 * M, Fr::inv(wN), nullptr, stream))) return rc;
  // kappa = 1 / (5^N - 1) (5 generates the whole multiplicative group: 5^N != 1), and kappa / n for n = M / 2
  uint32_t eN[8] = {(uint32_t)N, (uint32_t)((uint64_t)N >> 32), 0, 0, 0, 0, 0, 0};
  d->kappa = Fr::inv(Fr::sub(Fr::pow(g, eN), Fr::one()));
  d->kappa_n_inv29 = to_internal(Fr::mul(Fr::add(d->kappa, d->kappa), Fr::inv(host_from_u64((uint64_t)M))));
  const fe third = Fr::inv(host_from_u64(3));
  if ((rc = build_powers(d->coset_inv_ext, N, Fr::inv(g), &third, stream))) return rc;
  const unsigned blocks = (unsigned)((N + 255) / 256);
  launch("table_to_internal", table_to_internal, dim3(blocks), dim3(256), 0, stream, d->xs29, (const fe*)d->xs_ext, N);
  launch("table_to_internal", table_to_internal, dim3(blocks), dim3(256), 0, stream, d->pre3, (const fe*)d->pre3, N);
  launch("table_to_internal", table_to_internal, dim3((unsigned)((2 * M + 255) / 256)), dim3(256), 0, stream,
         d->tw29_inv, (const fe*)d->tw29_inv, 2 * M);
  if (log_m >= 1 && (rc = build_quot5(d, g, wN, to_internal, stream))) return rc;
  return (int)hipStreamSynchronize(stream);
}

void ntt3_free_domain(Ntt3Domain* d) {
  for (fe** t : {&d->xs_ext, &d->xs29, &d->pre3, &d->tw29_inv, &d->coset_inv_ext, &d->unscale5}) {
    if (*t) hipFree(*t);
    *t = nullptr;
  }
}

int ntt3_forward(const Ntt3Domain& d3, const NttDomain& dom_m, const NttSmallTables& small, fe* data, NttIo io,
                 uint32_t count, fe* scratch, hipStream_t stream) {
  if (dom_m.log_n != d3.log_m) return (int)hipErrorInvalidValue;
  const size_t M = (size_t)1 << d3.log_m;
  if (io.src_len > M) return (int)hipErrorInvalidValue;
  // array 3 q + a: the same polynomial q, pre-scaled by the powers of s_a, transformed, written to block a
  NttIo sub{};
  sub.src = io.src;
  sub.src_outer = io.src_outer;
  sub.src_inner = 0;
  sub.src_group = 3;
  sub.src_group2 = io.src_group ? io.src_group : 1;  // the caller's own grouping moves one level up
  sub.src_inner2 = io.src_inner;
  sub.src_len = io.src_len;
  sub.pre_scale = d3.pre3;
  sub.pre_inner = M;
  sub.lazy_out = 1;
  sub.dst_outer = io.dst_outer;
  sub.dst_inner = M;
  sub.dst_group = 3;
  sub.dst_group2 = io.dst_group ? io.dst_group : 1;
  sub.dst_inner2 = io.dst_inner;
  return ntt_run(dom_m, small, data, scratch, M, count * 3, 0, 0, stream, &sub);
}

int ntt3_inverse(const Ntt3Domain& d3, const NttDomain& dom_m, const NttSmallTables& small, fe* data, uint32_t count,
                 fe* scratch, hipStream_t stream, const fe* add) {
  if (dom_m.log_n != d3.log_m) return (int)hipErrorInvalidValue;
  if (add && d3.log_m == 0) return (int)hipErrorInvalidValue;  // blocks of M / 2
  const size_t M = (size_t)1 << d3.log_m, N = 3 * M;
  fe* y = scratch;
  fe* sub_scratch = scratch + (size_t)count * 3 * M;
  NttIo sub{};
  sub.src = data;
  sub.src_outer = N;
  sub.src_inner = M;  // block a of array q
  sub.src_group = 3;
  sub.src_len = M;
  sub.lazy_out = 1;
  sub.dst_outer = M;
  sub.dst_inner = 0;
  sub.dst_group = 1;
  // inverse sub-transforms of the three blocks (their 1 / M is applied inside), then the radix-3 stage with the
  // coset / 1/3 / form-changing table
  int rc = ntt_run(dom_m, small, y, sub_scratch, M, count * 3, 1, 0, stream, &sub);
  if (rc) return rc;
  launch("ntt3_combine", ntt3_combine, dim3((unsigned)((M + kThreads - 1) / kThreads), count), dim3(kThreads), 0, stream,
         (const fe*)y, data, N, (size_t)0, 1u, M, (const fe*)d3.tw29_inv, d3.w3inv_29, (const fe*)d3.coset_inv_ext, add);
  return 0;  // launch failures are latched by launch() and reported by take_launch_error()
}

// ---- five of the six n-cosets -----------------------------------------------------------------------------------------
int ntt3_forward5(const Ntt3Domain& d3, const NttDomain& dom_m, const NttDomain& dom_h, const NttSmallTables& small,
                  fe* data, NttIo io, uint32_t count, fe* scratch, hipStream_t stream) {
  if (dom_m.log_n != d3.log_m || d3.log_m < 5 || dom_h.log_n + 1 != d3.log_m) return (int)hipErrorInvalidValue;
  const size_t M = (size_t)1 << d3.log_m, nh = M / 2;
  if (io.src_len > M || io.src_len < nh) return (int)hipErrorInvalidValue;
  // arrays 2 q + a, a = 0, 1: polynomial q pre-scaled by the powers of s_a, to block a
  NttIo sub{};
  sub.src = io.src;
  sub.src_outer = io.src_outer;
  sub.src_inner = 0;
  sub.src_group = 2;
  sub.src_group2 = io.src_group ? io.src_group : 1;
  sub.src_inner2 = io.src_inner;
  sub.src_len = io.src_len;
  sub.pre_scale = d3.pre3;
  sub.pre_inner = M;
  sub.lazy_out = 1;
  sub.dst_outer = io.dst_outer;
  sub.dst_inner = M;
  sub.dst_group = 2;
  sub.dst_group2 = io.dst_group ? io.dst_group : 1;
  sub.dst_inner2 = io.dst_inner;
  int rc = ntt_run(dom_m, small, data, scratch, M, count * 2, 0, 0, stream, &sub);
  if (rc) return rc;
  // block 2, even elements: the n-point transform of polynomial q modulo X^n - s_2^n, pre-scaled by the powers of s_2
  NttIo h{};
  h.src = io.src;
  h.src_outer = io.src_outer;
  h.src_inner = io.src_inner;
  h.src_group = io.src_group ? io.src_group : 1;
  h.src_len = io.src_len;
  h.src_fold = io.src_len > nh ? nh : 0;
  h.pre_scale = d3.pre3 + 2 * M;
  h.lazy_out = 1;
  h.dst_outer = io.dst_outer;
  h.dst_inner = io.dst_inner;
  h.dst_group = io.dst_group ? io.dst_group : 1;
  return ntt_run(dom_h, small, data + 2 * M, scratch, nh, count, 0, 0, stream, &h);
}

int ntt3_inverse5(const Ntt3Domain& d3, const NttDomain& dom_m, const NttDomain& dom_h, const NttSmallTables& small,
                  fe* data, uint32_t count, fe* scratch, hipStream_t stream, const fe* top, const fe* add) {
  if (dom_m.log_n != d3.log_m || d3.log_m < 5 || dom_h.log_n + 1 != d3.log_m || !d3.unscale5 || !top)
    return (int)hipErrorInvalidValue;
  const size_t M = (size_t)1 << d3.log_m, N = 3 * M, nh = M / 2;
  fe* y01 = scratch;
  fe* y2 = y01 + (size_t)count * 2 * M;
  fe* sub_scratch = y2 + (size_t)count * nh;
  NttIo sub{};
  sub.src = data;
  sub.src_outer = N;
  sub.src_inner = M;  // block a of array q
  sub.src_group = 2;
  sub.src_len = M;
  sub.lazy_out = 1;
  sub.dst_outer = M;
  sub.dst_inner = 0;
  sub.dst_group = 1;
  int rc = ntt_run(dom_m, small, y01, sub_scratch, M, count * 2, 1, 0, stream, &sub);
  if (rc) return rc;
  NttIo h{};
  h.src = data + 2 * M;
  h.src_outer = N;
  h.src_inner = 0;
  h.src_group = 1;
  h.src_len = nh;
  h.lazy_out = 1;
  h.dst_outer = nh;
  h.dst_inner = 0;
  h.dst_group = 1;
  if ((rc = ntt_run(dom_h, small, y2, sub_scratch, nh, count, 1, 0, stream, &h))) return rc;
  launch("ntt3_combine5", ntt3_combine5, dim3((unsigned)((nh + kThreads - 1) / kThreads), count), dim3(kThreads), 0, stream,
         (const fe*)y01, (const fe*)y2, data, nh, (const fe*)d3.unscale5, d3.q5, top, add);
  return 0;  // launch failures are latched by launch() and reported by take_launch_error()
}

}  // namespace cap
