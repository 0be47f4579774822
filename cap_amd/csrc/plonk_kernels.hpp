// K7-K9 of SURVEY.md §8a: the O(n) element-wise / scan kernels of the TurboPlonk
// prover (permutation grand product, fused quotient evaluation, polynomial
// evaluation, linear combination, division by a linear factor).  Everything here
// is batched over P independent proofs that share one proving key.
//
// Restates on the device the per-round loops of jf-plonk's prover
// (`PlonkKzgSnark::prove`, call site src/proof/transfer.rs:181-186; algorithm as
// recalled in SURVEY.md Appendix A.2-A.6).
#pragma once
#include <hip/hip_runtime.h>

#include "field.hpp"
#include "field29.hpp"
#include "round_elem29.hpp"

namespace cap {
namespace pk {

constexpr int NW = 5;    // wire types
constexpr int NS = 13;   // selectors: q_lc x4, q_mul x2, q_hash x4, q_o, q_c, q_ecc
constexpr int NKX = NW - 1;           // columns k_j x, j = 1 .. 4, of the quotient domain (k_kx_columns)
constexpr int kPkcCols = NS + NW + NKX;  // columns of a key's coset table: 13 selectors, 5 sigmas, 4 x k_j x
constexpr int kThreads = 256;
constexpr int kScanPerThread = 4;
constexpr int kScanBlock = kThreads * kScanPerThread;  // 1024 elements per workgroup

// per-proof challenges, device layout
// beta_inv = 1 / beta (0 for beta = 0) and alpha_beta5 = alpha beta^5: k_quotient's permutation terms with beta folded out
struct Chal {
  fe beta, gamma, alpha, alpha2, beta_inv, alpha_beta5;
};

struct QuotConst {
  fe g;           // coset generator 5 (Montgomery)
  fe k[NW];       // wire-subset separators
  fe zh_inv[8];   // 1 / ((g * w_m^i)^n - 1), i mod 6 (m = 6n: six distinct values)
};

// dst[(q/inner)*dst_outer + (q%inner)*dst_inner + k] = k < len ? src[(q/inner)*src_outer + (q%inner)*src_inner + k] : 0
__global__ __launch_bounds__(kThreads) void k_pad_copy(fe* __restrict__ dst, size_t dst_outer, size_t dst_inner,
                                                       const fe* __restrict__ src, size_t src_outer, size_t src_inner,
                                                       uint32_t inner, size_t len, size_t total) {
  size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  uint32_t q = blockIdx.y;
  size_t d = (size_t)(q / inner) * dst_outer + (size_t)(q % inner) * dst_inner + k;
  fe v = Fr::zero();
  if (k < len) v = src[(size_t)(q / inner) * src_outer + (size_t)(q % inner) * src_inner + k];
  dst[d] = v;
}

// poly_q += (b_0 + b_1 X + ...)(X^n - 1); blinder index = (q/inner)*13 + bl_off + (q%inner)*nb + t.
// SET_TAIL: the coefficients n .. n + 7 hold nothing yet (the interpolation wrote n of the n + 8 slots): they are set -
// blinders, then zeros - instead of added to.
template <int SET_TAIL>
__global__ void k_blind(fe* __restrict__ polys, size_t stride, size_t n, const fe* __restrict__ blinders,
                        uint32_t inner, uint32_t bl_off, uint32_t nb, uint32_t count) {
  uint32_t t = threadIdx.x, q = blockIdx.x;
  if (q >= count) return;
  fe* p = polys + (size_t)q * stride;
  if (t >= nb) {
    if (SET_TAIL && t < 8 && n + t < stride) p[n + t] = Fr::zero();
    return;
  }
  fe b = blinders[(size_t)(q / inner) * 13 + bl_off + (size_t)(q % inner) * nb + t];
  p[t] = Fr::sub(p[t], b);
  p[n + t] = SET_TAIL ? b : Fr::add(p[n + t], b);
}

// commitments from evaluations (lagrange.hip): the MSM scalars of column q are its n values followed by its nb blinders -
// commit(w + (b0 + b1 X [+ b2 X^2])(X^n - 1)) = sum_j w_j [L_j] + sum_e b_e [tau^(n+e) - tau^e].  Column q's values start at
// evals + q * src_stride; its blinders at blinders[(q / inner) * 13 + bl_off + (q % inner) * nb ..] (k_blind's layout).
__global__ __launch_bounds__(kThreads) void k_stage_evals(const fe* __restrict__ evals, size_t src_stride, size_t n,
                                                          const fe* __restrict__ blinders, uint32_t inner,
                                                          uint32_t bl_off, uint32_t nb,
                                                          fe* __restrict__ dst /*[count][n + nb]*/) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t q = blockIdx.y;
  if (j >= n + nb) return;
  dst[(size_t)q * (n + nb) + j] =
      j < n ? evals[(size_t)q * src_stride + j]
            : blinders[(size_t)(q / inner) * 13 + bl_off + (size_t)(q % inner) * nb + (j - n)];
}

// round 2: per-row numerator / denominator of the permutation grand product
//   num_j = prod_i (w_i + beta k_i omega^j + gamma),   den_j = prod_i (w_i + beta sigma_i(omega^j) + gamma)
// On the lazy field.  All inputs are in arkworks' form (x * 2^256); a lazy product of two such values is x y 2^256 / 2^5,
// so the scalars that multiply data - beta and the k_i (qc29) - are taken in the internal form (x * 2^261: their products
// with arkworks-form data stay in arkworks' form), and the four products of each chain, which lose 2^5 apiece, are
// put right by one multiplication with 2^20 (internal form).  21 lazy multiplications of ~210 instructions instead of 18
// saturated ones of ~400.
// sig_of (optional): the sigma evaluations of proof p's own key - a batch may mix proofs of several keys on one domain
__global__ __launch_bounds__(kThreads) void k_perm_numden(const fe* __restrict__ wires /*[P][5][n]*/,
                                                          const fe* __restrict__ sig_eval /*[5][n]*/,
                                                          const fe* const* __restrict__ sig_of,
                                                          const fe* __restrict__ tw_n, const Chal* __restrict__ chal,
                                                          QuotConst qc29, size_t n, fe* __restrict__ num,
                                                          fe* __restrict__ den) {
  using F = Fr29;
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  uint32_t p = blockIdx.y;
  if (sig_of) sig_eval = sig_of[p];
  // the row's arithmetic: round_elem29.hpp
  perm_numden_row<F, fl, fe>(
      chal[p].beta, chal[p].gamma, tw_n[j], qc29.k,
      [&](int i) -> const fe& { return wires[((size_t)p * NW + i) * n + j]; },
      [&](int i) -> const fe& { return sig_eval[(size_t)i * n + j]; }, num[(size_t)p * n + j], den[(size_t)p * n + j]);
}

// ---- exclusive scans over [batch][len] arrays (stride elements apart) --------------------------------
// OP 0: field multiplication, 1: field addition.  REV: suffix scan (logical index len-1-k).
template <int OP>
__device__ __forceinline__ fe scan_op(const fe& a, const fe& b) {
  return OP == 0 ? Fr::mul(a, b) : Fr::add(a, b);
}
template <int OP>
__device__ __forceinline__ fe scan_identity() {
  return OP == 0 ? Fr::one() : Fr::zero();
}
__device__ __forceinline__ fe shfl_up_fe(const fe& a, int d) {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = __shfl_up(a.v[i], d);
  return r;
}

// phase 1: block-local exclusive scan; block totals to tot[batch][nblocks]
template <int OP, int REV>
__global__ __launch_bounds__(kThreads) void k_scan_local(const fe* __restrict__ in, fe* __restrict__ out, size_t len,
                                                         size_t stride, fe* __restrict__ tot, uint32_t nblocks) {
  __shared__ fe wave_tot[kThreads / 64];
  const uint32_t b = blockIdx.y, blk = blockIdx.x;
  const fe* src = in + (size_t)b * stride;
  fe* dst = out + (size_t)b * stride;
  size_t k0 = (size_t)blk * kScanBlock + (size_t)threadIdx.x * kScanPerThread;
  fe v[kScanPerThread];
  fe run = scan_identity<OP>();
#pragma unroll
  for (int t = 0; t < kScanPerThread; t++) {
    size_t k = k0 + t;
    fe x = scan_identity<OP>();
    if (k < len) x = src[REV ? (len - 1 - k) : k];
    v[t] = run;                 // exclusive within the thread
    run = t == 0 ? x : scan_op<OP>(run, x);
  }
  // inclusive scan of thread totals across the wavefront
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  fe inc = run;
  for (int d = 1; d < 64; d <<= 1) {
    fe o = shfl_up_fe(inc, d);
    if ((int)lane >= d) inc = scan_op<OP>(o, inc);
  }
  if (lane == 63) wave_tot[wave] = inc;
  fe excl = shfl_up_fe(inc, 1);
  if (lane == 0) excl = scan_identity<OP>();
  __syncthreads();
  fe wpre = scan_identity<OP>();
  for (uint32_t w = 0; w < wave; w++) wpre = scan_op<OP>(wpre, wave_tot[w]);
  fe base = scan_op<OP>(wpre, excl);
#pragma unroll
  for (int t = 0; t < kScanPerThread; t++) {
    size_t k = k0 + t;
    if (k < len) dst[REV ? (len - 1 - k) : k] = t == 0 ? base : scan_op<OP>(base, v[t]);
  }
  if (threadIdx.x == kThreads - 1) tot[(size_t)b * nblocks + blk] = scan_op<OP>(wpre, inc);
}

// phase 2: exclusive scan of the block totals (one wavefront per batch entry, 64 blocks per step)
template <int OP>
__global__ __launch_bounds__(64) void k_scan_totals(fe* __restrict__ tot, uint32_t nblocks) {
  fe* t = tot + (size_t)blockIdx.x * nblocks;
  const uint32_t lane = threadIdx.x;
  fe carry = scan_identity<OP>();
  for (uint32_t base = 0; base < nblocks; base += 64) {
    uint32_t i = base + lane;
    fe x = i < nblocks ? t[i] : scan_identity<OP>();
    fe inc = x;
    for (int d = 1; d < 64; d <<= 1) {
      fe o = shfl_up_fe(inc, d);
      if ((int)lane >= d) inc = scan_op<OP>(o, inc);
    }
    fe excl = shfl_up_fe(inc, 1);
    if (lane == 0) excl = scan_identity<OP>();
    if (i < nblocks) t[i] = scan_op<OP>(carry, excl);
    fe last;
#pragma unroll
    for (int w = 0; w < 8; w++) last.v[w] = __shfl(inc.v[w], 63);
    carry = scan_op<OP>(carry, last);
  }
}

// phase 3: fold the block prefix in
template <int OP, int REV>
__global__ __launch_bounds__(kThreads) void k_scan_apply(fe* __restrict__ out, size_t len, size_t stride,
                                                         const fe* __restrict__ tot, uint32_t nblocks) {
  const uint32_t b = blockIdx.y, blk = blockIdx.x;
  if (blk == 0) return;
  fe pre = tot[(size_t)b * nblocks + blk];
  fe* dst = out + (size_t)b * stride;
  for (int t = 0; t < kScanPerThread; t++) {
    size_t k = (size_t)blk * kScanBlock + (size_t)t * kThreads + threadIdx.x;
    if (k < len) {
      size_t idx = REV ? (len - 1 - k) : k;
      dst[idx] = scan_op<OP>(pre, dst[idx]);
    }
  }
}

// total[p] = sfx[p][0] * den[p][0], the product of all denominators of proof p: the host inverts it (one batched
// inversion for the whole batch, microseconds) where a lone device thread spent 0.17 ms on a 254-squaring chain
__global__ void k_perm_total(const fe* __restrict__ sfx, const fe* __restrict__ den, size_t n, fe* __restrict__ total,
                             uint32_t count) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  total[p] = Fr::mul(sfx[(size_t)p * n], den[(size_t)p * n]);
}

// inv_total[p] = 1 / (sfx[p][0] * den[p][0])   (device form, CAPGPU_PERM_INV_ON_DEVICE=1)
__global__ void k_perm_inv_total(const fe* __restrict__ sfx, const fe* __restrict__ den, size_t n,
                                 fe* __restrict__ inv_total, uint32_t count) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  // one thread per proof and nothing else on the device: the lazy field's windowed inversion in its row-wise
  // (latency) schedule - 0.31 -> 0.1 ms on the path of a single proof
  using F = Fl<FrP29, 0>;
  inv_total[p] = F::to_ext(F::inv(F::mul(F::from_ext(sfx[(size_t)p * n]), F::from_ext(den[(size_t)p * n]))));
}

// z[j] = prefix_num[j] * (suffix_den_excl[j] * den[j]) / prod(den); zero padding up to stride
__global__ __launch_bounds__(kThreads) void k_perm_finish(const fe* __restrict__ pre, const fe* __restrict__ sfx,
                                                          const fe* __restrict__ den,
                                                          const fe* __restrict__ inv_total, size_t n,
                                                          fe* __restrict__ z, size_t zstride) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t p = blockIdx.y;
  if (j >= zstride) return;
  fe v = Fr::zero();
  if (j < n) {
    size_t o = (size_t)p * n + j;
    v = Fr::mul(Fr::mul(pre[o], sfx[o]), Fr::mul(den[o], inv_total[p]));
  }
  z[(size_t)p * zstride + j] = v;
}

// ---- round 3: fused quotient evaluation on the coset of size m = 6n ----------------------------------
// (jf-plonk uses 8n; the quotient has degree < 5n + 8, so 6n = 3 * 2^(log n + 1) points determine it - ntt.hpp)
// All inputs are in the internal Montgomery form of the lazy 29-bit field (x * 2^261): the forward coset NTTs emit
// it (ntt3_forward) and the inverse coset NTT that follows consumes it (ntt3_inverse).
// pkc: [22][m] coset evaluations of 13 selectors then 5 sigmas, then k_j x_i for j = 1 .. 4 (shared by all proofs)
// cos: [P][6][m] coset evaluations of 5 wires, z;   tw_m: omega_m^i;   inv_nx1: 1 / (n (x_i - 1))
// The public-input term of the numerator is NOT evaluated here: PI(x) / Z_H(x) is added to the result as coefficients
// by the inverse transform that follows (ntt.hpp: Ntt3Domain::kappa; prove_run.hpp: pi_fold).
// Sums of products share one Montgomery reduction (at most 6 products per 64-bit column accumulator): ColAcc,
// round_elem29.hpp, where the per-point arithmetic of the kernels below lives.

// columns 18 .. 21 of a key's coset table: dst[j][i] = k_(j+1) x_i, internal form, canonical.  A function of the key's
// separators and the domain only: built once per key (per launch of k_quotient under the reference schedule).
__global__ __launch_bounds__(kThreads) void k_kx_columns(fe* __restrict__ dst, const fe* __restrict__ xs, QuotConst qc,
                                                         size_t m) {
  using F = Fr29;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const fl x = F::load(xs[i]);
#pragma unroll
  for (int j = 0; j < NKX; j++) dst[(size_t)j * m + i] = kx_elem<F, fl, fe>(qc.k[j + 1], x);
}

// pkc_of (optional): the key columns of proof p's own key (mixed-key batches), otherwise pkc for all
// FOLD: the permutation terms with beta folded out (below).  That form needs 1 / beta: a proof with beta = 0 (beta_inv = 0)
// is left to the direct form, k_quotient<false>, launched behind it with only_unfoldable = 1 - there every other proof
// leaves at once.  p is blockIdx.x, so either exit is taken by whole workgroups.  (One kernel with both forms behind a
// uniform branch takes 256 VGPRs + 71 AGPRs - one wave per SIMD; each form alone stays at two: 252 and 228 VGPRs.)
// k_quotient<false> with only_unfoldable = 0 is the direct form for every proof (CAPGPU_QUOT_FOLD=0).
__device__ __forceinline__ bool fe_nonzero(const fe& a) {
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) o |= a.v[k];
  return o != 0;
}
template <bool FOLD>
__global__ __launch_bounds__(kThreads) void k_quotient(const fe* __restrict__ pkc, const fe* const* __restrict__ pkc_of,
                                                       const fe* __restrict__ cos, const fe* __restrict__ xs,
                                                       const fe* __restrict__ inv_nx1,
                                                       const Chal* __restrict__ chal, QuotConst qc, size_t m,
                                                       uint32_t only_unfoldable, uint32_t five,
                                                       fe* __restrict__ t_out) {
  using F = Fr29;
  // grid (proofs, tiles): the proofs of one tile run together, so the 18 shared selector / sigma tiles are read from
  // HBM once per tile and served from L2 to the other proofs of the batch
  // five: the points are blocks 0 and 1 and the even elements of block 2, kept compactly - [M][M][M / 2] inside the same
  // strides (ntt.hpp: ntt3_forward5); the tables of the whole domain are read at `it`, the point's index there
  size_t i = (size_t)blockIdx.y * blockDim.x + threadIdx.x;
  if (i >= (five ? m - m / 6 : m)) return;
  const uint32_t p = blockIdx.x;
  if (FOLD ? !fe_nonzero(chal[p].beta_inv) : (only_unfoldable && fe_nonzero(chal[p].beta_inv))) return;
  if (pkc_of) pkc = pkc_of[p];
  const uint32_t mm = (uint32_t)(m / 3);                                  // block length M (uniform: scalar unit)
  const uint32_t blk = (i >= mm ? 1u : 0u) + (i >= 2 * (size_t)mm ? 1u : 0u);  // which of the three cosets
  const fe* c = cos + (size_t)p * 6 * m;
  const bool half = five && blk == 2;
  const size_t it = half ? 2 * i - 2 * (size_t)mm : i;
  struct Point {  // what the body reads once, each where it needs it
    const fe* c;
    const fe *__restrict__ xs, *__restrict__ inv_nx1;
    size_t m, i, it;
    uint32_t blk, mm;
    bool half;
    // index a M + k (ntt.hpp): x * omega_n = x * omega_M^2 is two steps further inside the same block of M = m / 3
    __device__ __forceinline__ const fe& z_next() const {
      const uint32_t k1 = (uint32_t)i - blk * mm;
      const size_t inext = (size_t)blk * mm + (half ? (k1 + 1) & (mm / 2 - 1) : (k1 + 2) & (mm - 1));
      return c[5 * m + inext];
    }
    __device__ __forceinline__ const fe& x() const { return xs[it]; }  // the point itself: s_a * omega_M^k at index a * M + k
    __device__ __forceinline__ const fe& inv() const { return inv_nx1[it]; }
    // x^n depends on the block and on the parity of k only: (s_a omega_M^k)^n = s_a^n (-1)^k = (5 omega_N^(3k + a))^n
    __device__ __forceinline__ const fe& zh_inv(const QuotConst& q) const {
      const uint32_t zi = 3 * (half ? 0u : ((uint32_t)i - blk * mm) & 1) + blk;  // < 6
      return q.zh_inv[zi];
    }
  };
  const Point at{c, xs, inv_nx1, m, i, it, blk, mm, half};
  // the point's arithmetic: round_elem29.hpp
  t_out[(size_t)p * m + i] = quotient_point<FOLD, F, fl, fe>(
      [&](int s) -> const fe& { return pkc[(size_t)s * m + it]; },
      [&](int j) -> const fe& { return c[(size_t)j * m + i]; }, at, chal[p], qc);
}

// out[i] = 1 / (n * (x_i - 1))   (one-time table of the proving key; xs = the points of the quotient domain)
__global__ __launch_bounds__(kThreads) void k_inv_nx1(fe* __restrict__ out, const fe* __restrict__ xs, fe n_mont,
                                                      size_t m) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  out[i] = Fr::inv(Fr::mul(n_mont, Fr::sub(xs[i], Fr::one())));
}

// flags[p] |= 1 if any coefficient at index >= lo is non-zero; |= 2 if coefficient lo-1 is zero
__global__ __launch_bounds__(kThreads) void k_check_degree(const fe* __restrict__ t, size_t m, size_t lo,
                                                           uint32_t* __restrict__ flags) {
  size_t k = lo - 1 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  uint32_t p = blockIdx.y;
  bool zero = Fr::is_zero(t[(size_t)p * m + k]);
  if (k == lo - 1) {
    if (zero) atomicOr(&flags[p], 2u);
  } else if (!zero) {
    atomicOr(&flags[p], 1u);
  }
}

// ---- five-coset quotient: the top 8 coefficients h = t[5n .. 5n + 8) from the polynomials in hand --------------------
// t (X^n - 1) = N and t has nothing at or above degree 6n, so h_i = N_(6n+i).  Only two parts of the numerator reach that
// degree (n >= 16):  alpha [ z prod_j (w_j + beta k_j X + gamma) - z(omega X) prod_j (w_j + beta sigma_j + gamma) ], of
// degree 6n + 7, and sum_i q_hash_i w_i^5 + q_ecc w_0 w_1 w_2 w_3 w_4, of degree 6n + 4.  Each factor enters through its
// top coefficients, written as a series from the top down - w_j: n + 1 - k, z: n + 2 - k, sigma_j and the selectors:
// n - 1 - k - and the products are products of series truncated at 8 terms.  beta k_j X and gamma do not reach.
// One workgroup of 64 lanes per proof: a series product is 36 field products, one per lane, and a sum per term.
// Saturated field, arkworks' form in and out.
__device__ __noinline__ void series_mul8(fe* dst, const fe* x, const fe* y, fe* prod) {
  const uint32_t t = threadIdx.x, a = t >> 3, b = t & 7;
  __syncthreads();  // the operands are written, prod is free
  if (a + b < 8) prod[t] = Fr::mul(x[a], y[b]);
  __syncthreads();
  fe s = Fr::zero();
  if (t < 8) {
    s = prod[t];
    for (uint32_t k = 1; k <= t; k++) s = Fr::add(s, prod[k * 8 + t - k]);
  }
  __syncthreads();  // (dst may be one of the operands)
  if (t < 8) dst[t] = s;
  __syncthreads();
}
// coef: the key's 18 polynomials [18][ps] (coef_of: proof p's own key), tw_n: omega_n^e, top: [P][8]
__global__ __launch_bounds__(64) void k_quotient_top(const fe* __restrict__ wpoly /*[P][5][ps]*/,
                                                     const fe* __restrict__ zpoly /*[P][ps]*/,
                                                     const fe* __restrict__ coef, const fe* const* __restrict__ coef_of,
                                                     const fe* __restrict__ tw_n, const Chal* __restrict__ chal, size_t n,
                                                     size_t ps, fe* __restrict__ top) {
  __shared__ fe W[NW][8], B[NW][8], sa[8], sb[8], sc[8], prod[64];
  const uint32_t p = blockIdx.x, t = threadIdx.x;
  if (coef_of) coef = coef_of[p];
  const fe* wp = wpoly + (size_t)p * NW * ps;
  const fe* zp = zpoly + (size_t)p * ps;
  if (t < NW * 8) {
    const uint32_t j = t >> 3, k = t & 7;
    const fe w = wp[(size_t)j * ps + n + 1 - k];
    W[j][k] = w;
    B[j][k] = k >= 2 ? Fr::add(w, Fr::mul(chal[p].beta, coef[(size_t)(NS + j) * ps + n + 1 - k])) : w;
  }
  fe h = Fr::zero();  // lane t < 8: h_t
  // gate terms: series index k <-> degree 6n + 4 - k <-> h_(4-k)
  auto take_gate = [&](const fe* s) {
    if (t < 5) h = Fr::add(h, s[4 - t]);
  };
  for (int i = 0; i < 4; i++) {  // q_hash_i w_i^5
    series_mul8(sa, W[i], W[i], prod);
    series_mul8(sa, sa, sa, prod);
    series_mul8(sa, sa, W[i], prod);
    if (t < 8) sb[t] = coef[(size_t)(6 + i) * ps + n - 1 - t];
    series_mul8(sc, sa, sb, prod);
    take_gate(sc);
  }
  series_mul8(sa, W[0], W[1], prod);
  for (int j = 2; j < NW; j++) series_mul8(sa, sa, W[j], prod);  // sa = prod_j w_j
  if (t < 8) sb[t] = coef[(size_t)12 * ps + n - 1 - t];          // q_ecc
  series_mul8(sc, sa, sb, prod);
  take_gate(sc);
  // permutation terms: series index k <-> degree 6n + 7 - k <-> h_(7-k)
  if (t < 8) sb[t] = zp[n + 2 - t];
  series_mul8(sc, sa, sb, prod);
  fe perm = Fr::zero();
  if (t < 8) perm = sc[7 - t];
  series_mul8(sa, B[0], B[1], prod);
  for (int j = 2; j < NW; j++) series_mul8(sa, sa, B[j], prod);
  if (t < 8) {  // z(omega X): coefficient c times omega^c (omega^n = 1)
    const size_t c = n + 2 - t;
    sb[t] = Fr::mul(zp[c], tw_n[c >= n ? c - n : c]);
  }
  series_mul8(sc, sa, sb, prod);
  if (t < 8) {
    perm = Fr::sub(perm, sc[7 - t]);
    top[(size_t)p * 8 + t] = Fr::add(h, Fr::mul(chal[p].alpha, perm));
  }
}

// ---- round 4/5 helpers ---------------------------------------------------------------------------------
// tables[q][k] = base_q^k, k < len;  pw[q][b] = base_q^(2^b), b < 24.  Two steps: a small table per base with
// base^i (i < 256) followed by base^(256 j), each entry by the binary method, then one multiplication per output.
constexpr uint32_t kPowLow = 256;
__global__ __launch_bounds__(kThreads) void k_powers_small(fe* __restrict__ small, uint32_t small_len,
                                                           const fe* __restrict__ pw) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= small_len) return;
  uint32_t q = blockIdx.y;
  const fe* b = pw + (size_t)q * 24;
  const uint32_t e = i < kPowLow ? i : (i - kPowLow) * kPowLow;
  fe r = Fr::one();
  bool started = false;
  for (int k = 0; (e >> k) != 0; k++) {
    if ((e >> k) & 1) {
      r = started ? Fr::mul(r, b[k]) : b[k];
      started = true;
    }
  }
  small[(size_t)q * small_len + i] = r;
}
__global__ __launch_bounds__(kThreads) void k_powers(fe* __restrict__ tables, size_t stride, size_t len,
                                                     const fe* __restrict__ small, uint32_t small_len) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= len) return;
  uint32_t q = blockIdx.y;
  const fe* t = small + (size_t)q * small_len;
  // blockDim.x == kPowLow: the high factor is the same for the whole workgroup
  tables[(size_t)q * stride + e] = Fr::mul(t[e & (kPowLow - 1)], t[kPowLow + (e >> 8)]);
}

struct EvalDesc {
  const fe* poly;
  const fe* pows;
  uint32_t len;
  uint32_t pad;
};

__device__ __forceinline__ fe wave_sum(fe v) {
  for (int d = 32; d >= 1; d >>= 1) {
    fe o;
#pragma unroll
    for (int i = 0; i < 8; i++) o.v[i] = __shfl_down(v.v[i], d);
    v = Fr::add(v, o);
  }
  return v;
}

// partial[e][chunk] = sum over the chunk of poly[k] * pows[k]
__global__ __launch_bounds__(kThreads) void k_eval_partial(const EvalDesc* __restrict__ desc, fe* __restrict__ partial,
                                                           uint32_t chunks, uint32_t per_chunk) {
  __shared__ fe sh[kThreads / 64];
  const uint32_t e = blockIdx.y, chunk = blockIdx.x;
  const EvalDesc d = desc[e];
  fe acc = Fr::zero();
  uint32_t lo = chunk * per_chunk, hi = lo + per_chunk;
  if (hi > d.len) hi = d.len;
  for (uint32_t k = lo + threadIdx.x; k < hi; k += kThreads) acc = Fr::add(acc, Fr::mul(d.poly[k], d.pows[k]));
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    fe r = sh[0];
    for (int w = 1; w < kThreads / 64; w++) r = Fr::add(r, sh[w]);
    partial[(size_t)e * chunks + chunk] = r;
  }
}
__global__ __launch_bounds__(64) void k_eval_final(const fe* __restrict__ partial, uint32_t chunks,
                                                   fe* __restrict__ out) {
  const uint32_t e = blockIdx.x;
  fe acc = Fr::zero();
  for (uint32_t k = threadIdx.x; k < chunks; k += 64) acc = Fr::add(acc, partial[(size_t)e * chunks + k]);
  acc = wave_sum(acc);
  if (threadIdx.x == 0) out[e] = acc;
}

struct LinTerm {
  const fe* poly;
  fe scalar;
  uint32_t len;
  uint32_t pad[3];
};

// out[p][k] = sum_t terms[p][t].scalar * terms[p][t].poly[k]   (k < terms[p][t].len), k < out_len
// Scalars arrive in the internal form of the lazy field (x * 2^261), polynomials in arkworks' form, so every product
// is back in arkworks' form; six products share one Montgomery reduction.
__global__ __launch_bounds__(kThreads) void k_lincomb(const LinTerm* __restrict__ terms, uint32_t nterms,
                                                      fe* __restrict__ out, size_t out_stride, size_t out_len) {
  using F = Fr29;
  size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= out_len) return;
  uint32_t p = blockIdx.y;
  const LinTerm* T = terms + (size_t)p * nterms;
  struct Terms {
    const LinTerm* T;
    uint32_t nterms;
    size_t k;
    __device__ __forceinline__ bool active(uint32_t t) const { return t < nterms && k < T[t].len; }
    __device__ __forceinline__ const fe& scalar(uint32_t t) const { return T[t].scalar; }
    __device__ __forceinline__ const fe& value(uint32_t t) const { return T[t].poly[k]; }
  };
  out[(size_t)p * out_stride + k] = lincomb_elem<F, fl, fe>(nterms, Terms{T, nterms, k});
}

// h[q][k] = f[q][k] * pows[tab(q)][k];  tab(q) = (q/2)*4 + (q%2)      (q = proof*2 + {zeta, zeta*omega})
__global__ __launch_bounds__(kThreads) void k_div_prepare(const fe* __restrict__ f, const fe* __restrict__ pows,
                                                          size_t stride, size_t len, fe* __restrict__ h) {
  size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= len) return;
  uint32_t q = blockIdx.y;
  size_t tab = (size_t)(q / 2) * 4 + (q % 2);
  h[(size_t)q * stride + k] = Fr::mul(f[(size_t)q * stride + k], pows[tab * stride + k]);
}
// quot[q][i] = sfx[q][i] * ainv^(i+1), i < len-1 (sfx = exclusive suffix sum of h); quot[q][len-1..stride) = 0
__global__ __launch_bounds__(kThreads) void k_div_finish(const fe* __restrict__ sfx, const fe* __restrict__ pows,
                                                         size_t stride, size_t len, fe* __restrict__ quot) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= stride) return;
  uint32_t q = blockIdx.y;
  size_t tab = (size_t)(q / 2) * 4 + 2 + (q % 2);
  fe v = Fr::zero();
  if (i + 1 < len) v = Fr::mul(sfx[(size_t)q * stride + i], pows[tab * stride + i + 1]);
  quot[(size_t)q * stride + i] = v;
}

}  // namespace pk
}  // namespace cap
