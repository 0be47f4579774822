// Radix-2 NTT / iNTT over BN254 Fr for gfx950 (K2 of SURVEY.md §8a).
//
// Replaces ark-poly 0.3.0 `Radix2EvaluationDomain::{fft,ifft,coset_fft,
// coset_ifft}_in_place` (Cargo.lock:194-196) reached from
// src/proof/transfer.rs:181-186 (PlonkKzgSnark::prove).  Semantics kept:
// natural order in / out, omega_n = omega_28^(2^(28-log n)), coset generator 5,
// inverse includes n^-1, coset inverse scales by 5^-i afterwards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"

namespace cap {

// Per-domain-size device tables (built once per log_n, kept resident).
struct NttDomain {
  uint32_t log_n = 0;
  fe* tw_fwd = nullptr;     // omega_n^e,  e in [0, n)
  fe* tw_inv = nullptr;     // omega_n^-e, e in [0, n)
  fe* coset_fwd = nullptr;  // 5^i,           i in [0, n)
  fe* coset_inv = nullptr;  // n^-1 * 5^-i,   i in [0, n)
  fe n_inv;                 // n^-1 (Montgomery)
  // the same tables in the internal Montgomery form of the lazy 29-bit field (x * 2^261, canonical): what the
  // NTT kernels multiply by.  (tw_fwd above stays in arkworks' form for the kernels that have not moved yet.)
  fe* tw29_fwd = nullptr;
  fe* tw29_inv = nullptr;
  fe* tw29_inv_n = nullptr;  // omega_n^-e / n: inter-pass twiddles of the plain inverse transforms (null: -DCAP_NTT_NO_INV_FOLD)
  fe* coset29_fwd = nullptr;
  fe* coset29_inv = nullptr;
  fe n_inv29;
};

// Small-size twiddles shared by every domain (internal form): fwd[s] -> omega_{2^s}^i, i < 2^(s-1), s <= kMaxLogTile
constexpr int kMaxLogTile = 11;
struct NttSmallTables {
  fe* fwd[kMaxLogTile + 1] = {nullptr};
  fe* inv[kMaxLogTile + 1] = {nullptr};
  // the same values unpacked to the 9 x 29-bit limbs the butterflies multiply by (36 B per entry): saves the
  // 8 -> 9 word unpacking in every butterfly
  uint32_t* fwd_u[kMaxLogTile + 1] = {nullptr};
  uint32_t* inv_u[kMaxLogTile + 1] = {nullptr};
  // tile counters of persistent pass launches (ntt.hip: a launch of many tiles is a few workgroups per CU that take tile
  // after tile from a counter); one slot per launch, reused in rotation on the context's one stream
  uint32_t* pass_counters = nullptr;
  mutable uint32_t next_counter = 0;
};
constexpr uint32_t kNttPassCounters = 256;

// Host-side table construction (runs tiny setup kernels).  Returns hipError_t as int.
int ntt_build_small_tables(NttSmallTables* t, hipStream_t stream);
int ntt_build_domain(NttDomain* d, uint32_t log_n, hipStream_t stream);
void ntt_free_domain(NttDomain* d);
void ntt_free_small_tables(NttSmallTables* t);

// omega_{2^log_n} in Montgomery form (host)
fe ntt_root_of_unity(uint32_t log_n);

// In-place (from the caller's view) batched transform of `count` arrays of 2^log_n
// elements, array b at data + b * stride_elems.  `scratch` must hold count * 2^log_n
// elements.  dir: 0 forward, 1 inverse.  coset: 0/1.
// Optional out-of-place addressing: the transform reads array q of the batch from
// src + (q / src_group) * src_outer + (q % src_group) * src_inner, treating elements at or beyond src_len as zero (a
// polynomial shorter than the domain needs no zero-padded copy), and writes it to
// data + (q / dst_group) * dst_outer + (q % dst_group) * dst_inner.  `scratch` then holds count * 2^log_n elements.
struct NttIo {
  const fe* src;
  size_t src_outer, src_inner, src_len;
  uint32_t src_group;
  size_t dst_outer, dst_inner;
  uint32_t dst_group;
  // decimated input (the 3 * 2^k transforms below): element g of array q is src[...][g * src_elem_stride]; src_len
  // and the pre-scale table are indexed by that source position plus (q % src_group) * src_inner
  uint32_t src_elem_stride = 1;
  uint32_t src_group2 = 1;        // second grouping level above src_group (see PassParams::in_group2)
  size_t src_inner2 = 0;
  uint32_t dst_group2 = 1;        // the same for the output
  size_t dst_inner2 = 0;
  size_t pre_inner = 0;           // pre-scale table of array q: pre_scale + (q % src_group) * pre_inner
  const fe* pre_scale = nullptr;  // overrides the coset table of the domain (internal form)
  int lazy_out = 0;               // leave results weakly reduced (< 2r) instead of canonical
  // plain inverse transforms (dir 1, coset 0) only: multiply every output by this scalar (internal form) in place of the
  // domain's n^-1 - a constant factor of the result rides on the multiplication the transform performs anyway
  int has_post_scalar = 0;
  fe post_scalar = {};
  // folded input (first pass, contiguous input only): element g of the transform is src[g] * pre[g] +
  // src[g + src_fold] * pre[g + src_fold], the second term only where g + src_fold < src_len - a polynomial a few
  // coefficients longer than the transform, reduced modulo X^n - s^n on the way in (0: no fold)
  size_t src_fold = 0;
};
int ntt_run(const NttDomain& dom, const NttSmallTables& small, fe* data, fe* scratch, size_t stride_elems,
            uint32_t count, int dir, int coset, hipStream_t stream, const NttIo* io = nullptr);

// How ntt_run transforms `count` arrays of 2^log_n elements: the one place that decides it (host only, no device
// needed; CAPGPU_NTT_TILE_LOG, CAPGPU_NTT_TILE_ADAPT and CAPGPU_NTT_PERSISTENT are read once per process).  Passes are
// listed in the order they run: passes - 1 column passes, then the row pass.  passes == 0: log_n == 0 or count == 0,
// nothing is launched.
struct NttPlan {
  uint32_t passes = 0;
  uint32_t tile_log = 0;              // log2 of the LDS tile the launch aims for (tile_log_for)
  uint32_t digits[3] = {0, 0, 0};     // log2 of the sub-transform size of each pass
  uint32_t log_c[3] = {0, 0, 0};      // log2 of the tile width of each pass: a tile is 2^(digit + log_c) elements
  uint64_t tiles[3] = {0, 0, 0};      // tiles per array of each pass
  uint32_t persistent[3] = {0, 0, 0}; // 1: the pass is launched as a few workgroups per CU that take tiles from a counter
};
int ntt_plan(uint32_t log_n, uint32_t count, NttPlan* out);  // 0, or hipErrorInvalidValue for a size that has no plan

// ---- evaluation on N = 3 * 2^k points ------------------------------------------------------------------------
// The quotient polynomial of the prover has degree < 5n + 8, so 6n = 3 * 2^(log n + 1) points carry it; jf-plonk
// evaluates on 8n only because it wants a power of two.  With M = 2^k = 2n and omega_N = omega_3 * omega_M^c,
// 3c = 1 (mod M)  (so omega_N^3 = omega_M and omega_N^6 = omega_n), the coset 5 <omega_N> is the union of the three
// cosets s_a <omega_M>, s_a = 5 omega_N^a, a = 0, 1, 2, and the evaluations are kept in that order:
//   index a M + k  <->  the point s_a omega_M^k          ("next row", x omega_n, is index a M + (k + 2 mod M)).
// Forward: the evaluations of a polynomial with at most M coefficients on the three cosets are three ordinary
// M-point coset transforms of the SAME zero-extended input - no radix-3 stage, no strided access.
// Inverse (the quotient, up to 3M coefficients): three ordinary inverse transforms of the blocks, then one radix-3
// stage:  t[k + M b] = 5^-(k + M b) / 3 * (Y0[k] + w3^-b omega_N^-k Y1[k] + w3^-2b omega_N^-2k Y2[k]),  w3 = omega_N^M.
// Constants of the five-coset inverse, internal form.  With Y = X^n and u = sum_j Y^j u_j(X) (deg u_j < n) the two inverse
// M-point transforms give, per i < n, E_a = u_0 + c_a^2 u_2 + c_a^4 u_4 and O_a = u_1 + c_a^2 u_3 (a = 0, 1) and the inverse
// n-point transform of block 2 gives R = sum_j c_2^j u_j: a fixed 5 x 5 system whose inverse splits into
//   (u_1, u_3) = odd (O_0, O_1),   (u_0, u_2, u_4) = even (E_0, O_0, E_1, O_1, R).
// mt[j]: coefficients of Mt(Y) = prod_{k<5} (Y - c_k) (monic; t = t_lo + Mt(X^n) h);  d[j] = 1 - mt[j]: the public-input
// addend kappa PI(X) (1 + Y + ... + Y^5) reduced modulo Mt.
struct Quot5Const {
  fe odd[2][2];
  fe even[3][5];
  fe mt[5];
  fe d[5];
};
struct Ntt3Domain {
  uint32_t log_m = 0;           // M = 2^log_m, N = 3 M
  fe* xs_ext = nullptr;         // the N points in the order above, arkworks form
  fe* xs29 = nullptr;           // the same, internal form
  fe* pre3 = nullptr;           // [3][M]: 32 * s_a^i, internal form: pre-scale of the forward sub-transform a
                                //         (arkworks-form coefficients in, internal-form evaluations out)
  fe* tw29_inv = nullptr;       // omega_N^-i, i < 2M, internal form (inverse radix-3 stage)
  fe* coset_inv_ext = nullptr;  // 5^-i / 3, i < N, as an arkworks-form integer: internal-form data in, arkworks out
  fe w3inv_29;                  // omega_N^-M, internal form
  fe omega;                     // omega_N, arkworks form (host)
  // kappa = 1 / (5^N - 1): every point x of the coset has x^N = 5^N, so with n = M / 2 (N = 6n)
  //   1 / (x^n - 1) = kappa (1 + x^n + ... + x^(5n))  there,
  // and the interpolant of A(x) / (x^n - 1) for a polynomial A of degree < n is kappa A(X) (1 + X^n + ... + X^(5n)):
  // A's coefficients, scaled, repeated in the six blocks of n (the `add` of ntt3_inverse)
  fe kappa;                     // arkworks form (host)
  fe kappa_n_inv29;             // kappa / n, internal form: NttIo::post_scalar of the n-point inverse transform that
                                // interpolates such an A from its values
  // ---- five of the six n-cosets (ntt3_forward5 / ntt3_inverse5) ----
  // Element e of block a lies on the n-coset k = a + 3 (e mod 2), where x^n = c_k = 5^n omega_6^k; the quotient has
  // 5n + 8 coefficients, so the cosets k = 0 .. 4 - blocks 0 and 1 and the EVEN elements of block 2, kept compactly:
  // [M][M][M / 2] - carry it once its top 8 coefficients are known.
  fe* unscale5 = nullptr;       // [M] s_0^-i, [M] s_1^-i, [M / 2] s_2^-i as arkworks-form integers (internal in, arkworks out)
  Quot5Const q5;                // the fixed solve and the addends' constants, internal form
};
int ntt3_build_domain(Ntt3Domain* d, uint32_t log_m, hipStream_t stream);
void ntt3_free_domain(Ntt3Domain* d);
// Forward: `count` polynomials (arkworks-form coefficients read through `io`, zero-extended beyond io.src_len <= M) ->
// internal-form evaluations (weakly reduced) in the block order above, written through io's dst addressing.
// dom_m: the 2^log_m domain.  scratch: 3 M count elements.
int ntt3_forward(const Ntt3Domain& d3, const NttDomain& dom_m, const NttSmallTables& small, fe* data, NttIo io,
                 uint32_t count, fe* scratch, hipStream_t stream);
// Inverse in place: data[q * N .. +N) internal-form evaluations (block order) -> arkworks-form coefficients (natural
// order, canonical).  scratch: 6 M count elements.
// add (optional): [count][M / 2] arkworks-form values; coefficient i of array q leaves as t[i] + add[q][i mod M / 2] - all
// six blocks of M / 2, inside the radix-3 stage.  Null: nothing is added.
int ntt3_inverse(const Ntt3Domain& d3, const NttDomain& dom_m, const NttSmallTables& small, fe* data, uint32_t count,
                 fe* scratch, hipStream_t stream, const fe* add = nullptr);

// The same pair on five of the six n-cosets (M >= 32).  Forward: blocks 0 and 1 as above, block 2 as ONE M / 2-point
// coset transform of the polynomial folded modulo X^n - s_2^n (NttIo::src_fold), written to the first M / 2 elements of
// block 2; the rest of the block is not touched.  dom_h: the 2^(log_m - 1) domain.  scratch: 2 M count elements.
int ntt3_forward5(const Ntt3Domain& d3, const NttDomain& dom_m, const NttDomain& dom_h, const NttSmallTables& small,
                  fe* data, NttIo io, uint32_t count, fe* scratch, hipStream_t stream);
// Inverse in place: data[q * N ..) holds [M][M][M / 2] internal-form evaluations -> all N arkworks-form coefficients,
// canonical: t = t_lo + Mt(X^n) h with t_lo the interpolant on the five cosets, top[q][8] = h (arkworks form) and zeros
// above 5n + 8.  add as above: coefficient j n + i takes d_j add[q][i].  scratch: 5 M count elements.
int ntt3_inverse5(const Ntt3Domain& d3, const NttDomain& dom_m, const NttDomain& dom_h, const NttSmallTables& small,
                  fe* data, uint32_t count, fe* scratch, hipStream_t stream, const fe* top, const fe* add = nullptr);

// out[i] = internal Montgomery form (x * 2^261, canonical) of the arkworks-form value in[i]
void ntt_table_to_internal(fe* out, const fe* in, size_t n, hipStream_t stream);

}  // namespace cap
