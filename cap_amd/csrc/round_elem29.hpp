// The arithmetic of the prover's four lazy-field round kernels (plonk_kernels.hpp: k_perm_numden, k_kx_columns,
// k_quotient<FOLD>, k_lincomb) where a host compiler can reach it: the per-row / per-point bodies as templates over the
// field class F, its value type V and the type W of a 32-byte memory image (Fr29, fl, fe in the kernels).  Memory is
// reached through small functors the kernels pass in, so pointer arithmetic and early exits stay there.
// tests/cpp/round_elem_check.cpp instantiates the same templates on the bound-tracking field of tests/cpp/bound29.hpp:
// every operand at its contract's maximum, every precondition of field29.hpp asserted (tests/golden/lazy_envelope.json).
#pragma once
#include "field29.hpp"

namespace cap {

// Sums of products that share one Montgomery reduction: at most SIX products of normalized operands per 64-bit column
// accumulator - a column takes up to 9 limb products of < 2^58 per mad, and the reduction adds 9 more and a carry:
// (6 * 9 + 9) * 2^58 + 2^36 < 2^64, and a seventh mad would not fit.
template <class F, class V>
struct ColAcc;
template <class F>
struct ColAcc<F, fl> {
  uint64_t c[18];
  CAP_HD void clear() {
#pragma unroll
    for (int k = 0; k < 18; k++) c[k] = 0;
  }
  CAP_HD void mad(const fl& a, const fl& b) {
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
      for (int j = 0; j < 9; j++) c[i + j] += (uint64_t)a.v[i] * b.v[j];
  }
  CAP_HD fl reduce() { return F::reduce_cols(c); }
};

constexpr int kRoundWires = 5;

// round 2: numerator and denominator of one row of the permutation grand product (see k_perm_numden).  beta_ext, gamma,
// tw (omega^j), k[i] and what wire(i), sig(i) return are 32-byte images: any value below 2^256.
template <class F, class V, class W, class WireFn, class SigFn>
static CAP_HD void perm_numden_row(const W& beta_ext, const W& gamma_img, const W& tw, const W* k, WireFn wire, SigFn sig,
                                   W& num, W& den) {
  const V beta = F::from_ext(beta_ext);  // internal form
  const V gamma = F::load(gamma_img);    // arkworks' form, only ever added
  const V bx = F::mul(beta, F::load(tw));
  V a, b;
#pragma unroll 1
  for (int i = 0; i < kRoundWires; i++) {
    const V wg = F::add(F::load(wire(i)), gamma);
    const V t1 = F::normalize(F::add(wg, i == 0 ? bx : F::mul(F::load(k[i]), bx)));
    const V t2 = F::normalize(F::add(wg, F::mul(beta, F::load(sig(i)))));
    a = i == 0 ? t1 : F::mul(a, t1);
    b = i == 0 ? t2 : F::mul(b, t2);
  }
  // 2^20 in the internal form: 2^281 mod r = (2^261 mod r) * 2^20 mod r, by 20 doublings of ONE
  V fix = F::one();
#pragma unroll 1
  for (int j = 0; j < 20; j++) fix = F::weak_reduce(F::add(fix, fix));
  num = F::pack(F::canonical(F::mul(a, fix)));
  den = F::pack(F::canonical(F::mul(b, fix)));
}

// k_kx_columns: k_j x, internal form, canonical
template <class F, class V, class W>
static CAP_HD W kx_elem(const W& k, const V& x) {
  return F::pack(F::canonical(F::mul(F::load(k), x)));
}

// round 3: one point of the quotient (see k_quotient).  sel(s): column s of the key's coset table at the point, col(j):
// coset evaluation j (5 wires, z) of the proof at the point; at.z_next(): z at x omega_n, at.x(): the point, at.inv():
// 1 / (n (x - 1)), at.zh_inv(qc): 1 / Z_H of the point (each evaluated where it is used, as the kernel always did);
// all 32-byte images below 2^256.  CH: Chal, QC: QuotConst (images).
template <bool FOLD, class F, class V, class W, class CH, class QC, class SelFn, class ColFn, class PointFn>
static CAP_HD W quotient_point(SelFn sel_img, ColFn col, PointFn at, const CH& ch, const QC& qc) {
  constexpr int NS = 13, NW = kRoundWires;
  auto sel = [&](int s) { return F::load(sel_img(s)); };
  V w0 = F::load(col(0)), w1 = F::load(col(1)), w2 = F::load(col(2)), w3 = F::load(col(3)), w4 = F::load(col(4));
  // gate constraint (spec eq. (1); selector order q_lc, q_mul, q_hash, q_o, q_c, q_ecc)
  V w01 = F::mul(w0, w1), w23 = F::mul(w2, w3);
  ColAcc<F, V> acc;
  acc.clear();
  acc.mad(sel(0), w0);
  acc.mad(sel(1), w1);
  acc.mad(sel(2), w2);
  acc.mad(sel(3), w3);
  acc.mad(sel(4), w01);
  acc.mad(sel(5), w23);
  V gate = acc.reduce();
  acc.clear();
  {
    V t = F::sqr(w0);
    acc.mad(sel(6), F::mul(F::sqr(t), w0));
    t = F::sqr(w1);
    acc.mad(sel(7), F::mul(F::sqr(t), w1));
    t = F::sqr(w2);
    acc.mad(sel(8), F::mul(F::sqr(t), w2));
    t = F::sqr(w3);
    acc.mad(sel(9), F::mul(F::sqr(t), w3));
  }
  acc.mad(sel(12), F::mul(F::mul(w01, w23), w4));
  acc.mad(F::neg(sel(10)), w4);
  V gate2 = acc.reduce();
  // gate + q_c: three values < 2p each, limbs < 2^31 after the lazy adds
  V total = F::normalize(F::add(F::add(gate, gate2), sel(11)));
  // permutation part:  alpha (z prod_j (w_j + gamma + beta k_j x) - z_omega prod_j (w_j + gamma + beta sigma_j)).
  // With u_j = (w_j + gamma) / beta every factor is beta (u_j + k_j x) resp. beta (u_j + sigma_j): five products by
  // 1 / beta take the place of the ten by beta (beta x, four k_j (beta x), five beta sigma_j), k_j x comes from the key's
  // table (columns 18 .. 21; k_0 = 1: x itself), and the five betas leave with alpha: alpha beta^5 (a' - b').  The same
  // field element as the direct form (the else branch: k_quotient<false>).
  const V gamma = F::load(ch.gamma);
  const V zx = F::load(col(5));
  if constexpr (FOLD) {
    const V beta_inv = F::load(ch.beta_inv);
    // w_j (a stored value: normalized, < 2^256) + gamma (canonical) is a lazy sum of two - limbs < 2^30, what a product
    // takes as it is; u_j is a product (normalized, < 1.2p), and u_j + k_j x (canonical) resp. u_j + sigma_j (stored,
    // < 2^256) again a lazy sum of two that feeds one product: no carry is propagated anywhere in this block
    V a = zx, b = F::load(at.z_next());
    V u = F::mul(F::add(w0, gamma), beta_inv);
    a = F::mul(a, F::add(u, F::load(at.x())));  // the point itself (internal form): s_a * omega_M^k at index a * M + k
    b = F::mul(b, F::add(u, sel(NS + 0)));
    u = F::mul(F::add(w1, gamma), beta_inv);
    a = F::mul(a, F::add(u, sel(NS + NW + 0)));
    b = F::mul(b, F::add(u, sel(NS + 1)));
    u = F::mul(F::add(w2, gamma), beta_inv);
    a = F::mul(a, F::add(u, sel(NS + NW + 1)));
    b = F::mul(b, F::add(u, sel(NS + 2)));
    u = F::mul(F::add(w3, gamma), beta_inv);
    a = F::mul(a, F::add(u, sel(NS + NW + 2)));
    b = F::mul(b, F::add(u, sel(NS + 3)));
    u = F::mul(F::add(w4, gamma), beta_inv);
    a = F::mul(a, F::add(u, sel(NS + NW + 3)));
    b = F::mul(b, F::add(u, sel(NS + 4)));
    // a, b: products (normalized, < 1.2p), as in the direct form
    total = F::normalize(F::add(total, F::mul(F::load(ch.alpha_beta5), F::sub(a, b))));
  } else {
    const V beta = F::load(ch.beta);
    V x = F::load(at.x());  // the point itself (internal form): s_a * omega_M^k at index a * M + k
    V bx = F::mul(beta, x);
    V a = zx, b = F::load(at.z_next());
    V wg = F::add(w0, gamma);
    a = F::mul(a, F::normalize(F::add(wg, bx)));
    b = F::mul(b, F::normalize(F::add(wg, F::mul(beta, sel(NS + 0)))));
    wg = F::add(w1, gamma);
    a = F::mul(a, F::normalize(F::add(wg, F::mul(F::load(qc.k[1]), bx))));
    b = F::mul(b, F::normalize(F::add(wg, F::mul(beta, sel(NS + 1)))));
    wg = F::add(w2, gamma);
    a = F::mul(a, F::normalize(F::add(wg, F::mul(F::load(qc.k[2]), bx))));
    b = F::mul(b, F::normalize(F::add(wg, F::mul(beta, sel(NS + 2)))));
    wg = F::add(w3, gamma);
    a = F::mul(a, F::normalize(F::add(wg, F::mul(F::load(qc.k[3]), bx))));
    b = F::mul(b, F::normalize(F::add(wg, F::mul(beta, sel(NS + 3)))));
    wg = F::add(w4, gamma);
    a = F::mul(a, F::normalize(F::add(wg, F::mul(F::load(qc.k[4]), bx))));
    b = F::mul(b, F::normalize(F::add(wg, F::mul(beta, sel(NS + 4)))));
    total = F::normalize(F::add(total, F::mul(F::load(ch.alpha), F::sub(a, b))));
  }
  // (gate + alpha * perm) / Z_H  +  alpha^2 (z - 1) / (n (x - 1)) : two products, one reduction
  V l1a = F::mul(F::load(ch.alpha2), F::sub(zx, F::one()));
  V r = F::mul_add_mul(total, F::load(at.zh_inv(qc)), l1a, F::load(at.inv()));
  return F::store(r);
}

// k_lincomb: sum_t scalar_t * poly_t[k], six products per reduction.  term.active(t) says whether term t reaches this
// coefficient; term.scalar(t) is its scalar (internal form) and term.value(t) its coefficient (arkworks' form).
// The running total grows by less than 2p per group of six: nterms <= 480 keeps it below the 169p the limbs hold.
template <class F, class V, class W, class TermFn>
static CAP_HD W lincomb_elem(uint32_t nterms, TermFn term) {
  V total = F::zero();
  for (uint32_t t0 = 0; t0 < nterms; t0 += 6) {
    ColAcc<F, V> acc;
    acc.clear();
#pragma unroll
    for (uint32_t u = 0; u < 6; u++) {
      const uint32_t t = t0 + u;
      if (term.active(t)) acc.mad(F::load(term.scalar(t)), F::load(term.value(t)));
    }
    total = F::normalize(F::add(total, acc.reduce()));
  }
  return F::pack(F::canonical(total));
}

}  // namespace cap
