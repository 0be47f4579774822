// The field code of the solver's DEFERRED form (the rule: solve_defer.hpp) on the lazy 29-bit field.  Host + device, like
// solve29.hpp, whose text it leaves alone: tests/cpp/solve_defer_check.cpp builds this header for the host with field29.hpp's
// bound assertions on and compares every value with the direct walk, limb for limb.
//
// Cell i < 4 of a FRAC row holds (N_i, D_i), D_i = 1 for a plain variable.  With
//   D = D0 D1 D2 D3,   E_i = prod_{j != i} D_j,   P = N0 N1 N2 N3
//   R' = q_c D + sum_i q_lc_i N_i E_i + q_mul0 (N0 N1)(D2 D3) + q_mul1 (N2 N3)(D0 D1) + sum_i q_hash_i N_i^5 D
// (the plan admits the row only when every pending cell has q_hash_i = 0, so the last sum runs over plain cells) the row's
// variable is
//   OUT_MUL   (N4, D4) = (R' / q_o, D)                  the constant 1 / q_o of the direct row
//   OUT_INV   (N4, D4) = (R', q_o D - q_ecc P);  D4 = 0 mod r: the row is reported and (N4, D4) = (0, 1) by a mask
// R' is `rest` of solve29.hpp over the numerators with every selector scaled by its cofactor: one text for the sums and
// their bounds.  Every scaled selector is a product (normalized, below 1.1 r), as a selector's own image is.
// D != 0 is an invariant - D4 = 0 exactly where the direct row's denominator q_o - q_ecc w0 w1 w2 w3 = D4 / D is 0.
//
// TIMING (include/capgpu.h).  No branch, loop bound or address depends on a value: which cells are pending and how many
// pairs a flush item resolves are the plan's; a cell's denominator is selected between its image and 1 by the plan's mask;
// the one data-dependent step is still the zero test of a row's own denominator, whose outcome is reported.
#pragma once
#include "solve29.hpp"

namespace cap {
namespace sv29 {

template <int SCHED = CAP_FL_SCHED, int INV = kInvFermat>
struct Defer {
  using S = Solve<SCHED, INV>;
  using F = typename S::F;

  // kind: 0 (OUT_MUL) or 1 (OUT_INV); num / den: the four input cells (den[i] = F::one() for a plain cell; normalized,
  // as from_ext and load give them); konst: 1 / q_o (OUT_MUL).  -> the pair (*n4, *d4), normalized; the return value: an
  // OUT_INV row whose denominator is 0 mod r.
  template <class Sel>
  static CAP_HD bool row_value_frac(Sel q, uint32_t kind, const fl* num, const fl* den, const fl& konst, fl* n4, fl* d4) {
    const fl d01 = F::mul(den[0], den[1]), d23 = F::mul(den[2], den[3]);
    const fl d = F::mul(d01, d23);
    const fl e0 = F::mul(den[1], d23), e1 = F::mul(den[0], d23), e2 = F::mul(d01, den[3]), e3 = F::mul(d01, den[2]);
    fl p;
    const fl r = S::rest(
        [&](int s) {
          // the selector times its cofactor.  (s is a compile-time constant at every call of rest but the hash pairs',
          // whose index runs; their cofactor is d either way, and that case stands first so that no select is left)
          if (s >= wc29::Q_HASH && s < wc29::Q_HASH + 4) return F::mul(q(s), d);
          if (s == wc29::Q_LC) return F::mul(q(s), e0);
          if (s == wc29::Q_LC + 1) return F::mul(q(s), e1);
          if (s == wc29::Q_LC + 2) return F::mul(q(s), e2);
          if (s == wc29::Q_LC + 3) return F::mul(q(s), e3);
          if (s == wc29::Q_MUL) return F::mul(q(s), d23);
          if (s == wc29::Q_MUL + 1) return F::mul(q(s), d01);
          return F::mul(q(s), d);  // Q_C
        },
        num, &p);
    if (kind == 0) {
      *n4 = F::mul(r, konst);
      *d4 = d;
      return false;
    }
    const fl dd = F::sub(F::mul(q(wc29::Q_O), d), F::mul(q(wc29::Q_ECC), p));
    const bool z = F::is_zero(dd);
    // (0, 1) for a zero denominator, by a mask over the limbs: all ones to keep the pair
    const uint32_t keep = (uint32_t)z - 1u;
    const fl one = F::one();
#pragma unroll
    for (int i = 0; i < 9; i++) {
      n4->v[i] = r.v[i] & keep;
      d4->v[i] = (dd.v[i] & keep) | (one.v[i] & ~keep);
    }
    return z;
  }

  // the inverse of a non-zero value in the form INV
  static CAP_HD fl inverse(const fl& a, const Exps& ex) {
    if constexpr (INV == kInvGcd) {
      return inv_gcd<FrP29, SCHED>(a);
    } else {
      return S::pow_words(a, [&](int w) { return ex.inv[w]; });
    }
  }

  // A flush item: v_i = N_i / D_i for i < count with ONE inversion.  den(i) / num(i): the pair's images; pre_store(i, x) /
  // pre_load(i): room for one value per pair (the prefix products D_0 .. D_{i-1}); put(i, v): the plain value.
  // count is the plan's; every D_i != 0.
  template <class Den, class Num, class PreStore, class PreLoad, class Put>
  static CAP_HD void flush_group(uint32_t count, Den den, Num num, PreStore pre_store, PreLoad pre_load, Put put, const Exps& ex) {
    fl acc = F::one();
#pragma unroll 1
    for (uint32_t i = 0; i < count; i++) {
      pre_store(i, acc);
      acc = F::mul(acc, den(i));
    }
    acc = inverse(acc, ex);
#pragma unroll 1
    for (uint32_t i = count; i-- > 0;) {
      const fl di = F::mul(acc, pre_load(i));  // 1 / D_i
      acc = F::mul(acc, den(i));
      put(i, F::mul(num(i), di));
    }
  }
};

}  // namespace sv29
}  // namespace cap
