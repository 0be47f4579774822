// Field inversion by a constant-time extended binary GCD in fixed jumps of divsteps (Bernstein, Yang: "Fast
// constant-time gcd computation and modular inversion", TCHES 2019(3) - "safegcd"), on the limbs of the lazy 29-bit
// field.  Host + device, no HIP needed on the host: tests/cpp/inv_gcd_check.cpp builds this header with field29.hpp's
// bound assertions on.
//
//   inv_gcd<PR, SCHED>(a)   a: any normalized fl in the internal Montgomery form (x * 2^261), lazy, possibly >= p.
//                           Returns a normalized fl below 4p in the same form whose canonical() is that of
//                           a^(p - 2): x^-1 * 2^261, and 0 for every representation of 0 (no test, no branch).
//
// The rule (section 8 of the paper, delta starting at 1; f odd):
//   divstep(delta, f, g) = (1 - delta, g, (g - f) / 2)          if delta > 0 and g is odd
//                          (1 + delta, f, (g + (g mod 2) f) / 2) otherwise
// THE COUNT.  Theorem 11.2 of the paper: for odd f and any g with f^2 + 4 g^2 <= 5 * 2^(2d), d >= 46,
// m = floor((49 d + 57) / 17) divsteps from delta = 1 end in g = 0 and f = +- gcd.  Here f = p and 0 <= g < p < 2^254, so
// f^2 + 4 g^2 < 5 * 2^508: d = 254 and m = floor(12503 / 17) = 735.  Divsteps after g = 0 change neither f nor g (g stays 0,
// f stays put), so the count is rounded up to whole jumps: 26 jumps of 29 = 754 >= 735.  (The "half-delta" start of later
// CPU libraries needs 590; its bound comes from a computer search and is not used here.)
//
// A JUMP of N = 29 divsteps reads only the low 29 bits of f and g - one limb each - and gives a matrix t = (u v; q r) of
// 32-bit signed words, |u| + |v| <= 2^29 and |q| + |r| <= 2^29, with  2^29 (f', g') = t (f, g).  Then
//   (f', g') = t (f, g) / 2^29                      exactly, over the integers (signed limbs, 64-bit columns)
//   (d', e') = t (d, e) / 2^29 mod p                the multiple of p added that makes the low limb vanish
// f, g, d, e: nine limbs, limbs 0 .. 7 in [0, 2^29), limb 8 signed (two's complement: the value is sum v_i 2^(29 i)).
// |f|, |g| <= p throughout (every step halves a sum or difference of two of them); d, e stay in (-2p, p) (the argument of
// update_de below).  Start: f = p, g = canonical(a), d = 0, e = c; then d = c f / g and e = c g / g (mod p) hold after every
// jump, and at the end f = +-1: d = +- c / g.  With g = x 2^261 and c = 2^522 mod p (PR::R522, canonical) that is
// +- x^-1 2^261: the result in the internal form with no product after the loop.  The sign of f selects d or -d by a mask;
// 2p is added and the carries walk up once, so the limbs come out normalized.
//
// Constant time (solve29.hpp:9-12 holds here too): every loop bound is a constant, every choice is a mask or a select on
// words in registers, nothing is indexed by a value.  The inner loop is a dozen and a half 32-bit operations per divstep
// and no multiplication; a jump's two updates are 90 signed 32 x 32 -> 64 multiply-adds.
#pragma once
#include "field29.hpp"

namespace cap {
namespace ig29 {

constexpr int kJump = 29;                                  // divsteps per jump = bits per limb
constexpr int kDivsteps = (49 * 254 + 57) / 17;            // 735 (Theorem 11.2, d = 254: both moduli are below 2^254)
constexpr int kJumps = (kDivsteps + kJump - 1) / kJump;    // 26
static_assert(kDivsteps == 735 && kJumps * kJump >= kDivsteps, "divstep count");

struct sl {  // nine signed limbs
  int32_t v[9];
};
struct Mat {
  int32_t u, v, q, r;
};
// what the loop ends in (host tests read it: g = 0 and f = +-1, or f = p for input 0)
struct End {
  sl f, g;
};

template <class PR, int SCHED = CAP_FL_SCHED>
struct InvGcd {
  using F = Fl<PR, SCHED>;
  static constexpr uint32_t M29 = F::M29;

  // kJump divsteps on the low limbs; eta = -delta.  Returns the new eta.  (u, v, q, r are kept unsigned: they are shifted
  // left while negative.)
  CAP_WRAPS static CAP_HD int32_t divsteps(int32_t eta, uint32_t f, uint32_t g, Mat* t) {
    uint32_t u = 1, v = 0, q = 0, r = 1;
#pragma unroll
    for (int i = 0; i < kJump; i++) {
      uint32_t c1 = (uint32_t)(eta >> 31);  // all ones: delta > 0
      const uint32_t c2 = 0u - (g & 1u);    // all ones: g odd
      // g, q, r += +- (f, u, v) where g is odd: minus where delta > 0
      g += ((f ^ c1) - c1) & c2;
      q += ((u ^ c1) - c1) & c2;
      r += ((v ^ c1) - c1) & c2;
      c1 &= c2;  // the swap: delta > 0 and g odd
      eta = (int32_t)(((uint32_t)eta ^ c1) - (c1 + 1u));  // delta -> 1 - delta, or 1 + delta
      f += g & c1;  // (f + (g - f) = g)
      u += q & c1;
      v += r & c1;
      g >>= 1;
      u <<= 1;
      v <<= 1;
    }
    t->u = (int32_t)u;
    t->v = (int32_t)v;
    t->q = (int32_t)q;
    t->r = (int32_t)r;
    return eta;
  }

  // (f, g) <- t (f, g) / 2^29, exact
  static CAP_HD void update_fg(sl& f, sl& g, const Mat& t) {
    const int64_t u = t.u, v = t.v, q = t.q, r = t.r;
    int64_t cf = u * f.v[0] + v * g.v[0], cg = q * f.v[0] + r * g.v[0];
    CAP_FL_ASSERT(((uint32_t)cf & M29) == 0 && ((uint32_t)cg & M29) == 0);
    cf >>= kJump;
    cg >>= kJump;
#pragma unroll
    for (int i = 1; i < 9; i++) {  // |u f_i + v g_i| <= 2^29 * 2^29, the carry below 2^31
      cf += u * f.v[i] + v * g.v[i];
      cg += q * f.v[i] + r * g.v[i];
      f.v[i - 1] = (int32_t)((uint32_t)cf & M29);
      g.v[i - 1] = (int32_t)((uint32_t)cg & M29);
      cf >>= kJump;
      cg >>= kJump;
    }
    CAP_FL_ASSERT(cf >= -(1 << 25) && cf < (1 << 25) && cg >= -(1 << 25) && cg < (1 << 25));
    f.v[8] = (int32_t)cf;
    g.v[8] = (int32_t)cg;
  }

  // (d, e) <- t (d, e) / 2^29 mod p, both in (-2p, p) before and after.  A negative d (e) first counts as d + p: md = u
  // [d < 0] + v [e < 0] multiples of p ride along, so the sum is u d* + v e* with d*, e* in (-p, p), inside (-2^29 p, 2^29 p)
  // since |u| + |v| <= 2^29.  Then md is lowered by k in [0, 2^29), the k that makes the low limb of the sum 0 mod 2^29:
  // the sum stays above -2^29 p - 2^29 p, and the quotient by 2^29 in (-2p, p).
  CAP_WRAPS static CAP_HD void update_de(sl& d, sl& e, const Mat& t) {
    const int64_t u = t.u, v = t.v, q = t.q, r = t.r;
    const int32_t sd = d.v[8] >> 31, se = e.v[8] >> 31;
    int32_t md = (t.u & sd) + (t.v & se), me = (t.q & sd) + (t.r & se);
    int64_t cd = u * d.v[0] + v * e.v[0], ce = q * d.v[0] + r * e.v[0];
    constexpr uint32_t pinv = (0u - PR::NINV) & M29;  // p^-1 mod 2^29
    md -= (int32_t)((mul_lo32(pinv, (uint32_t)cd) + (uint32_t)md) & M29);
    me -= (int32_t)((mul_lo32(pinv, (uint32_t)ce) + (uint32_t)me) & M29);
    cd += (int64_t)PR::MOD[0] * md;
    ce += (int64_t)PR::MOD[0] * me;
    CAP_FL_ASSERT(((uint32_t)cd & M29) == 0 && ((uint32_t)ce & M29) == 0);
    cd >>= kJump;
    ce >>= kJump;
#pragma unroll
    for (int i = 1; i < 9; i++) {  // |md|, |me| < 2^30: every column below 2^58 + 2^59 + the carry
      cd += u * d.v[i] + v * e.v[i] + (int64_t)PR::MOD[i] * md;
      ce += q * d.v[i] + r * e.v[i] + (int64_t)PR::MOD[i] * me;
      d.v[i - 1] = (int32_t)((uint32_t)cd & M29);
      e.v[i - 1] = (int32_t)((uint32_t)ce & M29);
      cd >>= kJump;
      ce >>= kJump;
    }
    // (-2p, p) at the top limb: p_8 is the modulus's top limb, the limbs below it add less than one unit of it
    CAP_FL_ASSERT(cd >= -2 * (int64_t)PR::MOD[8] - 2 && cd <= (int64_t)PR::MOD[8]);
    CAP_FL_ASSERT(ce >= -2 * (int64_t)PR::MOD[8] - 2 && ce <= (int64_t)PR::MOD[8]);
    d.v[8] = (int32_t)cd;
    e.v[8] = (int32_t)ce;
  }

  static CAP_HD fl run(const fl& a, End* end) {
    const fl g0 = F::canonical(a);
    sl f, g, d, e;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      f.v[i] = (int32_t)PR::MOD[i];
      g.v[i] = (int32_t)g0.v[i];
      d.v[i] = 0;
      e.v[i] = (int32_t)PR::R522[i];
    }
    int32_t eta = -1;
#pragma unroll 1
    for (int j = 0; j < kJumps; j++) {
      Mat t;
      eta = divsteps(eta, (uint32_t)f.v[0], (uint32_t)g.v[0], &t);
      update_de(d, e, t);
      update_fg(f, g, t);
    }
    if (end) {
      end->f = f;
      end->g = g;
    }
    // f = +-1 (p for input 0, where d = 0): +-d + 2p, in (0, 4p), carried into normalized limbs
    const int32_t sf = f.v[8] >> 31;
    fl out;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int32_t x = ((d.v[i] ^ sf) - sf) + (int32_t)(2 * PR::MOD[i]) + c;  // in (-2^29 - 2, 2^30 + 2^29)
      out.v[i] = (uint32_t)x & M29;
      c = x >> kJump;
    }
    const int32_t top = ((d.v[8] ^ sf) - sf) + (int32_t)(2 * PR::MOD[8]) + c;
    CAP_FL_ASSERT(top >= 0 && top < (1 << 29));
    out.v[8] = (uint32_t)top;
    return out;
  }
};

template <class PR, int SCHED>
CAP_HD fl inv_gcd(const fl& a) {
  return InvGcd<PR, SCHED>::run(a, nullptr);
}
// ... with the loop's final f and g handed out (host tests)
template <class PR, int SCHED>
CAP_HD fl inv_gcd(const fl& a, End* end) {
  return InvGcd<PR, SCHED>::run(a, end);
}

}  // namespace ig29
using ig29::inv_gcd;

}  // namespace cap
