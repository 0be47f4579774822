// BN254 G1 in XYZZ coordinates on the lazy 29-bit field (field29.hpp).  Same formulas as curve.hpp
// (madd-2008-s, add-2008-s, dbl-2008-s-1); what changes is bound bookkeeping instead of conditional
// subtractions.  Invariants of a point held in registers (`g1x`):
//     x, y   normalized, < 2p      (weak_reduce'd: they are differences)
//     zz,zzz normalized, < 1.1p    (products)
//     infinity  <=>  zz is the literal 0
// That is what the general functions (dbl*, add, add_mixed, term_mul) RETURN.  They ACCEPT more: the accumulator class of
// the lean forms below (x < 2p, y < 3p, zz, zzz < 1.2p - what madd_acc, add_affine_pair and add_acc take and return) and
// a point loaded from any four 32-byte images.  tests/cpp/curve_envelope_check.cpp runs this law on a field whose values
// are bounds and shows both classes to close under every chain the kernels build (tests/golden/lazy_envelope.json,
// section "curve", which also records how much further "y < k p" would still close for each lean form).
// Affine table entries (`g1_affine` in memory) hold canonical values (< p) in internal Montgomery form
// (x * 2^261 mod p); (0, 0) encodes infinity.  Bucket points in memory (`g1_xyzz`) hold any value < 2^256.
#pragma once
#include "curve.hpp"
#include "field29.hpp"

namespace cap {

struct g1a {  // affine, registers
  fl x, y;
};
struct g1x {  // XYZZ, registers
  fl x, y, zz, zzz;
};

// What goes with a field value type V: the register points, the memory images and the C ABI's constants.  The law below
// is written once over the field class F and V; tests/cpp/bound_curve29.hpp supplies the set for a field whose values are
// bounds (tests/cpp/curve_envelope_check.cpp runs the law on it for every input of a class).
template <class V>
struct G1Types;
template <>
struct G1Types<fl> {
  using A = g1a;
  using X = g1x;
  using MA = g1_affine;
  using MX = g1_xyzz;
  using MJ = g1_jac;
  static CAP_HD fe ext_one() { return Fq::one(); }
  static CAP_HD fe ext_zero() { return Fq::zero(); }
};
// the literal 0: every limb zero
static CAP_HD bool limbs_all_zero(const fl& a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) o |= a.v[i];
  return o == 0;
}

template <class F_, class V>
struct G1Law {
  using F = F_;
  using fl = V;
  using g1a = typename G1Types<V>::A;
  using g1x = typename G1Types<V>::X;
  using g1_affine = typename G1Types<V>::MA;
  using g1_xyzz = typename G1Types<V>::MX;
  using g1_jac = typename G1Types<V>::MJ;

  static CAP_HD bool all_zero(const fl& a) { return limbs_all_zero(a); }
  static CAP_HD bool is_inf(const g1x& p) { return all_zero(p.zz); }
  static CAP_HD bool is_inf(const g1a& p) { return all_zero(p.x) && all_zero(p.y); }
  static CAP_HD g1x inf() {
    g1x r;
    r.x = F::zero();
    r.y = F::zero();
    r.zz = F::zero();
    r.zzz = F::zero();
    return r;
  }
  static CAP_HD g1x from_affine(const g1a& p) {
    if (is_inf(p)) return inf();
    g1x r;
    r.x = p.x;
    r.y = p.y;
    r.zz = F::one();
    r.zzz = F::one();
    return r;
  }

  // ---- memory images ------------------------------------------------------------------------------------
  static CAP_HD g1a load(const g1_affine& m) {
    g1a r;
    r.x = F::load(m.x);
    r.y = F::load(m.y);
    return r;
  }
  static CAP_HD g1x load(const g1_xyzz& m) {
    g1x r;
    r.x = F::load(m.x);
    r.y = F::load(m.y);
    r.zz = F::load(m.zz);
    r.zzz = F::load(m.zzz);
    return r;
  }
  static CAP_HD g1_xyzz store(const g1x& p) {  // coordinates are already < 2p: pack only
    g1_xyzz m;
    m.x = F::pack(p.x);
    m.y = F::pack(p.y);
    m.zz = F::pack(p.zz);
    m.zzz = F::pack(p.zzz);
    return m;
  }
  static CAP_HD g1_affine store_affine(const g1a& p) {  // canonical
    g1_affine m;
    m.x = F::pack(F::canonical(p.x));
    m.y = F::pack(F::canonical(p.y));
    return m;
  }

  // ---- group law --------------------------------------------------------------------------------------------
  // doubling of an affine point (mdbl-2008-s-1); q canonical / < 2p
  static CAP_HD g1x dbl_affine(const g1a& q) {
    if (is_inf(q)) return inf();
    fl u = F::add(q.y, q.y);
    fl v = F::sqr(u);
    fl w = F::mul(u, v);
    fl s = F::mul(q.x, v);
    fl xx = F::sqr(q.x);
    fl m = F::normalize(F::add(F::add(xx, xx), xx));
    g1x r;
    r.x = F::weak_reduce(F::sub(F::sqr(m), F::add(s, s)));
    r.y = F::weak_reduce(F::mul_add_mul(m, F::sub(s, r.x), F::neg(w), q.y));
    r.zz = v;
    r.zzz = w;
    return r;
  }
  static CAP_HD g1x dbl(const g1x& p) {
    if (is_inf(p)) return p;
    fl u = F::add(p.y, p.y);
    fl v = F::sqr(u);
    fl w = F::mul(u, v);
    fl s = F::mul(p.x, v);
    fl xx = F::sqr(p.x);
    fl m = F::normalize(F::add(F::add(xx, xx), xx));
    g1x r;
    r.x = F::weak_reduce(F::sub(F::sqr(m), F::add(s, s)));
    r.y = F::weak_reduce(F::mul_add_mul(m, F::sub(s, r.x), F::neg(w), p.y));
    r.zz = F::mul(v, p.zz);
    r.zzz = F::mul(w, p.zzz);
    return r;
  }
  // acc + q, q affine; `negate` adds -q.  Handles infinity on either side, acc == q and acc == -q.
  static CAP_HD g1x add_mixed(const g1x& a, const g1a& q_in, bool negate = false) {
    if (is_inf(q_in)) return a;
    g1a q = q_in;
    if (negate) q.y = F::neg(q.y);  // 16p - y: normalized, fine as a multiplicand
    if (is_inf(a)) {
      g1x r;
      r.x = q.x;
      r.y = negate ? F::weak_reduce(q.y) : q.y;
      r.zz = F::one();
      r.zzz = F::one();
      return r;
    }
    fl u2 = F::mul(q.x, a.zz);
    fl s2 = F::mul(q.y, a.zzz);
    fl p = F::sub(u2, a.x);
    fl r = F::sub(s2, a.y);
    if (F::is_zero(p)) {
      if (F::is_zero(r)) {
        g1a qq;
        qq.x = q.x;
        qq.y = F::weak_reduce(q.y);
        return dbl_affine(qq);
      }
      return inf();
    }
    fl pp = F::sqr(p);
    fl ppp = F::mul(p, pp);
    fl qq = F::mul(a.x, pp);
    g1x o;
    o.x = F::weak_reduce(F::sub(F::sub(F::sqr(r), ppp), F::add(qq, qq)));
    o.y = F::weak_reduce(F::mul_add_mul(r, F::sub(qq, o.x), F::neg(a.y), ppp));  // one reduction for both products
    o.zz = F::mul(a.zz, pp);
    o.zzz = F::mul(a.zzz, ppp);
    return o;
  }
  // The mixed addition of the bucket-accumulation loop (msm_accumulate): acc += q (or -q), common case only.
  // Returns false - acc untouched - when the x-difference vanishes, which is how EVERY special case shows up: the
  // accumulator at infinity (zz = 0 and x = 0 make both sides 0), acc == q (doubling), acc == -q (cancellation); the
  // caller then takes the general add_mixed.  q must not be the point at infinity (the caller tests that).
  // Compared with add_mixed the carries are propagated only where the next operation needs them:
  //   * -q.y is 16p - y with un-carried limbs (< 2^31): it is one operand of one multiplication;
  //   * r^2 - ppp - 2qq is carried once, not twice;  qq - x3 (+ 2p, limbs < 1.5 * 2^30) feeds the fused product directly;
  //   * -acc.y is 4p - y with un-carried limbs (< 2^30);  y3 stays a product sum (< 1.5 p) without the weak reduction.
  // Invariants of acc here: x < 2p, y < 3p, zz, zzz < 1.2p, all with normalized limbs.
  static CAP_HD bool madd_acc(g1x& a, const g1a& q, bool negate) {
    const fl qy = negate ? F::neg_lazy(q.y) : q.y;
    const fl u2 = F::mul(q.x, a.zz);
    const fl s2 = F::mul(qy, a.zzz);
    const fl p = F::sub(u2, a.x);
    if (F::is_zero(p)) return false;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("; madd_acc: common path");  // no instruction: tools/isa_mix.py finds the hot block by this line
#endif
    const fl r = F::sub(s2, a.y);
    const fl pp = F::sqr(p);
    const fl ppp = F::mul(p, pp);
    const fl qq = F::mul(a.x, pp);
    g1x o;
    o.x = F::weak_reduce(F::sub_from_lazy(F::sub2p_lazy(F::sqr(r), ppp), F::add(qq, qq)));
    // one reduction for both products; both second operands un-carried: 9 x (2^29 * 1.5 * 2^30 + 2^30 * 2^29) plus the
    // reduction terms stays below 2^64 per column
    o.y = F::mul_add_mul(r, F::sub2p_lazy(qq, o.x), F::neg4p_lazy(a.y), ppp);
    o.zz = F::mul(a.zz, pp);
    o.zzz = F::mul(a.zzz, ppp);
    a = o;
    return true;
  }
  // The first addition of an item of msm_accumulate: out = (+-q0) + (+-q1) for two AFFINE table points (canonical, as
  // the table holds them), common case only.  With both z = 1 the cross products u2, s2 and the two products into zz,
  // zzz of the mixed addition fall away: 2 squarings, 2 products and the fused pair, 5 reductions, against the 2 + 10.5
  // multiplication-equivalents of add_mixed from infinity followed by madd_acc.
  // Returns false - out untouched - when the x-difference vanishes: q1 == +-q0; the caller then starts the item as
  // before.  Neither point may be the point at infinity (the caller tests both).
  // Carries and bounds:
  //   * p = x1 - x0 + 2p is carried (it is squared) and < 3p, so that zz = p^2 and zzz = p^3 come out < 1.1p;
  //   * +-y is y or 2p - y with un-carried limbs (< 2^30): the operands of one carried subtraction (r < 18p) and, with
  //     the opposite sign, the un-carried multiplicand of the fused product, as 4p - acc.y is in madd_acc;
  //   * x3 and y3 exactly as in madd_acc: y3 = r (qq - x3 + 2p) + (-+y0) ppp < (18 * 3.1 + 2 * 1.1) p^2 / 169p + p < 1.4p.
  // Out: the invariants madd_acc states - x < 2p, y < 3p, zz, zzz < 1.2p, normalized limbs.
  static CAP_HD bool add_affine_pair(g1x& out, const g1a& q0, bool neg0, const g1a& q1, bool neg1) {
    const fl p = F::sub2p(q1.x, q0.x);
    if (F::is_zero(p)) return false;
    const fl n0 = F::neg2p_lazy(q0.y);
    const fl y0 = neg0 ? n0 : q0.y, my0 = neg0 ? q0.y : n0;
    const fl y1 = neg1 ? F::neg2p_lazy(q1.y) : q1.y;
    const fl r = F::sub(y1, y0);
    const fl pp = F::sqr(p);
    const fl ppp = F::mul(p, pp);
    const fl qq = F::mul(q0.x, pp);
    g1x o;
    o.x = F::weak_reduce(F::sub_from_lazy(F::sub2p_lazy(F::sqr(r), ppp), F::add(qq, qq)));
    o.y = F::mul_add_mul(r, F::sub2p_lazy(qq, o.x), my0, ppp);
    o.zz = pp;
    o.zzz = ppp;
    out = o;
    return true;
  }
  // a += b for two XYZZ points, common case only - the running sums of the bucket reduction (msm_reduce_segments).
  // Returns false - a untouched - when the x-difference vanishes: either side at infinity (zz = 0 and x = 0 make both
  // cross products 0), a == b, a == -b; the caller falls back to add().  Carries as in madd_acc.
  // Invariants in and out: x < 2p, y < 3p, zz, zzz < 1.2p, normalized limbs.
  static CAP_HD bool add_acc(g1x& a, const g1x& b) {
    const fl u1 = F::mul(a.x, b.zz);
    const fl u2 = F::mul(b.x, a.zz);
    const fl p = F::sub(u2, u1);
    if (F::is_zero(p)) return false;
    const fl s1 = F::mul(a.y, b.zzz);
    const fl s2 = F::mul(b.y, a.zzz);
    const fl r = F::sub(s2, s1);
    const fl pp = F::sqr(p);
    const fl ppp = F::mul(p, pp);
    const fl qq = F::mul(u1, pp);
    g1x o;
    o.x = F::weak_reduce(F::sub_from_lazy(F::sub2p_lazy(F::sqr(r), ppp), F::add(qq, qq)));
    o.y = F::mul_add_mul(r, F::sub2p_lazy(qq, o.x), F::neg2p_lazy(s1), ppp);
    o.zz = F::mul(F::mul(a.zz, b.zz), pp);
    o.zzz = F::mul(F::mul(a.zzz, b.zzz), ppp);
    a = o;
    return true;
  }
  static CAP_HD g1x add(const g1x& a, const g1x& b) {
    if (is_inf(a)) return b;
    if (is_inf(b)) return a;
    fl u1 = F::mul(a.x, b.zz);
    fl u2 = F::mul(b.x, a.zz);
    fl s1 = F::mul(a.y, b.zzz);
    fl s2 = F::mul(b.y, a.zzz);
    fl p = F::sub(u2, u1);
    fl r = F::sub(s2, s1);
    if (F::is_zero(p)) {
      if (F::is_zero(r)) return dbl(a);
      return inf();
    }
    fl pp = F::sqr(p);
    fl ppp = F::mul(p, pp);
    fl qq = F::mul(u1, pp);
    g1x o;
    o.x = F::weak_reduce(F::sub(F::sub(F::sqr(r), ppp), F::add(qq, qq)));
    o.y = F::weak_reduce(F::mul_add_mul(r, F::sub(qq, o.x), F::neg(s1), ppp));
    o.zz = F::mul(F::mul(a.zz, b.zz), pp);
    o.zzz = F::mul(F::mul(a.zzz, b.zzz), ppp);
    return o;
  }

  // ---- scalar multiplication of one term (k_verify_terms, verify_dev.hip) ---------------------------------------
  // index of the highest set bit of a non-zero word
  static CAP_HD int top_bit(uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return 31 - __clz(w);
#else
    return 31 - __builtin_clz(w);
#endif
  }
  // [k] P for an affine P (internal form) and a 256-bit integer k (taken as the integer it is, not reduced): two bits
  // per step from the top
  static CAP_HD g1x term_mul(const g1a& b, const fe& k) {
    int top = -1;
    for (int i = 7; i >= 0 && top < 0; i--)
      if (k.v[i]) top = 32 * i + top_bit(k.v[i]);
    if (top < 0 || is_inf(b)) return inf();
    const g1x b2 = dbl_affine(b);
    const g1x b3 = add_mixed(b2, b);
    g1x acc = inf();
#pragma unroll 1
    for (int pos = top | 1; pos >= 1; pos -= 2) {  // digit = bits pos, pos - 1
      acc = dbl(dbl(acc));
      const uint32_t d = (k.v[(pos - 1) >> 5] >> ((pos - 1) & 31)) & 3u;
      if (d == 1) acc = add_mixed(acc, b);
      else if (d) acc = add(acc, d == 2 ? b2 : b3);
    }
    return acc;
  }

  // ---- inversion (a^(p-2)) and normalisation to affine ------------------------------------------------
  static CAP_HD fl inv(const fl& a) {
    // exponent p - 2, 32-bit words of the modulus
    fl r = F::one();
    bool started = false;
    for (int i = 7; i >= 0; i--) {
      uint32_t e = FqP::MOD[i] - (i == 0 ? 2u : 0u);  // low word of p is ...fd47: no borrow
      for (int b = 31; b >= 0; b--) {
        if (started) r = F::sqr(r);
        if ((e >> b) & 1) {
          r = started ? F::mul(r, a) : a;
          started = true;
        }
      }
    }
    return r;
  }
  static CAP_HD g1a to_affine(const g1x& p) {
    g1a r;
    if (is_inf(p)) {
      r.x = F::zero();
      r.y = F::zero();
      return r;
    }
    fl zi = inv(p.zzz);              // 1/zzz
    fl t = F::mul(zi, p.zz);         // zz/zzz
    fl zz_inv = F::sqr(t);           // zz^3 = zzz^2  =>  (zz/zzz)^2 = 1/zz
    r.x = F::mul(p.x, zz_inv);
    r.y = F::mul(p.y, zi);
    return r;
  }
  // the Jacobian triple of the C ABI, external Montgomery form (x * 2^256), canonical
  static CAP_HD g1_jac to_jac_ext(const g1x& p) {
    g1_jac r;
    if (is_inf(p)) {
      r.x = G1Types<V>::ext_one();
      r.y = G1Types<V>::ext_one();
      r.z = G1Types<V>::ext_zero();
      return r;
    }
    r.x = F::to_ext(F::mul(p.x, p.zz));
    r.y = F::to_ext(F::mul(p.y, p.zzz));
    r.z = F::to_ext(p.zz);
    return r;
  }
};
// the law on the lazy field with multiplication schedule SCHED: what every kernel uses
template <int SCHED>
struct G1LT : G1Law<Fl<FqP29, SCHED>, fl> {};
using G1L = G1LT<CAP_FL_SCHED>;  // the translation unit's default multiplication schedule (field29.hpp)

}  // namespace cap
