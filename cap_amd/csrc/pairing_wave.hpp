// The BN254 pairing check of pairing29.hpp in the form meant for latency: one Fq12 value spread over a group of SIX adjacent lanes
// of a wavefront, lane k holding the Fq2 coefficient of w^k (Fq12 = Fq2[w]/(w^6 - xi), the tower of pairing29.hpp read
// along w:  k = 0..5  <->  a0, b0, a1, b1, a2, b2  of  c0 = (a0, a1, a2), c1 = (b0, b1, b2)).
//
// Why.  k_pairing_check2 (verify_dev.hip) runs one check per lane: ~20 k dependent Fq products, 256 VGPRs + 256 AGPRs and
// 9.4 KB of scratch per lane, ~22 ms whether it decides 1 proof or 256 - the chip is empty and the chain is long.  The
// group form pays the chain in depth instead of lanes, as quad29.hpp does for the point additions that end a small MSM:
//                           one lane (pairing29.hpp)      lane k of a group (Fq products in sequence)
//   Fq12 product            54                            18   six Fq2 products  a_i b_(k-i), schoolbook along w
//   Fq12 squaring           36                            12   four Fq2 products: the unordered pairs {i, j}, i + j = k
//   sparse line product     42 + 2                         8 + 2
//   cyclotomic squaring     18                             3   one Fq2 product of the Fq4 squaring its lane belongs to
//   Frobenius               15                             3
// about 5 k instead of 20 k products in sequence per check by this count (not timed on the device yet), and no Fq12 ever
// sits in one lane's registers.
//
// Choice of L and of the distribution (candidates: 12 or 16 lanes holding one Fq of pairing.hpp's flat basis w^i, 6 or 8
// lanes holding one Fq2):
//   * The flat basis reduces by w^12 = 18 w^6 - 82, two extra constant products per wrapped term and bounds that grow
//     with the 18 and the 82; the tower's w^6 = xi = 9 + u wraps with mul_xi, additions only.  One Fq per lane would also
//     split every Fq2 product of the line, Frobenius and Granger-Scott formulas over two lanes (they are written in Fq2).
//   * With one Fq2 per lane every lane runs Tower<>::f2_* on whole Fq2 values: the bound contract of pairing29.hpp
//     (every held Fq normalized and < 2p) holds per lane unchanged, and the host test compares with Tower<> directly.
//   * 6 against 8: the exchange is ds_bpermute_b32 (any lane to any lane of the wavefront through the LDS crossbar, no
//     LDS memory, no barrier); a power-of-two group would only matter for DPP row operations, which cannot express the
//     rotations by k - i that the product needs.  6 lanes give floor(64 / 6) = 10 checks per wavefront against 8, with
//     4 idle lanes instead of 16.
//   Cost of the exchange: an Fq2 is 18 words, so an Fq12 product moves 2 x 6 x 18 = 216 words per lane against
//   18 Fq products of ~220 instructions each (~5 %); the moves of one product are independent of each other and are
//   issued ahead of the arithmetic.
//
// Resource use (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, k_pairing_check2_wave):
//   VGPRs 256, AGPRs 177, ScratchSize 0 bytes/lane, no dynamic stack, no VGPR spill, LDS 0, one wave per SIMD
// (k_pairing_check2: VGPRs 256, AGPRs 256, 9.4 KB of scratch per lane).  The group form keeps every Fq12-level operation
// inline (no call, so no argument area) and the final exponentiation is a table-driven program over six Fq12 registers
// (below), so the kernel holds ONE copy of each Fq12 operation.  Two things keep the stack at zero: registers of that
// program are chosen by comparison, never by index, and a choice between two Fq2 values is made word by word (pick) -
// a conditional between two struct lvalues selects an address and cost 364 bytes per lane in the first build.
//
// Bounds.  Every group operation is built from Tower<>::f2_add / f2_sub / f2_mul / f2_mul_xi / f2_mul_fq ..., whose
// results are normalized and < 2p (pairing29.hpp); nothing here adds limbs across lanes without a weak reduction, so the
// cross-lane sums of partial products are sums of values < 2p reduced after every addition - the same invariant as the
// one-lane tower.  The accumulations below say so where they happen.  tests/hip/pairing_wave_host.cpp runs this file
// on six emulated lanes with CAP_FL_CHECK and the unsigned-overflow sanitizer against Tower<>.
#pragma once
#include "pairing29.hpp"

namespace cap {
namespace pw {

using p29::f2;
using p29::line_coeffs;
using p29::PairConst;

constexpr int kGroup = 6;                    // lanes per check
constexpr int kGroupsPerWave = 64 / kGroup;  // 10

// ---- lane policies (as quad29.hpp) ------------------------------------------------------------------------------------
// V: what one "instruction" operates on.  map(f, a...): lane k gets f(k, a_k...).  from(a, src): lane k gets the value of
// lane src(k) of its group.  all(f, a): f(k, a_k) holds in every lane of the group.
#if defined(__HIPCC__)
struct GroupDev {
  using V = f2;
  // lanes 60..63 belong to no group: they shadow lanes 0..3 of the last group (they read, never decide or store)
  static __device__ __forceinline__ int base() {
    const int lane = (int)(threadIdx.x & 63), g = lane / kGroup;
    return g < kGroupsPerWave ? g * kGroup : (kGroupsPerWave - 1) * kGroup;
  }
  static __device__ __forceinline__ int k() {
    const int lane = (int)(threadIdx.x & 63), g = lane / kGroup;
    return lane - g * kGroup;
  }
  template <class Fn, class... A>
  static __device__ __forceinline__ V map(Fn f, const A&... a) { return f(k(), a...); }
  static __device__ __forceinline__ uint32_t pull(uint32_t v, int src) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((base() + src) << 2, (int)v);
  }
  template <class Src>
  static __device__ __forceinline__ V from(const V& a, Src src) {
    const int s = src(k());
    V r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      r.c0.v[i] = pull(a.c0.v[i], s);
      r.c1.v[i] = pull(a.c1.v[i], s);
    }
    return r;
  }
  template <class Fn>
  static __device__ __forceinline__ bool all(Fn f, const V& a) {
    const uint32_t mine = f(k(), a) ? 1u : 0u;
    uint32_t r = 1;
#pragma unroll
    for (int i = 0; i < kGroup; i++) r &= pull(mine, i);
    return r != 0;
  }
};
#endif

struct f2x6 {  // host emulation: the six lanes of one group
  f2 l[kGroup];
};
struct GroupSim {
  using V = f2x6;
  template <class Fn, class... A>
  static V map(Fn f, const A&... a) {
    V r;
    for (int k = 0; k < kGroup; k++) r.l[k] = f(k, a.l[k]...);
    return r;
  }
  template <class Src>
  static V from(const V& a, Src src) {
    V r;
    for (int k = 0; k < kGroup; k++) r.l[k] = a.l[src(k)];
    return r;
  }
  template <class Fn>
  static bool all(Fn f, const V& a) {
    bool r = true;
    for (int k = 0; k < kGroup; k++) r = f(k, a.l[k]) && r;
    return r;
  }
};

// ---- the squaring's schedule: lane k multiplies the unordered pairs {i, j}, i <= j, i + j = k (mod 6) ----------------
// slot t of lane k: bits 3k.. of SQ_I[t] / SQ_J[t] the two source lanes; bit k of SQ_USED[t] the slot is taken, of
// SQ_DBL[t] i != j (the product counts twice), of SQ_WRAP[t] i + j >= 6 (times w^6 = xi).  Even k have two squares and
// two cross pairs, odd k three cross pairs.
struct SqSchedule {
  uint32_t i[4], j[4], used[4], dbl[4], wrap[4];
};
constexpr SqSchedule make_sq_schedule() {
  SqSchedule s{};
  for (int k = 0; k < kGroup; k++) {
    int t = 0;
    for (int i = 0; i < kGroup; i++)
      for (int j = i; j < kGroup; j++)
        if ((i + j) % kGroup == k) {
          s.i[t] |= (uint32_t)i << (3 * k);
          s.j[t] |= (uint32_t)j << (3 * k);
          s.used[t] |= 1u << k;
          if (i != j) s.dbl[t] |= 1u << k;
          if (i + j >= kGroup) s.wrap[t] |= 1u << k;
          t++;
        }
  }
  return s;
}

// ---- the final exponentiation as a program over six Fq12 registers ----------------------------------------------------
// One instruction = op << 12 | d << 8 | a << 4 | b.  Tower<>::final_exp, same operations in the same order; a^x is
// expanded into its 62 cyclotomic squarings and 27 products, so that the kernel holds one copy of each operation.
enum Op : uint32_t { OP_MUL = 0, OP_CSQ = 1, OP_CONJ = 2, OP_FROB = 3, OP_NINV = 4, OP_COPY = 5 };
constexpr int kRegs = 6;
struct Program {
  uint16_t ins[320];
  int n;
};
constexpr Program make_final_exp() {
  Program p{};
  auto emit = [&](uint32_t op, int d, int a, int b) { p.ins[p.n++] = (uint16_t)(op << 12 | d << 8 | a << 4 | b); };
  auto exp_neg_x = [&](int d, int a) {  // d = conj(a^x), d != a
    emit(OP_COPY, d, a, 0);
    for (int i = 61; i >= 0; i--) {
      emit(OP_CSQ, d, d, 0);
      if ((PairConst::CURVE_X >> i) & 1) emit(OP_MUL, d, d, a);
    }
    emit(OP_CONJ, d, d, 0);
  };
  // easy part: R0 = f^((p^6 - 1)(p^2 + 1));  f^-1 = conj(f) / (f conj(f)), the norm f conj(f) lies in Fq6 (even lanes)
  emit(OP_CONJ, 1, 0, 0);  // R1 = conj(f)
  emit(OP_MUL, 2, 0, 1);   // R2 = f conj(f)
  emit(OP_NINV, 2, 2, 0);  // R2 = 1 / R2  (in Fq6)
  emit(OP_MUL, 2, 1, 2);   // R2 = f^-1
  emit(OP_MUL, 0, 1, 2);   // R0 = conj(f) f^-1
  emit(OP_FROB, 1, 0, 2);
  emit(OP_MUL, 0, 1, 0);   // R0 = r
  // hard part (Fuentes-Castaneda, Knapp, Rodriguez-Henriquez), names as in Tower<>::final_exp
  exp_neg_x(1, 0);         // R1 = y0
  emit(OP_CSQ, 1, 1, 0);   // R1 = y1
  emit(OP_CSQ, 2, 1, 0);   // R2 = y2
  emit(OP_MUL, 2, 2, 1);   // R2 = y3
  exp_neg_x(3, 2);         // R3 = y4
  emit(OP_CSQ, 4, 3, 0);   // R4 = y5
  exp_neg_x(5, 4);
  emit(OP_CONJ, 5, 5, 0);  // R5 = y6 = conj(y5^-x)
  emit(OP_MUL, 5, 5, 3);   // R5 = y7 = y6 y4
  emit(OP_CONJ, 2, 2, 0);
  emit(OP_MUL, 5, 5, 2);   // R5 = y8 = y7 conj(y3)
  emit(OP_MUL, 2, 5, 1);   // R2 = y9 = y8 y1
  emit(OP_MUL, 3, 5, 3);
  emit(OP_MUL, 3, 3, 0);   // R3 = y11 = y8 y4 r
  emit(OP_FROB, 1, 2, 1);
  emit(OP_MUL, 1, 1, 3);   // R1 = y13 = frob1(y9) y11
  emit(OP_FROB, 3, 5, 2);
  emit(OP_MUL, 3, 3, 1);   // R3 = y14 = frob2(y8) y13
  emit(OP_CONJ, 0, 0, 0);
  emit(OP_MUL, 0, 0, 2);
  emit(OP_FROB, 0, 0, 3);  // R0 = y15 = frob3(conj(r) y9)
  emit(OP_MUL, 0, 0, 3);   // R0 = y15 y14
  return p;
}

// ---- the arithmetic on groups -----------------------------------------------------------------------------------------
template <class P, int SCHED>
struct Wave {
  using T = p29::Tower<SCHED>;
  using F = typename T::F;
  using V = typename P::V;
  using g1_eval = typename T::g1_eval;

  // c ? a : b word by word: a choice between two VALUES.  (A conditional between two struct lvalues is a choice between
  // two addresses, and would put both on the stack.)
  static CAP_HD fl pick(bool c, const fl& a, const fl& b) {
    fl r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
  }
  static CAP_HD f2 pick(bool c, const f2& a, const f2& b) { return {pick(c, a.c0, b.c0), pick(c, a.c1, b.c1)}; }

  static CAP_HD V zero() {
    return P::map([](int) { return T::f2_zero(); });
  }
  static CAP_HD V one() {
    return P::map([](int k) { return pick(k == 0, T::f2_one(), T::f2_zero()); });
  }
  static CAP_HD V conj(const V& a) {  // a^(p^6): the odd powers of w change sign
    return P::map([](int k, const f2& x) { return pick(k & 1, T::f2_neg(x), x); }, a);
  }

  // r_k = sum_{i <= k} a_i b_(k-i) + xi sum_{i > k} a_i b_(k-i+6).  Lane k forms its six Fq2 products one after the
  // other: a_i is lane i's value for everybody, b_(k-i) a rotation.  Accumulation: `lo` and `hi` are sums of at most
  // six values, each addition is Tower<>::f2_add (carried and weak-reduced: < 2p after every step), and the closing
  // lo + xi hi is f2_add of a value < 2p and f2_mul_xi's result (< 2p): nothing lazy crosses a lane.
  static CAP_HD V mul(const V& a, const V& b) {
    V lo = zero(), hi = zero();
#pragma unroll 1  // one Fq2 product in the instruction stream (the kernel is code-size bound, not issue bound)
    for (int i = 0; i < kGroup; i++) {
      const V ai = P::from(a, [=](int) { return i; });
      const V bj = P::from(b, [=](int k) { return k >= i ? k - i : k - i + kGroup; });
      const V s = P::map([=](int k, const f2& x, const f2& y, const f2& l, const f2& h) {
        return T::f2_add(pick(i <= k, l, h), T::f2_mul(x, y));
      }, ai, bj, lo, hi);
      lo = P::map([=](int k, const f2& l, const f2& n) { return pick(i <= k, n, l); }, lo, s);
      hi = P::map([=](int k, const f2& h, const f2& n) { return pick(i <= k, h, n); }, hi, s);
    }
    return P::map([](int, const f2& l, const f2& h) { return T::f2_add(l, T::f2_mul_xi(h)); }, lo, hi);
  }
  // The same sum with a_i a_j and a_j a_i taken once (SqSchedule): four Fq2 products per lane.  A doubled product is
  // f2_dbl of a value < 2p (weak-reduced again), an unused slot adds zero; accumulation as in mul().
  template <int TT>
  static CAP_HD void sqr_slot(const V& a, V& lo, V& hi) {
    constexpr SqSchedule S = make_sq_schedule();
    constexpr uint32_t si = S.i[TT], sj = S.j[TT], used = S.used[TT], dbl = S.dbl[TT], wrap = S.wrap[TT];
    const V x = P::from(a, [](int k) { return (int)((si >> (3 * k)) & 7); });
    const V y = P::from(a, [](int k) { return (int)((sj >> (3 * k)) & 7); });
    const V s = P::map([](int k, const f2& u, const f2& v, const f2& l, const f2& h) {
      f2 m = T::f2_mul(u, v);
      const f2 d = T::f2_dbl(m);
      m = pick((dbl >> k) & 1, d, m);
      m = pick((used >> k) & 1, m, T::f2_zero());
      return T::f2_add(pick((wrap >> k) & 1, h, l), m);
    }, x, y, lo, hi);
    lo = P::map([](int k, const f2& l, const f2& n) { return pick((wrap >> k) & 1, l, n); }, lo, s);
    hi = P::map([](int k, const f2& h, const f2& n) { return pick((wrap >> k) & 1, n, h); }, hi, s);
  }
  static CAP_HD V sqr(const V& a) {
    V lo = zero(), hi = zero();
    sqr_slot<0>(a, lo, hi);
    sqr_slot<1>(a, lo, hi);
    sqr_slot<2>(a, lo, hi);
    sqr_slot<3>(a, lo, hi);
    return P::map([](int, const f2& l, const f2& h) { return T::f2_add(l, T::f2_mul_xi(h)); }, lo, hi);
  }
  // f * (s + b0 w + b1 w^3), s in Fq: Tower<>::f12_mul_line's operand read along w.
  //   r_k = s f_k + b0 f_(k-1) [xi for k < 1] + b1 f_(k-3) [xi for k < 3]
  // s, b0, b1 are the same in every lane of the group.  The three terms are products (< 2p, f2_mul / f2_mul_fq / f2_mul_xi
  // results), summed by two f2_add.
  static CAP_HD V mul_line(const V& f, const fl& s, const f2& b0, const f2& b1) {
    const V f1 = P::from(f, [](int k) { return k >= 1 ? k - 1 : k + 5; });
    const V f3 = P::from(f, [](int k) { return k >= 3 ? k - 3 : k + 3; });
    return P::map([=](int k, const f2& x, const f2& x1, const f2& x3) {
      const f2 t1 = T::f2_mul(x1, b0), t3 = T::f2_mul(x3, b1);
      const f2 w1 = T::f2_mul_xi(t1), w3 = T::f2_mul_xi(t3);
      return T::f2_add(T::f2_add(T::f2_mul_fq(x, s), pick(k < 1, w1, t1)), pick(k < 3, w3, t3));
    }, f, f1, f3);
  }
  // a^(p^j), j = 1, 2, 3: lane k's coefficient becomes conj^j(c) xi^(k (p^j - 1)/6)
  static CAP_HD V frob(const V& a, int j) {
    return P::map([=](int k, const f2& x) {
      const f2 c = pick(j & 1, T::f2_conj(x), x);
      const f2 m = T::f2_mul(c, T::f2_konst(PairConst::FROB[j - 1][k ? k - 1 : 0]));
      return pick(k != 0, m, c);
    }, a);
  }
  // Granger-Scott squaring (Tower<>::f12_cyclo_sqr): the three Fq4 squarings (z0 + z1 s)^2, (z2 + z3 s)^2, (z4 + z5 s)^2
  // have their halves in lanes (0, 3), (1, 4), (2, 5).  Lane k < 3 forms (x + y)(x + xi y), lane k + 3 forms t = x y; then
  // lo = that - t - xi t stays in lane k and hi = 2 t in lane k + 3, and one more move brings each t_n to the lane whose
  // coefficient it updates (3 t -+ 2 z; lane 1 takes xi t5).  Every step is a Tower<> operation on values < 2p.
  static CAP_HD V cyclo_sqr(const V& a) {
    const V o = P::from(a, [](int k) { return k >= 3 ? k - 3 : k + 3; });
    const V m = P::map([](int k, const f2& own, const f2& oth) {
      const f2 x = pick(k < 3, own, oth), y = pick(k < 3, oth, own);
      const f2 u = T::f2_add(x, y), v = T::f2_add(T::f2_mul_xi(y), x);
      return T::f2_mul(pick(k < 3, u, x), pick(k < 3, v, y));
    }, a, o);
    const V mo = P::from(m, [](int k) { return k >= 3 ? k - 3 : k + 3; });
    const V h = P::map([](int k, const f2& mine, const f2& t) {
      const f2 lo = T::f2_sub(T::f2_sub(mine, t), T::f2_mul_xi(t)), hi = T::f2_dbl(mine);
      return pick(k < 3, lo, hi);
    }, m, mo);
    // lanes 0..5 hold t0, t2, t4, t1, t3, t5; lane k needs t0, t5, t2, t1, t4, t3
    const V g = P::from(h, [](int k) { return (int)((0x22668u >> (3 * k)) & 7); });  // 0, 5, 1, 3, 2, 4 in 3-bit fields
    return P::map([](int k, const f2& t, const f2& z) {
      const f2 tx = T::f2_mul_xi(t);
      const f2 tt = pick(k == 1, tx, t);
      const f2 dm = T::f2_sub(tt, z), dp = T::f2_add(tt, z);
      return T::f2_add(T::f2_dbl(pick(k & 1, dp, dm)), tt);  // 3t - 2z (even k), 3t + 2z (odd k)
    }, g, a);
  }

  // 1 / a = a^(p - 2) without a window table (Fl::inv keeps 16 powers in an indexed array, i.e. on the stack): 253
  // squarings and the products of the set bits.  a normalized with limbs < 2^30; the result is a product (< 2p).
  static CAP_HD fl inv_bits(const fl& a) {
    fl r = F::one();
#pragma unroll 1
    for (int bit = 253; bit >= 0; bit--) {
      r = F::sqr(r);
      const int limb = bit / 29, off = bit % 29;
      const uint32_t e = FqP29::MOD[limb] - (limb == 0 ? 2u : 0u);  // the lowest limb of p ends in 7: no borrow
      if ((e >> off) & 1) r = F::mul(r, a);
    }
    return r;
  }
  // 1 / n for n in Fq6 (its three Fq2 coefficients in the even lanes; Tower<>::f6_inv).  Every lane forms the cofactors
  // and their norm t in Fq2; lane 0 alone inverts (one Fq inversion per check) and hands 1 / t to the others.
  static CAP_HD V ninv(const V& n) {
    const V n0 = P::from(n, [](int) { return 0; }), n1 = P::from(n, [](int) { return 2; });
    const V n2 = P::from(n, [](int) { return 4; });
    const V c0 = P::map([](int, const f2& x0, const f2& x1, const f2& x2) {
      return T::f2_sub(T::f2_sqr(x0), T::f2_mul_xi(T::f2_mul(x1, x2)));
    }, n0, n1, n2);
    const V c1 = P::map([](int, const f2& x0, const f2& x1, const f2& x2) {
      return T::f2_sub(T::f2_mul_xi(T::f2_sqr(x2)), T::f2_mul(x0, x1));
    }, n0, n1, n2);
    const V c2 = P::map([](int, const f2& x0, const f2& x1, const f2& x2) {
      return T::f2_sub(T::f2_sqr(x1), T::f2_mul(x0, x2));
    }, n0, n1, n2);
    const V t = P::map([](int, const f2& x0, const f2& x1, const f2& x2, const f2& y0, const f2& y1, const f2& y2) {
      return T::f2_add(T::f2_mul(x0, y0), T::f2_mul_xi(T::f2_add(T::f2_mul(x2, y1), T::f2_mul(x1, y2))));
    }, n0, n1, n2, c0, c1, c2);
    const V ti0 = P::map([](int k, const f2& x) {
      if (k != 0) return T::f2_zero();
      // sum of two products (< 1.5p each): normalized, limbs < 2^30, as Tower<>::f2_inv
      const fl d = inv_bits(F::add_norm(F::mul(x.c0, x.c0), F::mul(x.c1, x.c1)));
      return f2{F::mul(x.c0, d), T::neg(F::mul(x.c1, d))};
    }, t);
    const V ti = P::from(ti0, [](int) { return 0; });
    return P::map([](int k, const f2& y0, const f2& y1, const f2& y2, const f2& i) {
      const f2 r = T::f2_mul(pick(k == 0, y0, pick(k == 2, y1, y2)), i);
      return pick(k & 1, T::f2_zero(), r);
    }, c0, c1, c2, ti);
  }

  static CAP_HD uint32_t final_exp_ins(int pc) {
    constexpr Program prog = make_final_exp();
    return prog.ins[pc];
  }
  // f^(m (p^12 - 1)/r) as Tower<>::final_exp (same m, same chain); 0 stays 0
  static CAP_HD V final_exp(const V& f) {
    constexpr int n = make_final_exp().n;
    V R[kRegs];
#pragma unroll
    for (int r = 0; r < kRegs; r++) R[r] = f;
#pragma unroll 1
    for (int pc = 0; pc < n; pc++) {
      const uint32_t ins = final_exp_ins(pc);
      const int op = (int)(ins >> 12), d = (int)((ins >> 8) & 7), a = (int)((ins >> 4) & 7), b = (int)(ins & 7);
      V x = R[0], y = R[0];  // registers are picked by comparison, never by index: they stay registers
#pragma unroll
      for (int r = 1; r < kRegs; r++) {
        if (a == r) x = R[r];
        if (b == r) y = R[r];
      }
      V z = x;
      switch (op) {
        case OP_MUL: z = mul(x, y); break;
        case OP_CSQ: z = cyclo_sqr(x); break;
        case OP_CONJ: z = conj(x); break;
        case OP_FROB: z = frob(x, b); break;
        case OP_NINV: z = ninv(x); break;
        default: break;
      }
#pragma unroll
      for (int r = 0; r < kRegs; r++)
        if (d == r) R[r] = z;
    }
    return R[0];
  }
  static CAP_HD bool is_one(const V& a) {
    return P::all([](int k, const f2& x) {
      return k == 0 ? (F::eq(x.c0, F::one()) && F::is_zero(x.c1)) : T::f2_is_zero(x);
    }, a);
  }

  // ---- Miller loop over prepared lines (Tower<>::miller2: same lines, same order) -----------------------------------
  // p is the same in every lane of the group; `inf` points contribute a factor of 1
  static CAP_HD V mul_prepared(const V& f, const line_coeffs& l, const g1_eval& p) {
    if (p.inf) return f;
    const f2 m = {F::load(l.m0), F::load(l.m1)}, mu = {F::load(l.mu0), F::load(l.mu1)};
    return mul_line(f, p.s, T::f2_mul_fq(m, p.xp), mu);
  }
  // One loop over the kLines steps, so that the kernel holds one squaring and one line product: step idx is the
  // doubling of bit i of 6x + 2 (after a squaring, except for the leading bit), the addition that follows a set bit, or
  // - once the bits are used up - one of the two Frobenius steps.
  static CAP_HD V miller2(const line_coeffs* l1, const g1_eval& p1, const line_coeffs* l2, const g1_eval& p2) {
    V f = one();
    int i = 63;
    bool add_next = false;
#pragma unroll 1
    for (int idx = 0; idx < p29::kLines; idx++) {
      if (!add_next && i >= 0) {
        if (i != 63) f = sqr(f);
        add_next = (PairConst::ATE_LO >> i) & 1;
        i--;
      } else {
        add_next = false;
      }
#pragma unroll 1
      for (int q = 0; q < 2; q++) {
        const g1_eval p = {pick(q != 0, p2.s, p1.s), pick(q != 0, p2.xp, p1.xp), q ? p2.inf : p1.inf};
        f = mul_prepared(f, (q ? l2 : l1)[idx], p);
      }
    }
    return f;
  }
  // e(P1, Q1) e(P2, Q2) == 1.  No shortcut for two points at infinity: the loop then multiplies nothing and the final
  // exponentiation of 1 is 1, so every group of a wavefront runs the same instructions.
  static CAP_HD bool check2(const line_coeffs* l1, const g1_eval& p1, const line_coeffs* l2, const g1_eval& p2) {
    return is_one(final_exp(miller2(l1, p1, l2, p2)));
  }
};

}  // namespace pw
}  // namespace cap
