// Device conformance check: the operation table.  One record = one operation on raw operands (fl = 9 x uint32 limbs as
// they are, so un-normalized lazy inputs can be given exactly); results are raw limbs too.  Two drivers run this table:
// devcheck_host.cpp (g++/clang++, CAP_FL_CHECK on) and devcheck.hip (gfx950, one record per lane, one per quad for the
// quad group).  tests/devcheck_vectors.py generates the records, knows the layouts below and checks the results.
//
// Record layout (uint32 words).  in[0] = op, in[1] = field (0 Fq, 1 Fr), in[2] = multiplication schedule (0, 1),
// in[3] = aux; operands from in[4].  The last word of every output record is kDone + op: a record that was never
// written keeps the driver's 0xFF fill.  An fe operand occupies the first 8 words of a 9-word slot.
//   group      in words                              out words
//   FIELD      4 + 4 fl                       = 40   fl, flag, done                      = 11
//   FIELD32    4 + 3 fe                       = 28   fe, done                            =  9
//   CURVE      4 + g1x A + g1x B + fe k       = 85   g1x, flag, done                     = 38
//   QUAD       4 + g1x A + g1x B              = 76   g1x quad, g1x reloaded, g1x one-lane, flag, done = 110
//   TOWER      4 + f12 A + f12 B              = 220  f12, flag, done                     = 110
//   PAIR       4 + (x, y, inf) x 2 + q1, q2 + f12 = 152   f12, flag, done                = 110
// PAIR records name their G2 points by index into the file's G2 table (kNullQ = a point at infinity: a null line table);
// the drivers prepare the line tables on the host (pairing29.hpp: prepare_lines), as verify_dev.hip does.
#pragma once
#include <stdint.h>

#include "../../cap_amd/csrc/pairing29.hpp"
#include "../../cap_amd/csrc/quad29.hpp"

namespace devcheck {
using namespace cap;

enum Group { G_FIELD = 0, G_FIELD32 = 1, G_CURVE = 2, G_QUAD = 3, G_TOWER = 4, G_PAIR = 5, G_COUNT = 6 };
constexpr uint32_t kInWords[G_COUNT] = {40, 28, 85, 76, 220, 152};
constexpr uint32_t kOutWords[G_COUNT] = {11, 9, 38, 110, 110, 110};
constexpr uint32_t kDone = 0x600d0000u;
constexpr uint32_t kNullQ = 0xffffffffu;
constexpr uint32_t kMagic = 0x4b435644u;  // "DVCK"

// op codes: X(name, code) - tests/devcheck_vectors.py reads these lists
#define DC_FIELD_OPS(X)                                                                                              \
  X(mul, 0) X(sqr, 1) X(add, 2) X(sub, 3) X(weak_reduce, 4) X(canonical, 5) X(is_zero, 6) X(pack_unpack, 7)          \
  X(from_ext, 8) X(to_ext, 9) X(to_mont, 10) X(from_mont, 11) X(mul_add_mul, 12) X(eq, 13) X(inv, 14)                \
  X(mul_shoup, 15) X(shoup_quotient, 16) X(sub8p, 17) X(neg, 18) X(add_norm, 19) X(normalize, 20)                    \
  X(sub_from_lazy, 21) X(sub2p_lazy, 22) X(load, 23) X(pack, 24) X(store, 25) X(sub2p, 26) X(neg_lazy, 27)           \
  X(neg2p_lazy, 28) X(neg4p_lazy, 29) X(sub8p_lazy, 30)
#define DC_FIELD32_OPS(X) X(mul, 0) X(sqr, 1) X(add, 2) X(sub, 3) X(dbl, 4) X(inv, 5) X(pow, 6) X(neg, 7)
#define DC_CURVE_OPS(X)                                                                                              \
  X(from_affine, 0) X(dbl_affine, 1) X(dbl, 2) X(add_mixed, 3) X(madd_acc, 4) X(add_acc, 5) X(add, 6)                \
  X(to_affine, 7) X(store_load, 8) X(term_mul, 9) X(load_affine, 10) X(item_chain, 11) X(fold_chain, 12)
#define DC_QUAD_OPS(X) X(add, 0) X(dbl, 1) X(chain, 2) X(tree, 3)
#define DC_TOWER_OPS(X)                                                                                              \
  X(f2_mul, 0) X(f2_sqr, 1) X(f2_inv, 2) X(f2_mul_xi, 3) X(f6_mul, 4) X(f6_mul_01, 5) X(f6_inv, 6) X(f6_mul_v, 7)    \
  X(f12_mul, 8) X(f12_sqr, 9) X(f12_inv, 10) X(f12_conj, 11) X(f12_frob, 12) X(f12_mul_line, 13)                     \
  X(f12_cyclo_sqr, 14) X(f12_exp_x, 15) X(final_exp, 16)
#define DC_PAIR_OPS(X) X(mul_prepared, 0) X(miller2, 1) X(check2, 2) X(pairing2, 3)
#define DC_ENUM(name, code) name = code,
namespace fop { enum { DC_FIELD_OPS(DC_ENUM) }; }
namespace f32op { enum { DC_FIELD32_OPS(DC_ENUM) }; }
namespace cop { enum { DC_CURVE_OPS(DC_ENUM) }; }
namespace qop { enum { DC_QUAD_OPS(DC_ENUM) }; }
namespace top { enum { DC_TOWER_OPS(DC_ENUM) }; }
namespace pop { enum { DC_PAIR_OPS(DC_ENUM) }; }
#undef DC_ENUM

// ---- raw operands ----------------------------------------------------------------------------------------------------
static CAP_HD fl rd_fl(const uint32_t* w) {
  fl r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = w[i];
  return r;
}
static CAP_HD fe rd_fe(const uint32_t* w) {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = w[i];
  return r;
}
static CAP_HD void wr_fl(uint32_t* w, const fl& a) {
#pragma unroll
  for (int i = 0; i < 9; i++) w[i] = a.v[i];
}
static CAP_HD void wr_fe(uint32_t* w, const fe& a) {  // the ninth word of the slot is 0
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = a.v[i];
  w[8] = 0;
}
static CAP_HD g1x rd_g1x(const uint32_t* w) {
  g1x r;
  r.x = rd_fl(w);
  r.y = rd_fl(w + 9);
  r.zz = rd_fl(w + 18);
  r.zzz = rd_fl(w + 27);
  return r;
}
static CAP_HD void wr_g1x(uint32_t* w, const g1x& p) {
  wr_fl(w, p.x);
  wr_fl(w + 9, p.y);
  wr_fl(w + 18, p.zz);
  wr_fl(w + 27, p.zzz);
}
// f2 / f6 / f12 are 2 / 6 / 12 fl in struct order: (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2), each (c0, c1)
static CAP_HD p29::f2 rd_f2(const uint32_t* w) { return {rd_fl(w), rd_fl(w + 9)}; }
static CAP_HD p29::f6 rd_f6(const uint32_t* w) { return {rd_f2(w), rd_f2(w + 18), rd_f2(w + 36)}; }
static CAP_HD p29::f12 rd_f12(const uint32_t* w) { return {rd_f6(w), rd_f6(w + 54)}; }
static CAP_HD void wr_f2(uint32_t* w, const p29::f2& a) {
  wr_fl(w, a.c0);
  wr_fl(w + 9, a.c1);
}
static CAP_HD void wr_f6(uint32_t* w, const p29::f6& a) {
  wr_f2(w, a.c0);
  wr_f2(w + 18, a.c1);
  wr_f2(w + 36, a.c2);
}
static CAP_HD void wr_f12(uint32_t* w, const p29::f12& a) {
  wr_f6(w, a.c0);
  wr_f6(w + 54, a.c1);
}
static CAP_HD void zero_words(uint32_t* w, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) w[i] = 0;
}

// ---- deliberately wrong variants (host only, -DDEVCHECK_MUTANT=n): the checker must flag each in its own op -------
#ifndef DEVCHECK_MUTANT
#define DEVCHECK_MUTANT 0
#endif
#if DEVCHECK_MUTANT && (defined(__HIPCC__) || defined(__HIP__))
#error "mutants are host builds only"
#endif

// ---- FIELD --------------------------------------------------------------------------------------------------------------
template <class PR, int S>
static CAP_HD void field_ops(uint32_t op, const uint32_t* in, uint32_t* out) {
  using F = Fl<PR, S>;
  const fl a = rd_fl(in + 4), b = rd_fl(in + 13), c = rd_fl(in + 22), d = rd_fl(in + 31);
  fl r = F::zero();
  uint32_t flag = 0;
  bool is_fe = false;
  fe rf;
  switch (op) {
    case fop::mul: r = F::mul(a, b); break;
    case fop::sqr: r = F::sqr(a); break;
    case fop::add: r = F::add(a, b); break;
    case fop::sub: r = F::sub(a, b); break;
    case fop::weak_reduce: r = F::weak_reduce(a); break;
    case fop::canonical: r = F::canonical(a); break;
    case fop::is_zero: flag = F::is_zero(a) ? 1 : 0; break;
    case fop::pack_unpack: r = F::unpack(F::pack(a)); break;
    case fop::from_ext: r = F::from_ext(rd_fe(in + 4)); break;
    case fop::to_ext: rf = F::to_ext(a), is_fe = true; break;
    case fop::to_mont: r = F::to_mont(rd_fe(in + 4)); break;
    case fop::from_mont: rf = F::from_mont(a), is_fe = true; break;
    case fop::mul_add_mul: r = F::mul_add_mul(a, b, c, d); break;
    case fop::eq: flag = F::eq(a, b) ? 1 : 0; break;
    case fop::inv: r = F::inv(a); break;
    case fop::mul_shoup: r = F::mul_shoup(a, b, F::shoup_quotient(F::canonical(F::to_mont(F::pack(b))))); break;
    case fop::shoup_quotient: r = F::shoup_quotient(a); break;
    case fop::sub8p: r = F::sub8p(a, b); break;
    case fop::neg: r = F::neg(a); break;
    case fop::add_norm: r = F::add_norm(a, b); break;
    case fop::normalize: r = F::normalize(a); break;
    case fop::sub_from_lazy: r = F::sub_from_lazy(a, b); break;
    case fop::sub2p_lazy: r = F::sub2p_lazy(a, b); break;
    case fop::load: r = F::load(rd_fe(in + 4)); break;
    case fop::pack: rf = F::pack(a), is_fe = true; break;
    case fop::store: rf = F::store(a), is_fe = true; break;
    case fop::sub2p: r = F::sub2p(a, b); break;
    case fop::neg_lazy: r = F::neg_lazy(a); break;
    case fop::neg2p_lazy: r = F::neg2p_lazy(a); break;
    case fop::neg4p_lazy: r = F::neg4p_lazy(a); break;
    case fop::sub8p_lazy: r = F::sub8p_lazy(a, b); break;
    default: return;  // unknown op: the record keeps its fill
  }
  if (is_fe) wr_fe(out, rf);
  else wr_fl(out, r);
  out[9] = flag;
  out[10] = kDone + op;
}
static CAP_HD void run_field(const uint32_t* in, uint32_t* out) {
  const uint32_t op = in[0], sel = (in[1] & 1) * 2 + (in[2] & 1);
  if (in[1] > 1 || in[2] > 1) return;
  switch (sel) {
    case 0: field_ops<FqP29, 0>(op, in, out); break;
    case 1: field_ops<FqP29, 1>(op, in, out); break;
    case 2: field_ops<FrP29, 0>(op, in, out); break;
    default: field_ops<FrP29, 1>(op, in, out); break;
  }
}

// ---- FIELD32: the saturated field as the device runs it (CIOS mul_inline, Fermat inverse) ------------------------------
// (a host build takes the same forms when compiled with -DCAP_HOST_MUL32; without it, the host's 64-bit-limb forms)
template <class F>
static CAP_HD void field32_ops(uint32_t op, const uint32_t* in, uint32_t* out) {
  const fe a = rd_fe(in + 4), b = rd_fe(in + 12), e = rd_fe(in + 20);
  fe r;
  switch (op) {
    case f32op::mul: r = F::mul(a, b); break;
    case f32op::sqr: r = F::sqr(a); break;
    case f32op::add: r = F::add(a, b); break;
    case f32op::sub: r = F::sub(a, b); break;
    case f32op::dbl: r = F::dbl(a); break;
    case f32op::inv: r = F::inv(a); break;
    case f32op::pow: r = F::pow(a, e.v); break;
    case f32op::neg: r = F::neg(a); break;
    default: return;
  }
  for (int i = 0; i < 8; i++) out[i] = r.v[i];
  out[8] = kDone + op;
}
static CAP_HD void run_field32(const uint32_t* in, uint32_t* out) {
  if (in[1] == 0) field32_ops<Fq>(in[0], in, out);
  else if (in[1] == 1) field32_ops<Fr>(in[0], in, out);
}

// ---- CURVE --------------------------------------------------------------------------------------------------------------
template <int S>
struct CurveOps {
  using G = G1LT<S>;
  using F = typename G::F;
#if DEVCHECK_MUTANT == 2
  // mutant: a mixed addition that skips the equal-operand path (acc == q gives infinity instead of the doubling)
  static g1x add_mixed(const g1x& a, const g1a& q_in, bool negate) {
    if (G::is_inf(q_in)) return a;
    g1a q = q_in;
    if (negate) q.y = F::neg(q.y);
    if (!G::is_inf(a) && F::is_zero(F::sub(F::mul(q.x, a.zz), a.x))) return G::inf();
    return G::add_mixed(a, q_in, negate);
  }
#else
  static CAP_HD g1x add_mixed(const g1x& a, const g1a& q, bool negate) { return G::add_mixed(a, q, negate); }
#endif
#if DEVCHECK_MUTANT == 3
  // mutant: the scalar multiplication drops the top digit when the top bit sits at an even position
  static g1x term_mul(const g1a& b, const fe& k) {
    int top = -1;
    for (int i = 7; i >= 0 && top < 0; i--)
      if (k.v[i]) top = 32 * i + G::top_bit(k.v[i]);
    if (top < 0 || (top & 1)) return G::term_mul(b, k);
    fe k2 = k;
    k2.v[top >> 5] &= ~(1u << (top & 31));
    return G::term_mul(b, k2);
  }
#else
  static CAP_HD g1x term_mul(const g1a& b, const fe& k) { return G::term_mul(b, k); }
#endif
  static CAP_HD void run(uint32_t op, const uint32_t* in, uint32_t* out) {
    g1x A = rd_g1x(in + 4);
    const g1x B = rd_g1x(in + 40);
    g1a q;
    q.x = B.x;
    q.y = B.y;
    const bool neg = in[3] & 1;
    g1x r = G::inf();
    uint32_t flag = 0;
    switch (op) {
      case cop::from_affine: r = G::from_affine(q); break;
      case cop::dbl_affine: r = G::dbl_affine(q); break;
      case cop::dbl: r = G::dbl(A); break;
      case cop::add_mixed: r = add_mixed(A, q, neg); break;
      case cop::madd_acc: flag = G::madd_acc(A, q, neg) ? 1 : 0, r = A; break;
      case cop::add_acc: flag = G::add_acc(A, B) ? 1 : 0, r = A; break;
      case cop::add: r = G::add(A, B); break;
      case cop::to_affine: {
        const g1a t = G::to_affine(A);
        r.x = t.x;
        r.y = t.y;
        break;
      }
      case cop::store_load: r = G::load(G::store(A)); break;
      case cop::term_mul: r = term_mul(q, rd_fe(in + 76)); break;
      case cop::load_affine: {
        g1_affine m;
        m.x = rd_fe(in + 4);
        m.y = rd_fe(in + 13);
        const g1a t = G::load(m);
        r.x = t.x;
        r.y = t.y;
        flag = G::is_inf(t) ? 1 : 0;
        break;
      }
      case cop::item_chain: {
        // an item of msm_accumulate: add_affine_pair, six madd_acc with the signs of aux (bit i: entry i), store, load.
        // The four table points are (A.x, A.y), (A.zz, A.zzz), (B.x, B.y), (B.zz, B.zzz), taken in turn.
        const g1a t[4] = {{A.x, A.y}, {A.zz, A.zzz}, {B.x, B.y}, {B.zz, B.zzz}};
        const uint32_t sg = in[3];
        g1x acc = G::inf();
        bool ok = G::add_affine_pair(acc, t[0], (sg & 1) != 0, t[1], (sg & 2) != 0);
        for (int i = 2; i < 8; i++) ok = G::madd_acc(acc, t[i & 3], ((sg >> i) & 1) != 0) && ok;
        flag = ok ? 1 : 0;
        r = G::load(G::store(acc));
        break;
      }
      case cop::fold_chain: {
        // a fold of the reductions: (A + B) + A by add_acc twice, doubled, handed out as the C ABI's Jacobian triple
        // (x, y, z in the first three slots, 8 words each)
        g1x acc = A;
        bool ok = G::add_acc(acc, B);
        ok = G::add_acc(acc, A) && ok;
        const g1_jac j = G::to_jac_ext(G::dbl(acc));
        flag = ok ? 1 : 0;
        zero_words(out, 36);
        wr_fe(out, j.x);
        wr_fe(out + 9, j.y);
        wr_fe(out + 18, j.z);
        out[36] = flag;
        out[37] = kDone + op;
        return;
      }
      default: return;
    }
    wr_g1x(out, r);
    out[36] = flag;
    out[37] = kDone + op;
  }
};
static CAP_HD void run_curve(const uint32_t* in, uint32_t* out) {
  if (in[2] == 0) CurveOps<0>::run(in[0], in, out);
  else if (in[2] == 1) CurveOps<1>::run(in[0], in, out);
}

// ---- QUAD: one record per quad; P is the lane policy (QuadDev: four real lanes; QuadSim: four simulated ones) --------
// Every lane of the quad runs this with the same record; `writer` is true in one of them.
template <int S, class P, class Slow>
static CAP_HD void quad_ops(const uint32_t* in, uint32_t* out, Slow slow, bool writer) {
  using G = G1LT<S>;
  using Q = QuadG1<G, P>;
  using V = typename P::V;
  const uint32_t op = in[0];
  const g1x A = rd_g1x(in + 4), B = rd_g1x(in + 40);
  V a = Q::scatter(A);
  const V b = Q::scatter(B);
  g1x one = G::inf();  // the same sum by the one-lane code
  switch (op) {
    case qop::add:
      Q::add(a, b, slow);
      one = G::add(A, B);
      break;
    case qop::dbl:
      Q::dbl(a);
      one = G::dbl(A);
      break;
    case qop::chain:  // results fed back, a doubling and the memory image in between: 2 (A + B) + B + A
      Q::add(a, b, slow);
      Q::dbl(a);
      a = Q::scatter(G::load(G::store(Q::gather(a))));
      Q::add(a, b, slow);
      Q::add(a, Q::scatter(A), slow);
      one = G::add(G::add(G::dbl(G::add(A, B)), B), A);
      break;
    case qop::tree: {  // (A + 2A) + (B + 2B): both operands of the last addition are quad results
      V t2 = a, t3 = b, t1 = b;
      Q::dbl(t2);
      Q::dbl(t3);
      Q::add(a, t2, slow);
      Q::add(t1, t3, slow);
      Q::add(a, t1, slow);
      one = G::add(G::add(A, G::dbl(A)), G::add(B, G::dbl(B)));
      break;
    }
    default: return;
  }
  const g1x res = Q::gather(a);
  const g1x back = Q::gather(Q::scatter(G::load(G::store(res))));
  if (!writer) return;
  wr_g1x(out, res);
  wr_g1x(out + 36, back);
  wr_g1x(out + 72, one);
  out[108] = G::is_inf(res) ? 1 : 0;
  out[109] = kDone + op;
}

// ---- TOWER --------------------------------------------------------------------------------------------------------------
template <int S>
struct TowerOps {
  using T = p29::Tower<S>;
  using F = typename T::F;
#if DEVCHECK_MUTANT == 1
  // mutant: an Fq2 product whose second coefficient misses its final weak reduction
  static p29::f2 f2_mul(const p29::f2& a, const p29::f2& b) {
    const fl t0 = F::mul(a.c0, b.c0), t1 = F::mul(a.c1, b.c1);
    const fl s = F::mul(F::add(a.c0, a.c1), F::add(b.c0, b.c1));
    return {T::sub(t0, t1), F::sub(F::sub(s, t0), t1)};
  }
#else
  static CAP_HD p29::f2 f2_mul(const p29::f2& a, const p29::f2& b) { return T::f2_mul(a, b); }
#endif
#if DEVCHECK_MUTANT == 5
  // mutant: a Frobenius map that takes its constants from the wrong row
  static p29::f12 f12_frob(const p29::f12& a, int j) {
    p29::f12 r = T::f12_frob(a, j);
    const p29::f2 x = (j & 1) ? T::f2_conj(a.c1.c0) : a.c1.c0;
    r.c1.c0 = T::f2_mul(x, T::f2_konst(p29::PairConst::FROB[j % 3][0]));  // row j + 1 instead of row j
    return r;
  }
#else
  static CAP_HD p29::f12 f12_frob(const p29::f12& a, int j) { return T::f12_frob(a, j); }
#endif
  static CAP_HD void run(uint32_t op, const uint32_t* in, uint32_t* out) {
    const uint32_t* pa = in + 4;
    const uint32_t* pb = in + 112;
    zero_words(out, 108);
    switch (op) {
      case top::f2_mul: wr_f2(out, f2_mul(rd_f2(pa), rd_f2(pb))); break;
      case top::f2_sqr: wr_f2(out, T::f2_sqr(rd_f2(pa))); break;
      case top::f2_inv: wr_f2(out, T::f2_inv(rd_f2(pa))); break;
      case top::f2_mul_xi: wr_f2(out, T::f2_mul_xi(rd_f2(pa))); break;
      case top::f6_mul: wr_f6(out, T::f6_mul(rd_f6(pa), rd_f6(pb))); break;
      case top::f6_mul_01: wr_f6(out, T::f6_mul_01(rd_f6(pa), rd_f2(pb), rd_f2(pb + 18))); break;
      case top::f6_inv: wr_f6(out, T::f6_inv(rd_f6(pa))); break;
      case top::f6_mul_v: wr_f6(out, T::f6_mul_v(rd_f6(pa))); break;
      case top::f12_mul: wr_f12(out, T::f12_mul(rd_f12(pa), rd_f12(pb))); break;
      case top::f12_sqr: wr_f12(out, T::f12_sqr(rd_f12(pa))); break;
      case top::f12_inv: wr_f12(out, T::f12_inv(rd_f12(pa))); break;
      case top::f12_conj: wr_f12(out, T::f12_conj(rd_f12(pa))); break;
      case top::f12_frob:
        if (in[3] < 1 || in[3] > 3) return;
        wr_f12(out, f12_frob(rd_f12(pa), (int)in[3]));
        break;
      case top::f12_mul_line: wr_f12(out, T::f12_mul_line(rd_f12(pa), rd_fl(pb), rd_f2(pb + 9), rd_f2(pb + 27))); break;
      case top::f12_cyclo_sqr: wr_f12(out, T::f12_cyclo_sqr(rd_f12(pa))); break;
      case top::f12_exp_x: wr_f12(out, T::f12_exp_x(rd_f12(pa))); break;
      case top::final_exp: wr_f12(out, T::final_exp(rd_f12(pa))); break;
      default: return;
    }
    out[108] = 0;
    out[109] = kDone + op;
  }
};
static CAP_HD void run_tower(const uint32_t* in, uint32_t* out) {
  if (in[2] == 0) TowerOps<0>::run(in[0], in, out);
  else if (in[2] == 1) TowerOps<1>::run(in[0], in, out);
}

// ---- PAIR ---------------------------------------------------------------------------------------------------------------
// lines: the prepared tables of the file's G2 points, kLines entries each; nq: how many (indices are checked here)
template <int S>
struct PairOps {
  using T = p29::Tower<S>;
#if DEVCHECK_MUTANT == 4
  // mutant: a Miller loop that leaves out its last Frobenius line
  static p29::f12 miller2(const p29::line_coeffs* l1, const typename T::g1_eval& p1, const p29::line_coeffs* l2,
                          const typename T::g1_eval& p2) {
    p29::f12 f = T::f12_one();
    int idx = 0;
    for (int i = 63; i >= 0; i--) {
      if (i != 63) f = T::f12_sqr(f);
      for (int k = 0; k < 1 + (int)((p29::PairConst::ATE_LO >> i) & 1); k++, idx++) {
        f = T::mul_prepared(f, l1[idx], p1);
        f = T::mul_prepared(f, l2[idx], p2);
      }
    }
    f = T::mul_prepared(f, l1[idx], p1);
    return T::mul_prepared(f, l2[idx], p2);
  }
#else
  static CAP_HD p29::f12 miller2(const p29::line_coeffs* l1, const typename T::g1_eval& p1,
                                 const p29::line_coeffs* l2, const typename T::g1_eval& p2) {
    return T::miller2(l1, p1, l2, p2);
  }
#endif
  static CAP_HD void run(uint32_t op, const uint32_t* in, uint32_t* out, const p29::line_coeffs* lines, uint32_t nq) {
    const uint32_t q1 = in[42], q2 = in[43];
    if ((q1 != kNullQ && q1 >= nq) || (q2 != kNullQ && q2 >= nq)) return;
    const p29::line_coeffs* l1 = q1 == kNullQ ? nullptr : lines + (size_t)q1 * p29::kLines;
    const p29::line_coeffs* l2 = q2 == kNullQ ? nullptr : lines + (size_t)q2 * p29::kLines;
    // as k_pairing_check2: a null table stands for Q at infinity, its pair is a factor of 1
    const typename T::g1_eval e1 = T::eval_point(rd_fl(in + 4), rd_fl(in + 13), !l1 || in[22] != 0);
    const typename T::g1_eval e2 = T::eval_point(rd_fl(in + 23), rd_fl(in + 32), !l2 || in[41] != 0);
    const p29::line_coeffs* t1 = l1 ? l1 : l2;
    const p29::line_coeffs* t2 = l2 ? l2 : l1;
    zero_words(out, 109);
    switch (op) {
      case pop::mul_prepared:
        if (!l1 || in[3] >= (uint32_t)p29::kLines) return;
        wr_f12(out, T::mul_prepared(rd_f12(in + 44), l1[in[3]], e1));
        break;
      case pop::miller2:
        if (!t1) return;
        wr_f12(out, miller2(t1, e1, t2, e2));
        break;
      case pop::check2:
        if (!t1 && !(e1.inf && e2.inf)) return;
        out[108] = T::check2(t1, e1, t2, e2) ? 1 : 0;
        break;
      case pop::pairing2:
        if (!t1) return;
        wr_f12(out, T::final_exp(miller2(t1, e1, t2, e2)));
        break;
      default: return;
    }
    out[109] = kDone + op;
  }
};
static CAP_HD void run_pair(const uint32_t* in, uint32_t* out, const p29::line_coeffs* lines, uint32_t nq) {
  if (in[2] == 0) PairOps<0>::run(in[0], in, out, lines, nq);
  else if (in[2] == 1) PairOps<1>::run(in[0], in, out, lines, nq);
}

}  // namespace devcheck
