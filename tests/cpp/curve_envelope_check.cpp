// The G1 group law of cap_amd/csrc/curve29.hpp (G1Law<F, V>) on the bound-tracking field (bound29.hpp, bound_curve29.hpp):
// every operation and every chain the kernels build from them, for ALL inputs of the classes the headers name.  Driven by
// tests/test_curve_envelope_host.py:
//   curve_envelope_check envelope [CONTROL]   the bounds of every result as JSON (the "curve" section of
//                                             tests/golden/lazy_envelope.json); exit code 2 and the violated operation on
//                                             stderr if a precondition fails or a result leaves the class its comment names.
//                                             CONTROL - what the check exists to catch, the driver expects exit code 2:
//                                               y17      class A widened to y < 17p
//                                               noweak   the accumulate chain restated without the weak_reduce on o.x
//   curve_envelope_check ops                  "op sched operand.." lines on stdin: is_zero, eq, inv, and the lazy forms of
//                                             mul and mul_add_mul - the real operation next to the bound one
//   curve_envelope_check run SCHED            concrete operands on stdin through the real G1LT<SCHED> with the bound
//                                             assertions of field29.hpp on (layouts at run_rows)
//
// The classes are the headers' words, fixed here as constants (units of p / 2^20):
//   T  table point in memory (g1_affine): canonical
//   R  register point of the general law: x, y normalized < 2p; zz, zzz normalized < 1.1p
//   A  accumulator of the lean forms (madd_acc, add_affine_pair, add_acc): x < 2p, y < 3p, zz, zzz < 1.2p, normalized
//   M  bucket point in memory (g1_xyzz): what store writes, and "any value < 2^256"
#define CAP_FL_CHECK 1
#include "bound_curve29.hpp"

#include "../../cap_amd/csrc/lagrange_elem29.hpp"
#include "../../cap_amd/csrc/quad29.hpp"

#include <algorithm>
#include <string>
#include <vector>

using namespace cap;
using capbound::bfe;
using capbound::bfl;
using capbound::bg1_affine;
using capbound::bg1_jac;
using capbound::bg1_xyzz;
using capbound::bg1a;
using capbound::bg1x;
using capbound::BoundBranch;
using capbound::BoundLog;
using BF = capbound::BoundFl<FqP29>;
using G = G1Law<BF, bfl>;
static constexpr uint64_t U = BF::U;

struct Cls {  // magnitudes of x, y, zz, zzz
  const char* name;
  uint64_t x, y, zz, zzz;
};
static const Cls CLS_T = {"T", U, U, U, U};
static const Cls CLS_R = {"R", 2 * U, 2 * U, U * 11 / 10, U * 11 / 10};
static Cls CLS_A = {"A", 2 * U, 3 * U, U * 12 / 10, U * 12 / 10};  // (the controls widen it)
static const Cls CLS_M = {"M", BF::C256 + 1, BF::C256 + 1, BF::C256 + 1, BF::C256 + 1};

static bg1x pt(const Cls& c) {
  bg1x r;
  r.x = BF::norm_of(c.x);
  r.y = BF::norm_of(c.y);
  r.zz = BF::norm_of(c.zz);
  r.zzz = BF::norm_of(c.zzz);
  return r;
}
static bg1_affine table_point() { return bg1_affine{BF::image(U), BF::image(U)}; }
static bg1_xyzz any_bucket() { return bg1_xyzz{BF::image_256(), BF::image_256(), BF::image_256(), BF::image_256()}; }
static bool fits(const bfl& a, uint64_t mag) { return a.zero || (BF::normalized(a) && a.mag <= mag); }
static void require_class(const bg1x& p, const Cls& c, const char* op) {
  CAP_BOUND_REQUIRE(fits(p.x, c.x), op);
  CAP_BOUND_REQUIRE(fits(p.y, c.y), op);
  CAP_BOUND_REQUIRE(fits(p.zz, c.zz), op);
  CAP_BOUND_REQUIRE(fits(p.zzz, c.zzz), op);
}
static bg1x join(const bg1x& a, const bg1x& b) {
  return bg1x{BF::join(a.x, b.x), BF::join(a.y, b.y), BF::join(a.zz, b.zz), BF::join(a.zzz, b.zzz)};
}
static bool same(const bfl& a, const bfl& b) { return a.lo == b.lo && a.hi == b.hi && a.mag == b.mag && a.zero == b.zero; }
static bool same(const bg1x& a, const bg1x& b) {
  return same(a.x, b.x) && same(a.y, b.y) && same(a.zz, b.zz) && same(a.zzz, b.zzz);
}

// ---- the table --------------------------------------------------------------------------------------------------
static std::string g_json;
static bool g_first = true;
static void open_section(const char* name) {
  g_json += std::string(g_json.empty() || g_json.back() == '{' ? "" : ", ") + "\"" + name + "\": {";
  g_first = true;
}
static void close_section() { g_json += "}"; }
static std::string coord(const char* n, const bfl& a) {
  char buf[128];
  snprintf(buf, sizeof buf, "\"%s\": [%llu, %llu]", n, (unsigned long long)BF::lim(a), (unsigned long long)a.mag);
  return buf;
}
static void entry(const std::string& name, const std::string& body) {
  g_json += std::string(g_first ? "" : ", ") + "\"" + name + "\": {" + body + "}";
  g_first = false;
}
static void rec(const std::string& name, const bg1x& p, const Cls* cls) {  // [largest limb, magnitude] per coordinate
  if (cls) require_class(p, *cls, name.c_str());
  entry(name, coord("x", p.x) + ", " + coord("y", p.y) + ", " + coord("zz", p.zz) + ", " + coord("zzz", p.zzz));
}
static void rec(const std::string& name, const bg1a& p, uint64_t mag) {
  CAP_BOUND_REQUIRE(fits(p.x, mag) && fits(p.y, mag), name.c_str());
  entry(name, coord("x", p.x) + ", " + coord("y", p.y));
}
static std::string image(const char* n, const bfe& a) {
  return std::string("\"") + n + "\": " + std::to_string((unsigned long long)a.mag);
}
static void rec(const std::string& name, const bg1_xyzz& m, uint64_t mag) {
  CAP_BOUND_REQUIRE(m.x.mag <= mag && m.y.mag <= mag && m.zz.mag <= mag && m.zzz.mag <= mag, name.c_str());
  entry(name, image("x", m.x) + ", " + image("y", m.y) + ", " + image("zz", m.zz) + ", " + image("zzz", m.zzz));
}
static void rec(const std::string& name, const bg1_jac& m) {  // the C ABI: canonical
  CAP_BOUND_REQUIRE(m.x.mag <= U && m.y.mag <= U && m.z.mag <= U, name.c_str());
  entry(name, image("x", m.x) + ", " + image("y", m.y) + ", " + image("z", m.z));
}
struct At {  // names the operation in every message below it
  explicit At(const char* w, uint32_t plan = 0) {
    BoundLog::where() = w;
    BoundBranch::reset(plan);
  }
};

// ---- operations, every path ----------------------------------------------------------------------------------
// The zero tests of a function are answered by a plan (bound29.hpp: BoundBranch): 0 the common path; bit 0 the
// x-difference vanishes; bits 0 and 1 both differences vanish (a doubling).
static bg1x add_mixed_all(const bg1x& a, const bg1a& q, const char* w) {  // every path and both signs, joined
  bg1x out = G::inf();
  for (int neg = 0; neg < 2; neg++)
    for (uint32_t plan : {0u, 1u, 3u}) {
      At at(w, plan);
      out = join(out, G::add_mixed(a, q, neg != 0));
    }
  return out;
}
static bg1x add_all(const bg1x& a, const bg1x& b, const char* w) {
  bg1x out = G::inf();
  for (uint32_t plan : {0u, 1u, 3u}) {
    At at(w, plan);
    out = join(out, G::add(a, b));
  }
  return out;
}
// add_tree of msm.hip: skip, copy, the lean addition, or the general one when it refuses
static bg1x add_tree_all(const bg1x& a, const bg1x& b, const char* w) {
  bg1x out = join(a, b);
  {
    At at(w);
    bg1x s = a;
    if (G::add_acc(s, b)) out = join(out, s);
  }
  for (uint32_t plan : {1u, 3u}) {  // add_acc refused: the same difference vanishes in add()
    At at(w, plan);
    out = join(out, G::add(a, b));
  }
  return join(out, add_all(a, b, w));
}

// the body of madd_acc once more, so that a carry can be left out of it (WEAK = false): what the envelope exists to
// catch.  With WEAK it must agree with G::madd_acc bound for bound (checked in the table run).
template <bool WEAK>
static bool madd_acc_restated(bg1x& a, const bg1a& q, bool negate) {
  using F = BF;
  const bfl qy = negate ? F::neg_lazy(q.y) : q.y;
  const bfl u2 = F::mul(q.x, a.zz);
  const bfl s2 = F::mul(qy, a.zzz);
  const bfl p = F::sub(u2, a.x);
  if (F::is_zero(p)) return false;
  const bfl r = F::sub(s2, a.y);
  const bfl pp = F::sqr(p);
  const bfl ppp = F::mul(p, pp);
  const bfl qq = F::mul(a.x, pp);
  bg1x o;
  const bfl x3 = F::sub_from_lazy(F::sub2p_lazy(F::sqr(r), ppp), F::add(qq, qq));
  o.x = WEAK ? F::weak_reduce(x3) : x3;
  o.y = F::mul_add_mul(r, F::sub2p_lazy(qq, o.x), F::neg4p_lazy(a.y), ppp);
  o.zz = F::mul(a.zz, pp);
  o.zzz = F::mul(a.zzz, ppp);
  a = o;
  return true;
}

// ---- chains: one function per kernel body, run to the fixed point of the class ---------------------------------------
template <class Step>
static bg1x fixed_point(bg1x c, Step step, const char* w) {
  for (int it = 0; it < 64; it++) {
    const bg1x n = join(c, step(c));
    if (same(n, c)) return c;
    c = n;
  }
  CAP_BOUND_REQUIRE(!"the class keeps growing", w);
  return c;
}
// msm_accumulate: the item starts at infinity or with add_affine_pair; every further entry goes through madd_acc or,
// at any step, through add_mixed (a table point at infinity, the accumulator at infinity, acc == +-q)
template <bool WEAK>
static bg1x chain_accumulate(const Cls& acc_class, bg1_xyzz* stored) {
  const char* w = "msm_accumulate";
  const bg1a t = G::load(table_point());
  bg1x start = add_mixed_all(G::inf(), t, w);
  for (int s = 0; s < 4; s++) {
    At at(w);
    bg1x o = G::inf();
    if (G::add_affine_pair(o, t, (s & 1) != 0, t, (s & 2) != 0)) start = join(start, o);
  }
  const bg1x acc = fixed_point(start, [&](const bg1x& c) {
    require_class(c, acc_class, "msm_accumulate: acc");
    bg1x n = add_mixed_all(c, t, w);
    for (int neg = 0; neg < 2; neg++) {
      At at(w);
      bg1x a = c;
      if (madd_acc_restated<WEAK>(a, t, neg != 0)) n = join(n, a);
      At again(w);
      bg1x b = c;
      if (WEAK && G::madd_acc(b, t, neg != 0)) CAP_BOUND_REQUIRE(same(a, b), "madd_acc restated");
    }
    return n;
  }, w);
  At at(w);
  *stored = G::store(acc);
  return acc;
}
// msm_reduce_segments: S = T = the top bucket, then S += c, T += S per bucket - skip, copy, add_acc, or add
static void chain_segments(const bg1_xyzz& bucket, bg1x* S_out, bg1x* T_out, bg1_xyzz* stored) {
  const char* w = "msm_reduce_segments";
  const bg1x c = G::load(bucket);
  bg1x S = c, T = c;
  for (int it = 0;; it++) {
    const bg1x S2 = join(S, add_tree_all(S, c, w));
    const bg1x T2 = join(T, add_tree_all(T, S2, w));
    if (same(S2, S) && same(T2, T)) break;
    S = S2;
    T = T2;
    if (it == 64) {
      CAP_BOUND_REQUIRE(!"the class keeps growing", w);
      break;
    }
  }
  At at(w);
  *stored = G::store(join(S, T));
  *S_out = S;
  *T_out = T;
}
// wave_sum / add_tree / mul_small and the folds built from them (msm_reduce_final, msm_reduce_grid*, msm_reduce_bits*,
// msm_combine*, msm_sum_parts, msm_var_horner): points loaded from bucket memory, summed with add_tree and add, doubled
// (mul_small, the window Horner), stored and loaded again in any order - the closure of that set
static bg1x chain_fold(const bg1_xyzz& bucket, bg1_xyzz* stored, bg1_jac* out) {
  const char* w = "folds";
  const bg1x x = fixed_point(G::load(bucket), [&](const bg1x& c) {
    bg1x n = join(add_tree_all(c, c, w), add_all(c, c, w));
    At at(w);
    n = join(n, G::dbl(c));
    return join(n, G::load(G::store(c)));
  }, w);
  At at(w);
  *stored = G::store(x);
  *out = G::to_jac_ext(x);
  return x;
}
// msm_precompute_kernel: a caller's base (two from_ext products, made canonical) is stored as a table row, then doubled
// window by window; every window's point goes through to_affine and store_affine and is read back as a table point
static bg1a chain_precompute(bg1_affine* row) {
  const char* w = "msm_precompute_kernel";
  At at(w);
  const bfe any = BF::image_256();
  const bg1a p = bg1a{BF::canonical(BF::from_ext(any)), BF::canonical(BF::from_ext(any))};
  *row = G::store_affine(p);
  const bg1x acc = fixed_point(G::from_affine(p), [&](const bg1x& c) {
    At at2(w);
    return G::dbl(c);
  }, w);
  At at3(w);
  const bg1_affine m = G::store_affine(G::to_affine(acc));
  row->x.mag = std::max(row->x.mag, m.x.mag);
  row->y.mag = std::max(row->y.mag, m.y.mag);
  return G::load(*row);
}
// g1_sum_kernel / g1_sum_ranks_kernel: Jacobian points of the C ABI - any three images - converted and summed with add
static bg1x chain_g1_sum(bg1_jac* out) {
  const char* w = "g1_sum_kernel";
  At at(w);
  const bfe any = BF::image_256();
  bg1x q;
  const bfl z = BF::from_ext(any);
  q.zz = BF::sqr(z);
  q.zzz = BF::mul(q.zz, z);
  q.x = BF::weak_reduce(BF::from_ext(any));
  q.y = BF::weak_reduce(BF::from_ext(any));
  const bg1x acc = fixed_point(q, [&](const bg1x& c) { return join(add_all(c, q, w), add_all(c, c, w)); }, w);
  At at2(w);
  *out = G::to_jac_ext(acc);
  return acc;
}
// term_mul: two bits per step over b, 2b, 3b.  b as k_verify_terms hands it over (load_abi: two from_ext products)
static bg1a abi_point() {
  const bfe any = BF::image_256();
  return bg1a{BF::from_ext(any), BF::from_ext(any)};
}
static bg1x chain_term_mul(const bg1a& b, const char* w) {
  bg1x b2, b3;
  {
    At at(w);
    b2 = G::dbl_affine(b);
  }
  b3 = add_mixed_all(b2, b, w);
  return fixed_point(add_mixed_all(G::inf(), b, w), [&](const bg1x& c) {
    At at(w);
    const bg1x d = G::dbl(G::dbl(c));
    return join(join(d, add_mixed_all(d, b, w)), join(add_all(d, b2, w), add_all(d, b3, w)));
  }, w);
}
// k_verify_terms: the terms summed per lane with add, a tree of add, to_affine, -y for B, to_ext
static bg1x chain_verify_terms(bfe* ox, bfe* oy) {
  const char* w = "k_verify_terms";
  const bg1x v = chain_term_mul(abi_point(), w);
  const bg1x acc = fixed_point(v, [&](const bg1x& c) { return join(add_all(c, v, w), add_all(c, c, w)); }, w);
  At at(w);
  bg1a q = G::to_affine(acc);
  *ox = BF::to_ext(q.x);
  *oy = BF::to_ext(BF::join(q.y, BF::neg(q.y)));
  return acc;
}

// ---- the quad-lane form (quad29.hpp) ---------------------------------------------------------------------------------
// Class Q, quad29.hpp's words: x, y < 2p; zz, zzz < 1.2p; limbs normalized.  The zero test of QuadG1::add is bit 0 of the
// plan; the general addition it then hands the gathered points to (`slow`) takes bits 1 and 2.
using QB = QuadG1<G, QuadSimT<bfl>>;
static const Cls CLS_Q = {"Q", 2 * U, 2 * U, U * 12 / 10, U * 12 / 10};
static bg1x quad_add(const bg1x& a, const bg1x& b, uint32_t plan, const char* w) {
  At at(w, plan);
  QB::V qa = QB::scatter(a);
  QB::add(qa, QB::scatter(b), [](const bg1x& x, const bg1x& y) { return G::add(x, y); });
  return QB::gather(qa);
}
static bg1x quad_dbl(const bg1x& a, const char* w) {
  At at(w);
  QB::V qa = QB::scatter(a);
  QB::dbl(qa);
  return QB::gather(qa);
}
static bg1x quad_closure(const bg1x& start, const char* w) {
  return fixed_point(start, [&](const bg1x& c) {
    bg1x n = quad_dbl(c, w);
    for (uint32_t plan : {0u, 1u, 3u, 7u}) n = join(n, quad_add(c, c, plan, w));
    return n;
  }, w);
}

// the finishing kernels that hold their points as quads (msm_combine_quad, msm_reduce_grid_quad, msm_reduce_grid_final_quad,
// msm_reduce_final_quad, msm_var_horner) mix both forms: the fold closure with the quad addition and doubling in it
static bg1x chain_fold_quad(const bg1_xyzz& bucket) {
  const char* w = "folds with the quad form";
  return fixed_point(G::load(bucket), [&](const bg1x& c) {
    bg1x n = join(add_tree_all(c, c, w), add_all(c, c, w));
    n = join(n, quad_dbl(c, w));
    for (uint32_t plan : {0u, 1u, 3u, 7u}) n = join(n, quad_add(c, c, plan, w));
    At at(w);
    n = join(n, G::dbl(c));
    return join(n, G::load(G::store(c)));
  }, w);
}

// ---- the Lagrange key builder (lagrange_elem29.hpp) ------------------------------------------------------------------
using BLag = LagT<kBoundSched>;
static bg1_xyzz join(const bg1_xyzz& a, const bg1_xyzz& b) {
  auto j = [](const bfe& x, const bfe& y) {
    bfe r;
    r.mag = x.mag > y.mag ? x.mag : y.mag;
    r.zero = x.zero && y.zero;
    return r;
  };
  return bg1_xyzz{j(a.x, b.x), j(a.y, b.y), j(a.zz, b.zz), j(a.zzz, b.zzz)};
}
static bool same(const bg1_xyzz& a, const bg1_xyzz& b) {
  return a.x.mag == b.x.mag && a.y.mag == b.y.mag && a.zz.mag == b.zz.mag && a.zzz.mag == b.zzz.mag;
}
static fe scalar_of(uint32_t pat) {
  fe k;
  for (int i = 0; i < 8; i++) k.v[i] = pat;
  return k;
}
// scalar_mul over every order of digits: b, 2b, 3b, then acc = 4 acc (+ one of them)
static bg1x lag_scalar_mul_closure(const bg1x& b, const char* w) {
  bg1x b2;
  {
    At at(w);
    b2 = G::dbl(b);
  }
  const bg1x b3 = add_all(b2, b, w);
  return fixed_point(join(b, join(b2, b3)), [&](const bg1x& c) {
    At at(w);
    const bg1x d = G::dbl(G::dbl(c));
    return join(join(d, add_all(d, b, w)), join(add_all(d, b2, w), add_all(d, b3, w)));
  }, w);
}
// lag_stage to the fixed point of the memory class: (A, B) -> (A + [k] B, A - [k] B) through the g1_xyzz image
static bg1_xyzz chain_lag_stage(const bg1_xyzz& start) {
  const char* w = "lag_stage";
  bg1_xyzz m = start;
  const uint32_t pats[4] = {0xffffffffu, 0x6c6c6c6cu, 0x1b1b1b1bu, 0x00000001u};
  for (int it = 0; it < 64; it++) {
    bg1_xyzz n = m, lo, hi;
    for (uint32_t plan = 0; plan < 16; plan++) {
      At at(w, plan);
      BLag::butterfly(m, m, scalar_of(1), false, lo, hi);
      n = join(n, join(lo, hi));
    }
    for (uint32_t pat : pats)
      for (uint32_t plan : {0u, 0xffffffffu, 0x55555555u, 0x33333333u, 0xaaaaaaaau}) {
        At at(w, plan);
        BLag::butterfly(m, m, scalar_of(pat), true, lo, hi);
        n = join(n, join(lo, hi));
      }
    {  // any order of digits: the closure of scalar_mul, then the two sums as butterfly forms them
      const bg1x A = G::load(m), B = lag_scalar_mul_closure(G::load(m), w);
      At at(w);
      const bg1x nb = BLag::neg_pt(B);
      const bg1x sums = join(add_all(A, B, w), add_all(A, nb, w));
      At at2(w);
      n = join(n, G::store(sums));
    }
    if (same(n, m)) return m;
    m = n;
  }
  CAP_BOUND_REQUIRE(!"the class keeps growing", w);
  return m;
}

// the largest k for which `closes(k)` holds with class A's y < k p, scanning up from the stated 3
template <class Fn>
static int largest_k(Fn closes) {
  BoundLog::quiet() = true;
  const bool fatal = BoundLog::fatal();
  BoundLog::fatal() = false;
  const long before = BoundLog::failures();
  const Cls keep = CLS_A;
  int best = 0;
  for (int k = 1; k <= 168; k++) {  // (a class below what the form itself returns does not close either)
    CLS_A.y = (uint64_t)k * U;
    const long f0 = BoundLog::failures();
    closes();
    if (BoundLog::failures() == f0) best = k;
  }
  CLS_A = keep;
  BoundLog::failures() = before;
  BoundLog::fatal() = fatal;
  BoundLog::quiet() = false;
  return best;
}

static int envelope(const std::string& control) {
  BoundLog::fatal() = !control.empty();  // a control stops at the first violation and names it
  if (control == "y17") CLS_A.y = 17 * U;
  if (control == "y17") {
    // the lean forms on the widened class: the field precondition that fails is named
    const bg1a tp = G::load(table_point());
    for (int neg = 0; neg < 2; neg++) {
      At at("madd_acc");
      bg1x a = pt(CLS_A);
      G::madd_acc(a, tp, neg != 0);
    }
  }
  const bg1_affine tm = table_point();
  const bg1a t = G::load(tm);
  const bg1x R = pt(CLS_R), ANY = G::load(any_bucket());
  g_json = "{\"curve\": {";
  char buf[256];
  snprintf(buf, sizeof buf, "\"classes\": {\"T\": [%llu, %llu], \"R\": [%llu, %llu, %llu, %llu], \"A\": [%llu, %llu, %llu, %llu], \"M\": %llu}",
           (unsigned long long)CLS_T.x, (unsigned long long)CLS_T.y, (unsigned long long)CLS_R.x, (unsigned long long)CLS_R.y,
           (unsigned long long)CLS_R.zz, (unsigned long long)CLS_R.zzz, (unsigned long long)CLS_A.x, (unsigned long long)CLS_A.y,
           (unsigned long long)CLS_A.zz, (unsigned long long)CLS_A.zzz, (unsigned long long)CLS_M.x);
  g_json += buf;

  open_section("ops");
  const bg1x A = pt(CLS_A);
  {
    At at("load");
    rec("load(T)", t, U);
    rec("load(M any image)", ANY, &CLS_M);
    rec("from_affine(T)", G::from_affine(t), &CLS_R);
  }
  {
    At at("dbl_affine");
    rec("dbl_affine(T)", G::dbl_affine(t), &CLS_R);
    rec("dbl_affine(x, y < 2p)", G::dbl_affine(bg1a{R.x, R.y}), &CLS_R);
    rec("dbl_affine(inf)", G::dbl_affine(bg1a{BF::zero(), BF::zero()}), &CLS_R);
  }
  {
    At at("dbl");
    rec("dbl(R)", G::dbl(R), &CLS_R);
    rec("dbl(A)", G::dbl(A), &CLS_R);
    rec("dbl(M any image)", G::dbl(ANY), &CLS_R);
    rec("dbl(inf)", G::dbl(G::inf()), &CLS_R);
  }
  for (int neg = 0; neg < 2; neg++) {
    const std::string sign = neg ? "-T" : "T";
    for (const bg1x* a : {&R, &A}) {
      const std::string cl = a == &R ? "R" : "A";
      const char* names[3] = {"", ": acc == -q", ": acc == q"};
      int i = 0;
      for (uint32_t plan : {0u, 1u, 3u}) {
        At at("add_mixed", plan);
        rec("add_mixed(" + cl + ", " + sign + ")" + names[i++], G::add_mixed(*a, t, neg != 0), &CLS_R);
      }
    }
    At at("add_mixed");
    rec("add_mixed(inf, " + sign + ")", G::add_mixed(G::inf(), t, neg != 0), &CLS_R);
    rec("add_mixed(A, inf " + sign + ")", G::add_mixed(A, bg1a{BF::zero(), BF::zero()}, neg != 0), &CLS_A);
    {
      At at2("madd_acc");
      bg1x a = A;
      const bool ok = G::madd_acc(a, t, neg != 0);
      CAP_BOUND_REQUIRE(ok, "madd_acc");
      rec("madd_acc(A, " + sign + ")", a, &CLS_A);
    }
    {
      At at2("madd_acc", 1);
      bg1x a = A;
      CAP_BOUND_REQUIRE(!G::madd_acc(a, t, neg != 0) && same(a, A), "madd_acc");  // refused: acc untouched
    }
  }
  {
    // zz (and zzz) of the accumulator any 32-byte image: no precondition of the lean forms fails and the result is
    // back in class A - the forms do not depend on the 1.2p of their comment
    bg1x wide = A;
    wide.zz = BF::load(BF::image_256());
    wide.zzz = BF::load(BF::image_256());
    for (int neg = 0; neg < 2; neg++) {
      At at("madd_acc");
      bg1x a = wide;
      CAP_BOUND_REQUIRE(G::madd_acc(a, t, neg != 0), "madd_acc");
      rec(std::string("madd_acc(A with zz, zzz any image, ") + (neg ? "-T)" : "T)"), a, &CLS_A);
    }
    At at("add_acc");
    bg1x a = wide;
    CAP_BOUND_REQUIRE(G::add_acc(a, wide), "add_acc");
    rec("add_acc(A with zz, zzz any image, same)", a, &CLS_A);
  }
  for (int s = 0; s < 4; s++) {
    At at("add_affine_pair");
    bg1x o = G::inf();
    const bool ok = G::add_affine_pair(o, t, (s & 1) != 0, t, (s & 2) != 0);
    CAP_BOUND_REQUIRE(ok, "add_affine_pair");
    rec(std::string("add_affine_pair(") + (s & 1 ? "-T" : "T") + ", " + (s & 2 ? "-T" : "T") + ")", o, &CLS_A);
    At at2("add_affine_pair", 1);
    bg1x u = A;
    CAP_BOUND_REQUIRE(!G::add_affine_pair(u, t, (s & 1) != 0, t, (s & 2) != 0) && same(u, A), "add_affine_pair");
  }
  for (const bg1x* a : {&A, &ANY}) {
    const std::string cl = a == &A ? "A" : "M any image";
    {
      At at("add_acc");
      bg1x s = *a;
      const bool ok = G::add_acc(s, *a);
      CAP_BOUND_REQUIRE(ok, "add_acc");
      rec("add_acc(" + cl + ", " + cl + ")", s, &CLS_A);
      At at2("add_acc", 1);
      bg1x u = *a;
      CAP_BOUND_REQUIRE(!G::add_acc(u, *a) && same(u, *a), "add_acc");
    }
    const char* names[3] = {"", ": a == -b", ": a == b"};
    int i = 0;
    for (uint32_t plan : {0u, 1u, 3u}) {
      At at("add", plan);
      rec("add(" + cl + ", " + cl + ")" + names[i++], G::add(*a, *a), &CLS_R);
    }
    At at("add");
    rec("add(inf, " + cl + ")", G::add(G::inf(), *a), a == &A ? &CLS_A : &CLS_M);
    rec("add(" + cl + ", inf)", G::add(*a, G::inf()), a == &A ? &CLS_A : &CLS_M);
  }
  {
    At at("add");
    rec("add(R, R)", G::add(R, R), &CLS_R);
  }
  {
    // scalars that take every digit (0 .. 3) and every length class; the bound field runs the real control flow
    const uint32_t pats[4] = {0xffffffffu, 0x6c6c6c6cu, 0x1b1b1b1bu, 0x00000001u};
    bg1x all = G::inf();
    for (uint32_t pat : pats)
      for (uint32_t plan : {0u, 1u, 3u}) {
        At at("term_mul", plan);
        fe k;
        for (int i = 0; i < 8; i++) k.v[i] = pat;
        all = join(all, G::term_mul(abi_point(), k));
      }
    rec("term_mul(ABI point, k)", all, &CLS_R);
    rec("term_mul: closure over all digit orders", chain_term_mul(abi_point(), "term_mul"), &CLS_R);
    At at("term_mul");
    fe zero_k;
    for (int i = 0; i < 8; i++) zero_k.v[i] = 0;
    rec("term_mul(ABI point, 0)", G::term_mul(abi_point(), zero_k), &CLS_R);
  }
  {
    At at("inv");
    const bfl i = G::inv(A.zzz);
    entry("inv(zzz of A)", coord("out", i));
    entry("inv(any image)", coord("out", G::inv(ANY.zzz)));
    entry("F::inv(any image)", coord("out", BF::inv(ANY.zzz)));
    At at2("to_affine");
    rec("to_affine(A)", G::to_affine(A), 2 * U);
    rec("to_affine(M any image)", G::to_affine(ANY), 2 * U);
    rec("to_affine(inf)", G::to_affine(G::inf()), 2 * U);
    At at3("store_affine");
    const bg1_affine sa = G::store_affine(G::to_affine(ANY));
    CAP_BOUND_REQUIRE(sa.x.mag <= U && sa.y.mag <= U, "store_affine");
    entry("store_affine(to_affine(M any image))", image("x", sa.x) + ", " + image("y", sa.y));
    At at4("store");
    rec("store(R)", G::store(R), BF::C256);
    rec("store(A)", G::store(A), BF::C256);
    At at5("to_jac_ext");
    rec("to_jac_ext(A)", G::to_jac_ext(A));
    rec("to_jac_ext(M any image)", G::to_jac_ext(ANY));
    rec("to_jac_ext(inf)", G::to_jac_ext(G::inf()));
  }
  close_section();

  open_section("chains");
  bg1_xyzz item, seg, folded;
  bg1_jac jac;
  bg1x S, T;
  if (control == "noweak") chain_accumulate<false>(CLS_A, &item);
  rec("msm_accumulate: acc", chain_accumulate<true>(CLS_A, &item), &CLS_A);
  rec("msm_accumulate: stored", item, BF::C256);
  chain_segments(item, &S, &T, &seg);
  rec("msm_reduce_segments(item sums): S", S, &CLS_A);
  rec("msm_reduce_segments(item sums): T", T, &CLS_A);
  rec("msm_reduce_segments(item sums): stored", seg, BF::C256);
  bg1_xyzz seg_any;
  chain_segments(any_bucket(), &S, &T, &seg_any);
  rec("msm_reduce_segments(any image): S", S, &CLS_M);
  rec("msm_reduce_segments(any image): T", T, &CLS_M);
  rec("msm_reduce_segments(any image): stored", seg_any, BF::C256 + 1);
  rec("folds(segment sums): point", chain_fold(seg, &folded, &jac), &CLS_A);
  rec("folds(segment sums): stored", folded, BF::C256);
  rec("folds(segment sums): to_jac_ext", jac);
  rec("folds(any image): point", chain_fold(any_bucket(), &folded, &jac), &CLS_M);
  rec("folds(any image): stored", folded, BF::C256 + 1);
  rec("folds(any image): to_jac_ext", jac);
  {
    bg1_affine row;
    rec("msm_precompute_kernel: row read back", chain_precompute(&row), U);  // class T: canonical
    CAP_BOUND_REQUIRE(row.x.mag <= U && row.y.mag <= U, "msm_precompute_kernel");
  }
  rec("g1_sum_kernel: acc", chain_g1_sum(&jac), &CLS_R);
  rec("g1_sum_kernel: to_jac_ext", jac);
  bfe ox, oy;
  rec("k_verify_terms: acc", chain_verify_terms(&ox, &oy), &CLS_R);
  CAP_BOUND_REQUIRE(ox.mag <= U && oy.mag <= U, "k_verify_terms");
  entry("k_verify_terms: out", image("x", ox) + ", " + image("y", oy));
  close_section();

  // the room the next optimisation of the lean forms has: the largest k for which "y < k p" still closes
  open_section("largest_k_of_y");
  if (control.empty()) {
    const int k_madd = largest_k([&] {
      for (int neg = 0; neg < 2; neg++) {
        BoundBranch::reset();
        bg1x a = pt(CLS_A);
        G::madd_acc(a, t, neg != 0);
        require_class(a, CLS_A, "madd_acc");
      }
    });
    const int k_acc = largest_k([&] {
      BoundBranch::reset();
      bg1x a = pt(CLS_A);
      G::add_acc(a, pt(CLS_A));
      require_class(a, CLS_A, "add_acc");
    });
    const int k_item = largest_k([&] {
      bg1_xyzz m;
      bg1x a = pt(CLS_A);
      for (int neg = 0; neg < 2; neg++) {
        BoundBranch::reset();
        bg1x b = pt(CLS_A);
        G::madd_acc(b, t, neg != 0);
        a = join(a, b);
      }
      require_class(a, CLS_A, "madd_acc");
      m = G::store(pt(CLS_A));
      (void)m;
    });
    const int k_seg = largest_k([&] {
      BoundBranch::reset();
      bg1x a = pt(CLS_A);
      G::add_acc(a, G::load(G::store(pt(CLS_A))));
      require_class(a, CLS_A, "add_acc");
    });
    snprintf(buf, sizeof buf, "\"madd_acc\": %d, \"add_acc\": %d, \"madd_acc then store\": %d, \"store, load, add_acc\": %d", k_madd,
             k_acc, k_item, k_seg);
    g_json += buf;
  }
  close_section();
  g_json += "}";

  g_json += ", \"quad\": {";
  open_section("ops");
  const bg1x Q = pt(CLS_Q);
  rec("add(Q, Q)", quad_add(Q, Q, 0, "QuadG1::add"), &CLS_Q);
  rec("add(Q, Q): slow", quad_add(Q, Q, 1, "QuadG1::add"), &CLS_Q);
  rec("add(Q, Q): slow, a == -b", quad_add(Q, Q, 3, "QuadG1::add"), &CLS_Q);
  rec("add(Q, Q): slow, a == b", quad_add(Q, Q, 7, "QuadG1::add"), &CLS_Q);
  rec("add(inf, Q)", quad_add(G::inf(), Q, 0, "QuadG1::add"), &CLS_Q);
  rec("add(Q, inf)", quad_add(Q, G::inf(), 0, "QuadG1::add"), &CLS_Q);
  rec("dbl(Q)", quad_dbl(Q, "QuadG1::dbl"), &CLS_Q);
  rec("dbl(inf)", quad_dbl(G::inf(), "QuadG1::dbl"), &CLS_Q);
  rec("add(A, A)", quad_add(A, A, 0, "QuadG1::add"), &CLS_Q);
  rec("add(M any image, M any image)", quad_add(ANY, ANY, 0, "QuadG1::add"), &CLS_Q);
  rec("dbl(A)", quad_dbl(A, "QuadG1::dbl"), &CLS_Q);
  rec("dbl(M any image)", quad_dbl(ANY, "QuadG1::dbl"), &CLS_Q);
  close_section();
  open_section("chains");
  rec("add / dbl from Q", quad_closure(Q, "quad closure"), &CLS_Q);
  rec("add / dbl from A", quad_closure(A, "quad closure"), &CLS_A);
  rec("add / dbl from M any image", quad_closure(ANY, "quad closure"), &CLS_M);
  rec("folds with the quad form (segment sums)", chain_fold_quad(seg), &CLS_A);
  rec("folds with the quad form (any image)", chain_fold_quad(any_bucket()), &CLS_M);
  close_section();
  g_json += "}";

  g_json += ", \"lagrange\": {";
  open_section("chains");
  {
    At at("lag_load");
    const bg1_xyzz loaded = BLag::load_point(tm);
    rec("lag_load: stored", loaded, U);
    const bg1_xyzz stage = chain_lag_stage(loaded);
    rec("lag_stage: stored", stage, BF::C256);
    rec("lag_stage(any image): stored", chain_lag_stage(any_bucket()), BF::C256 + 1);
    rec("scalar_mul: closure over all digit orders", lag_scalar_mul_closure(G::load(stage), "scalar_mul"), &CLS_R);
    const bg1_xyzz a[2] = {stage, stage};
    const bg1_affine srs[2] = {tm, tm};
    bfe worst = bfe();
    for (uint32_t pat : {0xffffffffu, 0x6c6c6c6cu, 0x1b1b1b1bu, 0x00000001u, 0u})
      for (uint32_t j = 0; j < 2; j++)
        for (uint32_t plan : {0u, 1u, 3u}) {
          At at2("lag_finish", plan);
          bg1_affine o;
          BLag::finish(a, 1, scalar_of(pat), srs, j, o);
          worst.mag = std::max(worst.mag, std::max(o.x.mag, o.y.mag));
        }
    CAP_BOUND_REQUIRE(worst.mag <= U, "lag_finish");
    entry("lag_finish: out", image("x, y", worst));
  }
  close_section();
  g_json += "}}";
  printf("%s\n", g_json.c_str());
  return BoundLog::failures() ? 2 : 0;
}

// ---- run: concrete operands through the real law -------------------------------------------------------------------
// Every line: OP then its operands; a point is 4 x 9 hex limbs (x y zz zzz), an affine point 2 x 9, a flag 0 / 1.
//   madd A Q neg | pair Q0 neg0 Q1 neg1 | addacc A B | add A B | addmixed A Q neg | dbl A | dblaffine Q |
//   item Q0 n0 Q1 n1 (Q neg) x 6  (add_affine_pair -> 6 x madd_acc -> store -> load) |
//   fold A B C  (add_acc, add_acc -> dbl -> to_jac_ext; prints the point before to_jac_ext and the triple after)
//   termmul | toaffine | jac | inv | segwalk | mulsmall | quad | lagstage | lagfinish | terms: see the branches below
// -> "ok" (0 / 1: the lean form's return value) and the result's limbs
static bool rd(fl& o) {
  for (int i = 0; i < 9; i++)
    if (scanf("%x", &o.v[i]) != 1) return false;
  return true;
}
static bool rd(g1x& p) { return rd(p.x) && rd(p.y) && rd(p.zz) && rd(p.zzz); }
static bool rd(g1a& p) { return rd(p.x) && rd(p.y); }
static void pr(const fl& a) {
  for (int i = 0; i < 9; i++) printf(" %x", a.v[i]);
}
static void pr(int ok, const g1x& p) {
  printf("%d", ok);
  pr(p.x), pr(p.y), pr(p.zz), pr(p.zzz);
  printf("\n");
}
static void pr_words(const fe& w) {
  for (int i = 7; i >= 0; i--) printf("%08x", w.v[i]);
  printf(" ");
}
template <class GL>
struct LagLawOf;
template <>
struct LagLawOf<G1LT<0>> {
  using T = LagT<0>;
};
template <>
struct LagLawOf<G1LT<1>> {
  using T = LagT<1>;
};
template <class GL>
static int run_rows() {
  char op[16];
  while (scanf("%15s", op) == 1) {
    const std::string o(op);
    g1x a, b, c;
    g1a q, q1;
    int n0, n1;
    if (o == "madd") {
      if (!rd(a) || !rd(q) || scanf("%d", &n0) != 1) return 3;
      const bool ok = GL::madd_acc(a, q, n0 != 0);
      pr(ok, a);
    } else if (o == "pair") {
      if (!rd(q) || scanf("%d", &n0) != 1 || !rd(q1) || scanf("%d", &n1) != 1) return 3;
      a = GL::inf();
      const bool ok = GL::add_affine_pair(a, q, n0 != 0, q1, n1 != 0);
      pr(ok, a);
    } else if (o == "addacc") {
      if (!rd(a) || !rd(b)) return 3;
      const bool ok = GL::add_acc(a, b);
      pr(ok, a);
    } else if (o == "add") {
      if (!rd(a) || !rd(b)) return 3;
      pr(1, GL::add(a, b));
    } else if (o == "addmixed") {
      if (!rd(a) || !rd(q) || scanf("%d", &n0) != 1) return 3;
      pr(1, GL::add_mixed(a, q, n0 != 0));
    } else if (o == "dbl") {
      if (!rd(a)) return 3;
      pr(1, GL::dbl(a));
    } else if (o == "dblaffine") {
      if (!rd(q)) return 3;
      pr(1, GL::dbl_affine(q));
    } else if (o == "item") {
      if (!rd(q) || scanf("%d", &n0) != 1 || !rd(q1) || scanf("%d", &n1) != 1) return 3;
      a = GL::inf();
      bool ok = GL::add_affine_pair(a, q, n0 != 0, q1, n1 != 0);
      for (int i = 0; i < 6; i++) {
        if (!rd(q) || scanf("%d", &n0) != 1) return 3;
        ok = ok && GL::madd_acc(a, q, n0 != 0);
      }
      pr(ok, GL::load(GL::store(a)));
    } else if (o == "fold") {
      if (!rd(a) || !rd(b) || !rd(c)) return 3;
      bool ok = GL::add_acc(a, b);
      ok = ok && GL::add_acc(a, c);
      a = GL::dbl(a);
      pr(ok, a);
      const g1_jac j = GL::to_jac_ext(a);
      for (const fe* w : {&j.x, &j.y, &j.z}) {
        for (int i = 7; i >= 0; i--) printf("%08x", w->v[i]);
        printf(" ");
      }
      printf("\n");
    } else if (o == "termmul") {  // Q, then the scalar as 8 hex words, low word first
      fe k;
      if (!rd(q)) return 3;
      for (int i = 0; i < 8; i++)
        if (scanf("%x", &k.v[i]) != 1) return 3;
      pr(1, GL::term_mul(q, k));
    } else if (o == "toaffine") {  // -> x, y of to_affine, then store_affine's two images
      if (!rd(a)) return 3;
      const g1a t = GL::to_affine(a);
      g1x out = GL::inf();
      out.x = t.x, out.y = t.y;
      pr(1, out);
      const g1_affine m = GL::store_affine(t);
      pr_words(m.x), pr_words(m.y);
      printf("\n");
    } else if (o == "jac") {  // to_jac_ext of a point as given (a bucket image)
      if (!rd(a)) return 3;
      const g1_jac j = GL::to_jac_ext(a);
      pr_words(j.x), pr_words(j.y), pr_words(j.z);
      printf("\n");
    } else if (o == "inv") {
      if (!rd(a.x)) return 3;
      a.y = GL::inv(a.x);
      a.zz = GL::F::inv(a.x);
      a.zzz = GL::F::zero();
      pr(1, a);
    } else if (o == "segwalk") {  // n buckets (all-zero = empty): the S / T walk of msm_reduce_segments -> S, T reloaded
      int n;
      if (scanf("%d", &n) != 1 || n < 1 || n > 16) return 3;
      std::vector<g1_xyzz> bk(n);
      for (auto& m : bk) {
        if (!rd(a)) return 3;
        m = GL::store(a);
      }
      g1x S = GL::load(bk[n - 1]), T = S;
      for (int j = n - 1; j > 0; j--) {
        const g1x cur = GL::load(bk[j - 1]);
        if (!GL::is_inf(cur)) {
          if (GL::is_inf(S)) S = cur;
          else if (!GL::add_acc(S, cur)) S = GL::add(S, cur);
        }
        if (!GL::is_inf(S)) {
          if (GL::is_inf(T)) T = S;
          else if (!GL::add_acc(T, S)) T = GL::add(T, S);
        }
      }
      pr(1, GL::load(GL::store(S)));
      pr(1, GL::load(GL::store(T)));
    } else if (o == "mulsmall") {  // A k: mul_small of msm.hip
      uint32_t k;
      if (!rd(a) || scanf("%u", &k) != 1) return 3;
      g1x r = GL::inf();
      for (int bit = 31; bit >= 0; bit--) {
        if (!GL::is_inf(r)) r = GL::dbl(r);
        if ((k >> bit) & 1) r = GL::add(r, a);
      }
      pr(1, r);
    } else if (o == "horner") {  // c n S_(n-1) .. S_0: the window Horner of msm_var_horner - c doublings, then the next sum
      int c, n;
      if (scanf("%d %d", &c, &n) != 2 || n < 1 || n > 8 || c < 1 || c > 16) return 3;
      g1x acc = GL::inf();
      for (int w = 0; w < n; w++) {
        if (!rd(b)) return 3;
        if (w)
          for (int k = 0; k < c; k++) acc = GL::dbl(acc);
        if (!GL::is_inf(b)) {  // add_tree of msm.hip
          if (GL::is_inf(acc)) acc = b;
          else if (!GL::add_acc(acc, b)) acc = GL::add(acc, b);
        }
      }
      pr(1, GL::load(GL::store(acc)));
    } else if (o == "g1sum") {  // n, then n x (x y z as 8 hex words each): the body of g1_sum_kernel / g1_sum_ranks_kernel
      int n;
      if (scanf("%d", &n) != 1 || n < 1 || n > 8) return 3;
      using F = typename GL::F;
      g1x acc = GL::inf();
      for (int t = 0; t < n; t++) {
        fe w[3];
        for (auto& e : w)
          for (int i = 0; i < 8; i++)
            if (scanf("%x", &e.v[i]) != 1) return 3;
        g1x p = GL::inf();
        if (!Fq::is_zero(w[2])) {
          const fl z = F::from_ext(w[2]);
          p.zz = F::sqr(z);
          p.zzz = F::mul(p.zz, z);
          p.x = F::weak_reduce(F::from_ext(w[0]));
          p.y = F::weak_reduce(F::from_ext(w[1]));
        }
        acc = GL::add(acc, p);
      }
      acc = GL::add(acc, acc);  // a level of the shuffle tree with the lane's own value: the doubling path
      pr(1, acc);
      const g1_jac j = GL::to_jac_ext(acc);
      pr_words(j.x), pr_words(j.y), pr_words(j.z);
      printf("\n");
    } else if (o == "quad") {  // A B: the quad-lane (A + B), 2 (A + B) and 2 (A + B) + B
      if (!rd(a) || !rd(b)) return 3;
      using Q = QuadG1<GL, QuadSim>;
      auto slow = [](const g1x& x, const g1x& y) { return GL::add(x, y); };
      typename Q::V v = Q::scatter(a);
      Q::add(v, Q::scatter(b), slow);
      pr(1, Q::gather(v));
      Q::dbl(v);
      pr(1, Q::gather(v));
      Q::add(v, Q::scatter(b), slow);
      pr(1, Q::gather(v));
    } else if (o == "lagstage") {  // A B k(8 words) has_k: lag_stage's butterfly through the images -> lo, hi reloaded
      fe k;
      if (!rd(a) || !rd(b)) return 3;
      for (int i = 0; i < 8; i++)
        if (scanf("%x", &k.v[i]) != 1) return 3;
      if (scanf("%d", &n0) != 1) return 3;
      using L = LagLawOf<GL>;
      g1_xyzz lo, hi;
      L::T::butterfly(GL::store(a), GL::store(b), k, n0 != 0, lo, hi);
      pr(1, GL::load(lo));
      pr(1, GL::load(hi));
    } else if (o == "lagfinish") {  // j n_inv(8 words) A0 A1 srs0 .. srs3: lag_finish with n = 2 - j < 2 scales a[j], j = 2, 3
                                    // is a blinding point srs[j] - srs[j - 2]; the array through store(), the rows through
                                    // store_affine() -> the two words of out[j]
      uint32_t j;
      fe k;
      if (scanf("%u", &j) != 1 || j > 3) return 3;
      for (int i = 0; i < 8; i++)
        if (scanf("%x", &k.v[i]) != 1) return 3;
      g1_xyzz arr[2];
      g1_affine srs[4], out;
      for (auto& m : arr) {
        if (!rd(a)) return 3;
        m = GL::store(a);
      }
      for (auto& m : srs) {
        if (!rd(q)) return 3;
        m = GL::store_affine(q);
      }
      LagLawOf<GL>::T::finish(arr, 2, k, srs, j, out);
      pr_words(out.x), pr_words(out.y);
      printf("\n");
    } else if (o == "terms") {  // n, then n x (Q k): k_verify_terms - term_mul, add, to_affine, -y, to_ext
      int n;
      if (scanf("%d", &n) != 1 || n < 1 || n > 8) return 3;
      g1x acc = GL::inf();
      for (int t = 0; t < n; t++) {
        fe k;
        if (!rd(q)) return 3;
        for (int i = 0; i < 8; i++)
          if (scanf("%x", &k.v[i]) != 1) return 3;
        acc = GL::add(acc, GL::term_mul(q, k));
      }
      acc = GL::add(acc, GL::inf());
      g1a t = GL::to_affine(acc);
      t.y = GL::F::neg(t.y);
      pr_words(GL::F::to_ext(t.x)), pr_words(GL::F::to_ext(t.y));
      printf("\n");
    } else {
      return 3;
    }
  }
  return 0;
}

// ---- ops: the operations bound29.hpp gained for the law, the real one and the bound one side by side --------------------
// line: op sched n, then n operands "L v0 .. v8 lo hi mag zero" (hex limbs, then the operand's class); prints
// "B 0|1" (is_zero, eq) or "L v0 .. v8 lo hi mag" - tests/cpp/ntt_elem_check.cpp's protocol, on the base field
template <class F>
static bool one_op(const std::string& op, const fl* x, const bfl* b) {
  BoundBranch::reset();
  if (op == "is_zero") {
    (void)BF::is_zero(b[0]);
    printf("B %d\n", F::is_zero(x[0]) ? 1 : 0);
    return true;
  }
  if (op == "eq") {
    (void)BF::eq(b[0], b[1]);
    printf("B %d\n", F::eq(x[0], x[1]) ? 1 : 0);
    return true;
  }
  fl r;
  bfl br;
  if (op == "inv") {
    r = F::inv(x[0]);
    br = BF::inv(b[0]);
  } else if (op == "g1_inv") {  // the square-and-multiply of the law (G1Law::inv)
    r = G1Law<F, fl>::inv(x[0]);
    br = G::inv(b[0]);
  } else if (op == "mul") {
    r = F::mul(x[0], x[1]);
    br = BF::mul(b[0], b[1]);
  } else if (op == "mul_add_mul") {
    r = F::mul_add_mul(x[0], x[1], x[2], x[3]);
    br = BF::mul_add_mul(b[0], b[1], b[2], b[3]);
  } else {
    return false;
  }
  printf("L");
  for (int i = 0; i < 9; i++) printf(" %x", r.v[i]);
  printf(" %llx %llx %llx\n", (unsigned long long)br.lo, (unsigned long long)br.hi, (unsigned long long)br.mag);
  return true;
}
static int run_ops() {
  char op[32];
  int sched, n;
  while (scanf("%31s %d %d", op, &sched, &n) == 3) {
    fl x[4];
    bfl b[4];
    if (n < 1 || n > 4) return 3;
    for (int i = 0; i < n; i++) {
      char kind[4];
      unsigned long long lo, hi, mag;
      int z;
      if (scanf("%3s", kind) != 1 || kind[0] != 'L') return 3;
      for (int k = 0; k < 9; k++)
        if (scanf("%x", &x[i].v[k]) != 1) return 3;
      if (scanf("%llx %llx %llx %d", &lo, &hi, &mag, &z) != 4) return 3;
      b[i].lo = lo, b[i].hi = hi, b[i].mag = mag, b[i].zero = z != 0;
    }
    if (!(sched ? one_op<Fl<FqP29, 1>>(op, x, b) : one_op<Fl<FqP29, 0>>(op, x, b))) {
      fprintf(stderr, "unknown op %s\n", op);
      return 3;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "envelope") return envelope(argc > 2 ? argv[2] : "");
  if (mode == "ops") return run_ops();
  if (mode == "run" && argc == 3) return atoi(argv[2]) ? run_rows<G1LT<1>>() : run_rows<G1LT<0>>();
  fprintf(stderr, "usage: curve_envelope_check envelope [y17 | noweak] | run SCHED | ops\n");
  return 3;
}
