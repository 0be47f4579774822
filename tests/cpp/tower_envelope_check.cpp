// The pairing tower of cap_amd/csrc/pairing29.hpp (Tower<SCHED>, through TowerField) on the bound-tracking field (bound29.hpp,
// bound_tower29.hpp): every function, the Miller loop and the final exponentiation for ALL inputs of class E.  Driven by
// tests/test_tower_envelope_host.py:
//   tower_envelope_check envelope [e17]   the largest limb and magnitude over the coefficients of every result as JSON (the
//                                         "tower" section of tests/golden/lazy_envelope.json); exit code 2 and the violated
//                                         operation on stderr if a precondition fails or a result leaves class E.
//                                         e17: class E widened to coefficients < 17p - the driver expects exit code 2
//   tower_envelope_check run              concrete elements on stdin through the real Tower<0> / Tower<1> with the bound
//                                         assertions of field29.hpp on (layout at run_rows)
// Class E, the header's words: every Fq value held in an f2 / f6 / f12 is normalized and < 2p.  Line coefficients are
// canonical and packed.  The G1 point of a pairing is what k_pairing_check2 hands over: load_abi's two from_ext products
// of arbitrary 32-byte images, through eval_point.
#define CAP_FL_CHECK 1
#include "bound_tower29.hpp"

#include "../hip/devcheck_ops.hpp"

#include <algorithm>
#include <string>
#include <vector>

using namespace cap;
using capbound::bf12;
using capbound::bf2;
using capbound::bf6;
using capbound::bfe;
using capbound::bfl;
using capbound::bline;
using capbound::BoundBranch;
using capbound::BoundLog;
using BF = capbound::BoundFl<FqP29>;
using T = capbound::BoundTower;
static constexpr uint64_t U = BF::U;
static constexpr uint64_t CLASS_E = 2 * U;  // the header's "< 2p"
static uint64_t E_MAG = CLASS_E;            // the class the operands are drawn from (e17 widens it)

struct Worst {  // over the coefficients of a result
  uint64_t lim = 0, mag = 0;
  bool ok = true;
  void take(const bfl& a) {
    if (a.zero) return;
    lim = std::max(lim, BF::lim(a));
    mag = std::max(mag, a.mag);
    ok = ok && BF::normalized(a) && a.mag <= CLASS_E;
  }
  void take(const bf2& a) { take(a.c0), take(a.c1); }
  void take(const bf6& a) { take(a.c0), take(a.c1), take(a.c2); }
  void take(const bf12& a) { take(a.c0), take(a.c1); }
};
static std::string g_json;
static bool g_first = true;
template <class X>
static void rec(const char* name, const X& x) {
  Worst w;
  w.take(x);
  CAP_BOUND_REQUIRE(w.ok, name);  // the result is in class E
  char buf[200];
  snprintf(buf, sizeof buf, "%s\"%s\": [%llu, %llu]", g_first ? "" : ", ", name, (unsigned long long)w.lim,
           (unsigned long long)w.mag);
  g_json += buf;
  g_first = false;
}
static void at(const char* w, uint32_t plan = 0) {
  BoundLog::where() = w;
  BoundBranch::reset(plan);
}
static bfl e1() { return BF::norm_of(E_MAG); }
static bf2 e2() { return bf2{e1(), e1()}; }
static bf6 e6() { return bf6{e2(), e2(), e2()}; }
static bf12 e12() { return bf12{e6(), e6()}; }
static bfl join(const bfl& a, const bfl& b) { return BF::join(a, b); }
static bf2 join(const bf2& a, const bf2& b) { return bf2{join(a.c0, b.c0), join(a.c1, b.c1)}; }
static bf6 join(const bf6& a, const bf6& b) { return bf6{join(a.c0, b.c0), join(a.c1, b.c1), join(a.c2, b.c2)}; }
static bf12 join(const bf12& a, const bf12& b) { return bf12{join(a.c0, b.c0), join(a.c1, b.c1)}; }
static bool same(const bf12& a, const bf12& b) {
  const bfl* p = &a.c0.c0.c0;
  const bfl* q = &b.c0.c0.c0;
  for (int i = 0; i < 12; i++)
    if (p[i].lo != q[i].lo || p[i].hi != q[i].hi || p[i].mag != q[i].mag || p[i].zero != q[i].zero) return false;
  return true;
}
template <class Step>
static bf12 fixed_point(bf12 c, Step step, const char* w) {
  for (int it = 0; it < 64; it++) {
    const bf12 n = join(c, step(c));
    if (same(n, c)) return c;
    c = n;
  }
  CAP_BOUND_REQUIRE(!"the class keeps growing", w);
  return c;
}

static int envelope(bool wide) {
  static_assert(sizeof(bf12) == 12 * sizeof(bfl), "same() walks the twelve coefficients");
  BoundLog::fatal() = wide;
  if (wide) E_MAG = 17 * U;
  g_json = "{\"tower\": {\"class_E\": " + std::to_string((unsigned long long)E_MAG) + ", \"ops\": {";
  const bfl a1 = e1();
  const bf2 a2 = e2();
  const bf6 a6 = e6();
  const bf12 a12 = e12();
#define OP(name, expr) \
  do {                 \
    at(name);          \
    rec(name, expr);   \
  } while (0)
  OP("add", T::add(a1, a1));
  OP("sub", T::sub(a1, a1));
  OP("neg", T::neg(a1));
  OP("mul9", T::mul9(a1));
  OP("f2_add", T::f2_add(a2, a2));
  OP("f2_sub", T::f2_sub(a2, a2));
  OP("f2_neg", T::f2_neg(a2));
  OP("f2_conj", T::f2_conj(a2));
  OP("f2_dbl", T::f2_dbl(a2));
  OP("f2_mul", T::f2_mul(a2, a2));
  OP("f2_sqr", T::f2_sqr(a2));
  OP("f2_mul_fq", T::f2_mul_fq(a2, a1));
  OP("f2_mul_xi", T::f2_mul_xi(a2));
  OP("f2_inv", T::f2_inv(a2));
  OP("f2_konst", T::f2_konst(p29::PairConst::FROB[0][0]));
  OP("f6_add", T::f6_add(a6, a6));
  OP("f6_sub", T::f6_sub(a6, a6));
  OP("f6_neg", T::f6_neg(a6));
  OP("f6_mul_v", T::f6_mul_v(a6));
  OP("f6_mul", T::f6_mul(a6, a6));
  OP("f6_mul_01", T::f6_mul_01(a6, a2, a2));
  OP("f6_mul_fq", T::f6_mul_fq(a6, a1));
  OP("f6_mul_f2", T::f6_mul_f2(a6, a2));
  OP("f6_inv", T::f6_inv(a6));
  OP("f12_one", T::f12_one());
  OP("f12_conj", T::f12_conj(a12));
  OP("f12_mul", T::f12_mul(a12, a12));
  OP("f12_sqr", T::f12_sqr(a12));
  OP("f12_mul_line", T::f12_mul_line(a12, a1, a2, a2));
  OP("f12_inv", T::f12_inv(a12));
  OP("f12_frob 1", T::f12_frob(a12, 1));
  OP("f12_frob 2", T::f12_frob(a12, 2));
  OP("f12_frob 3", T::f12_frob(a12, 3));
  OP("f12_cyclo_sqr", T::f12_cyclo_sqr(a12));
  OP("f12_exp_x", T::f12_exp_x(a12));
  OP("f12_exp_neg_x", T::f12_exp_neg_x(a12));
  OP("final_exp", T::final_exp(a12));
  // the zero tests: both answers of every one (the operands must be normalized, < 2^261, and sub's subtrahend < 15.9p)
  for (uint32_t plan : {0u, 0xffffffffu, 0x55555555u, 0xaaaaaaaau}) {
    at("f12_is_one", plan);
    (void)T::f12_is_one(a12);
    at("f2_is_zero", plan);
    (void)T::f2_is_zero(a2);
  }
  // the G1 point as k_pairing_check2 hands it over, and a prepared line
  at("eval_point");
  const bfe any = BF::image_256();
  const T::g1_eval pe = T::eval_point(BF::from_ext(any), BF::from_ext(any), false);
  rec("eval_point: s", pe.s);
  rec("eval_point: xp", pe.xp);
  const bline line = bline{BF::image(U), BF::image(U), BF::image(U), BF::image(U)};
  OP("mul_prepared", T::mul_prepared(a12, line, pe));
  const T::g1_eval pinf = T::eval_point(BF::from_ext(any), BF::from_ext(any), true);
  OP("mul_prepared: infinity", T::mul_prepared(a12, line, pinf));
  g_json += "}, \"chains\": {";
  g_first = true;
  // the Miller loop as miller2 runs it (its control flow is a constant), and its step to the fixed point of the class
  const std::vector<bline> lines(p29::kLines, line);
  OP("miller2", T::miller2(lines.data(), pe, lines.data(), pe));
  OP("miller2: one pair at infinity", T::miller2(lines.data(), pe, lines.data(), pinf));
  at("miller step");
  const bf12 f = fixed_point(T::f12_one(), [&](const bf12& c) {
    const bf12 s = T::f12_sqr(c);
    return join(s, join(T::mul_prepared(c, line, pe), T::mul_prepared(s, line, pe)));
  }, "miller step");
  rec("miller step: fixed point", f);
  OP("final_exp(miller2)", T::final_exp(f));
  at("f12_exp_x step");
  rec("f12_exp_x step: fixed point", fixed_point(a12, [&](const bf12& c) {
        const bf12 s = T::f12_cyclo_sqr(c);
        return join(s, T::f12_mul(s, a12));
      }, "f12_exp_x step"));
  for (uint32_t plan : {0u, 0xffffffffu}) {
    at("check2", plan);
    (void)T::check2(lines.data(), pe, lines.data(), pe);
  }
  g_json += "}}}";
  printf("%s\n", g_json.c_str());
  return BoundLog::failures() ? 2 : 0;
}

// ---- run: concrete elements through the real tower ---------------------------------------------------------------------
// Every line: op code, schedule, aux, then two elements of 108 hex words (tests/hip/devcheck_ops.hpp: the TOWER group's
// record, so that tests/devcheck_vectors.py's conversions and oracle expectations serve here too) -> 108 result words
static int run_rows() {
  using namespace devcheck;
  std::vector<uint32_t> in(kInWords[G_TOWER]), out(kOutWords[G_TOWER]);
  while (scanf("%x %x %x", &in[0], &in[2], &in[3]) == 3) {
    in[1] = 0;
    for (size_t i = 4; i < in.size(); i++)
      if (scanf("%x", &in[i]) != 1) return 3;
    std::fill(out.begin(), out.end(), 0xffffffffu);
    run_tower(in.data(), out.data());
    if (out[109] != kDone + in[0]) return 3;
    for (int i = 0; i < 108; i++) printf("%x ", out[i]);
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "envelope") return envelope(argc > 2 && std::string(argv[2]) == "e17");
  if (mode == "run") return run_rows();
  fprintf(stderr, "usage: tower_envelope_check envelope [e17] | run\n");
  return 3;
}
