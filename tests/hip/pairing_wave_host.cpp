// Host driver for cap_amd/csrc/pairing_wave.hpp: the lane-group Fq12 arithmetic on six emulated lanes (pw::GroupSim)
// with field29.hpp's bound assertions on, next to the one-lane Tower<> of pairing29.hpp on the same inputs.  Reads one
// operation per line on stdin and prints TWO lines per operation: the group form's result, then Tower<>'s;
// tests/test_pairing_wave_host.py demands them equal and checks them against Python integers / oracle/pairing.py.
// Values are hex integers.  An Fq12 is 12 of them: for k = 0..5 the Fq2 coefficient (x, y) of w^k.  A line that starts
// with R takes every field value RAW: the integer (< 2^261) is spread over the 29-bit limbs and used as the internal
// representative as it stands (bound-extreme inputs: p, 2p - 1, ...), and results are printed as canonical internal
// values; otherwise values are plain integers, converted to and from the Montgomery form.
//   M a b | S a | C a | I a | E a | F j a     product, squaring, cyclotomic squaring, inverse, final exponentiation, Frobenius
//   N a s b0 b1                               a * (s + b0 w + b1 w^3): the sparse product by a line
//   L P Q                                     the prepared-line Miller loop of one pair
//   K P1 Q1 P2 Q2                             1 if e(P1, Q1) e(P2, Q2) == 1 else 0
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/pairing_wave.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace cap;
using T = p29::Tower<CAP_FL_SCHED>;
using W = pw::Wave<pw::GroupSim, CAP_FL_SCHED>;
using F = T::F;
using V = W::V;

static bool g_raw = false;

static void read_hex(char* s) {
  if (scanf(" %159s", s) != 1) exit(2);
}
static uint32_t nibble(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }
static fe read_fe() {
  char s[160];
  read_hex(s);
  fe r;
  memset(&r, 0, sizeof r);
  const int n = (int)strlen(s);
  for (int i = 0; i < n; i++) {
    const int d = n - 1 - i;
    r.v[d / 8] |= nibble(s[i]) << (4 * (d % 8));
  }
  return r;
}
static fl read_raw() {
  char s[160];
  read_hex(s);
  fl r = F::zero();
  const int n = (int)strlen(s);
  for (int i = 0; i < n; i++) {
    const int d = n - 1 - i;
    const uint32_t v = nibble(s[i]);
    for (int b = 0; b < 4; b++)
      if ((v >> b) & 1) {
        const int pos = 4 * d + b;
        if (pos >= 261) exit(4);
        r.v[pos / 29] |= 1u << (pos % 29);
      }
  }
  return r;
}
static fl read_fl() { return g_raw ? read_raw() : F::to_mont(read_fe()); }
static void print_fl(const fl& a) {
  const fe o = g_raw ? F::pack(F::canonical(a)) : F::from_mont(a);
  for (int i = 7; i >= 0; i--) printf("%08x", o.v[i]);
  printf(" ");
}
static p29::f2 read_f2() {
  p29::f2 r;
  r.c0 = read_fl();
  r.c1 = read_fl();
  return r;
}
static p29::f2* slot(p29::f12& a, int k) {
  p29::f6& h = (k & 1) ? a.c1 : a.c0;
  return k / 2 == 0 ? &h.c0 : (k / 2 == 1 ? &h.c1 : &h.c2);
}
static V read_v() {
  V a;
  for (int k = 0; k < pw::kGroup; k++) a.l[k] = read_f2();
  return a;
}
static p29::f12 to_tower(const V& v) {
  p29::f12 a;
  for (int k = 0; k < pw::kGroup; k++) *slot(a, k) = v.l[k];
  return a;
}
static void print_v(const V& a) {
  for (int k = 0; k < pw::kGroup; k++) {
    print_fl(a.l[k].c0);
    print_fl(a.l[k].c1);
  }
  printf("\n");
}
static void print_both(const V& w, p29::f12 t) {
  print_v(w);
  V tv;
  for (int k = 0; k < pw::kGroup; k++) tv.l[k] = *slot(t, k);
  print_v(tv);
}
static T::g1_eval read_g1() {
  const fe x = read_fe(), y = read_fe();
  bool inf = true;
  for (int i = 0; i < 8; i++) inf = inf && x.v[i] == 0 && y.v[i] == 0;
  return T::eval_point(F::to_mont(x), F::to_mont(y), inf);
}
static std::vector<p29::line_coeffs> read_g2_lines() {
  pairing::g2_affine q;
  q.x.c0 = Fq::to_mont(read_fe());
  q.x.c1 = Fq::to_mont(read_fe());
  q.y.c0 = Fq::to_mont(read_fe());
  q.y.c1 = Fq::to_mont(read_fe());
  std::vector<p29::line_coeffs> l(p29::kLines);
  p29::prepare_lines(q, l.data());
  return l;
}

int main() {
  char op;
  while (scanf(" %c", &op) == 1) {
    g_raw = false;
    if (op == 'R') {
      g_raw = true;
      if (scanf(" %c", &op) != 1) return 2;
    }
    switch (op) {
      case 'M': {
        const V a = read_v(), b = read_v();
        print_both(W::mul(a, b), T::f12_mul(to_tower(a), to_tower(b)));
        break;
      }
      case 'S': {
        const V a = read_v();
        print_both(W::sqr(a), T::f12_sqr(to_tower(a)));
        break;
      }
      case 'C': {
        const V a = read_v();
        print_both(W::cyclo_sqr(a), T::f12_cyclo_sqr(to_tower(a)));
        break;
      }
      case 'I': {  // conj(a) / (a conj(a)), the way the easy part takes its inverse
        const V a = read_v();
        const V c = W::conj(a);
        print_both(W::mul(c, W::ninv(W::mul(a, c))), T::f12_inv(to_tower(a)));
        break;
      }
      case 'E': {
        const V a = read_v();
        print_both(W::final_exp(a), T::final_exp(to_tower(a)));
        break;
      }
      case 'F': {
        int j = 0;
        if (scanf(" %d", &j) != 1) return 2;
        const V a = read_v();
        print_both(W::frob(a, j), T::f12_frob(to_tower(a), j));
        break;
      }
      case 'N': {
        const V a = read_v();
        const fl s = read_fl();
        const p29::f2 b0 = read_f2(), b1 = read_f2();
        print_both(W::mul_line(a, s, b0, b1), T::f12_mul_line(to_tower(a), s, b0, b1));
        break;
      }
      case 'L': {
        const T::g1_eval p = read_g1();
        const std::vector<p29::line_coeffs> l = read_g2_lines();
        T::g1_eval none = p;
        none.inf = true;
        print_both(W::miller2(l.data(), p, l.data(), none), T::miller2(l.data(), p, l.data(), none));
        break;
      }
      case 'K': {
        const T::g1_eval p1 = read_g1();
        const std::vector<p29::line_coeffs> l1 = read_g2_lines();
        const T::g1_eval p2 = read_g1();
        const std::vector<p29::line_coeffs> l2 = read_g2_lines();
        printf("%d\n%d\n", W::check2(l1.data(), p1, l2.data(), p2) ? 1 : 0,
               T::check2(l1.data(), p1, l2.data(), p2) ? 1 : 0);
        break;
      }
      default: return 3;
    }
    fflush(stdout);
  }
  return 0;
}
