// Host-side check of cap_amd/csrc/pairing29.hpp (tower arithmetic, prepared-line Miller loop, final exponentiation) with
// field29.hpp's bound assertions enabled.  Reads one operation per line on stdin, plain hex integers, prints the result;
// tests/test_pairing29_host.py compares with oracle/pairing.py.  An Fq12 is 12 integers: for k = 0..5 the Fq2
// coefficient (x, y) of w^k in the tower (x + y u).  A G1 point is (x, y), (0, 0) = infinity; a G2 point (x0, x1, y0, y1).
//   M a b | S a | C a | I a | E a | F j a   product, squaring, cyclotomic squaring, inverse, final exponentiation, Frobenius
//   L P Q        the prepared-line Miller loop of one pair (before the final exponentiation)
//   P P Q        e(P, Q) after the final exponentiation
//   K P1 Q1 P2 Q2  1 if e(P1, Q1) e(P2, Q2) == 1 else 0
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/pairing29.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace cap;
using T = p29::Tower<CAP_FL_SCHED>;
using F = T::F;

static fe read_fe() {
  char s[160];
  if (scanf(" %159s", s) != 1) exit(2);
  fe r;
  memset(&r, 0, sizeof r);
  const int n = (int)strlen(s);
  for (int i = 0; i < n; i++) {
    const int d = n - 1 - i;  // nibble index from the low end
    char c = s[i];
    uint32_t v = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    r.v[d / 8] |= v << (4 * (d % 8));
  }
  return r;
}
static void print_fe(const fe& a) {
  for (int i = 7; i >= 0; i--) printf("%08x", a.v[i]);
}
static fl read_fl() { return F::to_mont(read_fe()); }
static void print_fl(const fl& a) {
  print_fe(F::from_mont(a));
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
static p29::f12 read_f12() {
  p29::f12 a;
  for (int k = 0; k < 6; k++) *slot(a, k) = read_f2();
  return a;
}
static void print_f12(p29::f12 a) {
  for (int k = 0; k < 6; k++) {
    print_fl(slot(a, k)->c0);
    print_fl(slot(a, k)->c1);
  }
  printf("\n");
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
    switch (op) {
      case 'M': {
        p29::f12 a = read_f12(), b = read_f12();
        print_f12(T::f12_mul(a, b));
        break;
      }
      case 'S': print_f12(T::f12_sqr(read_f12())); break;
      case 'C': print_f12(T::f12_cyclo_sqr(read_f12())); break;
      case 'I': print_f12(T::f12_inv(read_f12())); break;
      case 'E': print_f12(T::final_exp(read_f12())); break;
      case 'F': {
        int j = 0;
        if (scanf(" %d", &j) != 1) return 2;
        print_f12(T::f12_frob(read_f12(), j));
        break;
      }
      case 'L':
      case 'P': {
        const T::g1_eval p = read_g1();
        const std::vector<p29::line_coeffs> l = read_g2_lines();
        T::g1_eval none = p;
        none.inf = true;
        p29::f12 f = T::miller2(l.data(), p, l.data(), none);
        print_f12(op == 'L' ? f : T::final_exp(f));
        break;
      }
      case 'K': {
        const T::g1_eval p1 = read_g1();
        const std::vector<p29::line_coeffs> l1 = read_g2_lines();
        const T::g1_eval p2 = read_g1();
        const std::vector<p29::line_coeffs> l2 = read_g2_lines();
        printf("%d\n", T::check2(l1.data(), p1, l2.data(), p2) ? 1 : 0);
        break;
      }
      default: return 3;
    }
    fflush(stdout);
  }
  return 0;
}
