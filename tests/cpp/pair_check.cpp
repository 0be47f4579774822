// Host-side check of the first addition of an accumulation item (G1L::add_affine_pair, cap_amd/csrc/curve29.hpp): two
// affine table points, each with a sign, against add_mixed(add_mixed(inf, q0), q1) compared as affine points; the
// refusal on q1 == +-q0; and the accumulator invariants madd_acc states for what comes out (x < 2p, y < 3p, zz, zzz <
// 1.2p, normalized limbs), followed by a madd_acc chain that starts from the pair.  Built twice by
// tests/test_pair_host.py: with the CAP_FL_CHECK assertions, and with clang++ -fsanitize=unsigned-integer-overflow.
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/curve29.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace cap;

static g1a conv(const g1_affine& p) {
  g1a r;
  if (G1::is_inf(p)) { r.x = Fq29::zero(); r.y = Fq29::zero(); return r; }
  r.x = Fq29::canonical(Fq29::from_ext(p.x));
  r.y = Fq29::canonical(Fq29::from_ext(p.y));
  return r;
}
// x * den < p * num, exactly (limbs of x below 2^32)
static bool below(const fl& x, uint64_t num, uint64_t den) {
  uint64_t a[10] = {0}, b[10] = {0};
  uint64_t ca = 0, cb = 0;
  for (int i = 0; i < 9; i++) {
    uint64_t ta = (uint64_t)x.v[i] * den + ca, tb = (uint64_t)FqP29::MOD[i] * num + cb;
    a[i] = ta & 0x1fffffffu; ca = ta >> 29;
    b[i] = tb & 0x1fffffffu; cb = tb >> 29;
  }
  a[9] = ca; b[9] = cb;
  for (int i = 9; i >= 0; i--) if (a[i] != b[i]) return a[i] < b[i];
  return false;
}
static bool normalized(const fl& x) {
  for (int i = 0; i < 8; i++) if (x.v[i] >> 29) return false;
  return true;
}
template <class G>
static bool invariants(const g1x& a) {
  return normalized(a.x) && normalized(a.y) && normalized(a.zz) && normalized(a.zzz) && below(a.x, 2, 1) &&
         below(a.y, 3, 1) && below(a.zz, 6, 5) && below(a.zzz, 6, 5);
}
template <class G>
static bool same_point(const g1x& a, const g1x& b) {
  const g1a pa = G::to_affine(a), pb = G::to_affine(b);
  if (G::is_inf(a) || G::is_inf(b)) return G::is_inf(a) == G::is_inf(b);
  return G::F::eq(pa.x, pb.x) && G::F::eq(pa.y, pb.y);
}

template <int SCHED>
static int pairs() {
  using G = G1LT<SCHED>;
  const int N = 96;
  std::vector<g1a> pts(N);
  g1_affine g; g.x = Fq::one(); g.y = Fq::dbl(Fq::one());
  g1_xyzz acc = G1::from_affine(g);
  uint32_t s = 777;
  for (int i = 0; i < N; i++) {
    pts[i] = conv(G1::to_affine(acc));
    s = (uint32_t)(((uint64_t)s * 1103515245ull + 12345ull) % 2147483648ull);
    const int reps = 1 + (int)(s % 5);
    for (int k = 0; k < reps; k++) acc = G1::add_mixed(acc, g);
    acc = G1::dbl(acc);
  }
  int bad = 0;
  for (int i = 0; i < N; i++) {
    const g1a &q0 = pts[i], &q1 = pts[(i * 7 + 3) % N == i ? (i + 1) % N : (i * 7 + 3) % N];
    for (int sg = 0; sg < 4; sg++) {
      const bool n0 = sg & 1, n1 = (sg & 2) != 0;
      g1x out = G::inf();
      if (!G::add_affine_pair(out, q0, n0, q1, n1)) { bad++; if (bad < 5) printf("pair %d/%d refused\n", i, sg); continue; }
      if (!invariants<G>(out)) { bad++; if (bad < 5) printf("pair %d/%d: invariants\n", i, sg); }
      const g1x ref = G::add_mixed(G::add_mixed(G::inf(), q0, n0), q1, n1);
      if (!same_point<G>(out, ref)) { bad++; if (bad < 5) printf("pair %d/%d differs\n", i, sg); }
      // the item goes on with madd_acc, and its result goes through the 32-byte image
      g1x a = out, b = ref;
      for (int k = 0; k < 3; k++) {
        const g1a& q = pts[(i + 11 * (k + 1)) % N];
        const bool ng = ((i + k + sg) % 3) == 0;
        if (!G::madd_acc(a, q, ng)) a = G::add_mixed(a, q, ng);
        b = G::add_mixed(b, q, ng);
        if (!invariants<G>(a)) { bad++; if (bad < 5) printf("pair %d/%d: invariants after madd_acc %d\n", i, sg, k); }
      }
      a = G::load(G::store(a));
      if (!same_point<G>(a, b)) { bad++; if (bad < 5) printf("chain %d/%d differs\n", i, sg); }
    }
    // q1 == +-q0: refused, out untouched
    for (int sg = 0; sg < 4; sg++) {
      g1x out = G::inf();
      out.x.v[0] = 12345;
      if (G::add_affine_pair(out, q0, sg & 1, q0, (sg & 2) != 0) || out.x.v[0] != 12345 || !G::is_inf(out)) {
        bad++;
        if (bad < 5) printf("pair %d/%d: equal x not refused\n", i, sg);
      }
    }
  }
  // extreme canonical coordinates: only the integer arithmetic is exercised (nothing may wrap, every contract holds)
  {
    g1a lo, hi;
    lo.x = G::F::zero(); lo.y = G::F::zero(); lo.x.v[0] = 1; lo.y.v[0] = 1;
    for (int i = 0; i < 9; i++) hi.x.v[i] = hi.y.v[i] = FqP29::MOD[i];
    hi.x.v[0] -= 1; hi.y.v[0] -= 2;   // p - 1, p - 2
    const g1a* ops[2] = {&lo, &hi};
    for (int a = 0; a < 2; a++)
      for (int sg = 0; sg < 4; sg++) {
        g1x out = G::inf();
        if (!G::add_affine_pair(out, *ops[a], sg & 1, *ops[1 - a], (sg & 2) != 0) || !invariants<G>(out)) {
          bad++;
          printf("extreme operands %d/%d\n", a, sg);
        }
      }
  }
  return bad;
}

int main() {
  int bad = pairs<0>() + pairs<1>();
  printf("bad=%d\n", bad);
  return bad != 0;
}
