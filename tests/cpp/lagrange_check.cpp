// Host twin of the Lagrange key builder: the functions of cap_amd/csrc/lagrange_elem29.hpp - what the lanes of
// lag_load, lag_stage and lag_finish execute - with the bound assertions of field29.hpp on (CAP_FL_CHECK), driven by
// tests/test_lagrange_host.py.  Points come in and go out as the C ABI holds them: affine, 2 x 256 bits in arkworks'
// Montgomery form, (0, 0) for infinity; scalars are canonical integers.  All numbers are hex words on stdin / stdout.
//
//   lagrange_check scalar      lines "x y form k":  [k] B, B = P (form 0), 2P held with zz != 1 (form 1), or infinity held
//                              with non-zero x, y and zz = 0 (form 2, what a cancelled sum looks like)
//   lagrange_check transform   "log_n", then n + 3 lines "x y" (the SRS), max(n / 2, 1) twiddles omega^-k, then 1/n:
//                              the whole build, lanes emulated as loops between the launches, every point going through
//                              the g1_xyzz memory image between two stages
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/lagrange_elem29.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace cap;

static bool read_fe(fe& out) {
  char buf[128];
  if (scanf("%100s", buf) != 1) return false;
  std::string s(buf);
  if (s.size() > 64) return false;
  s = std::string(64 - s.size(), '0') + s;
  for (int w = 0; w < 8; w++) out.v[w] = (uint32_t)strtoul(s.substr(64 - 8 * (w + 1), 8).c_str(), nullptr, 16);
  return true;
}
static void print_fe(const fe& a, char end) {
  for (int w = 7; w >= 0; w--) printf("%08x", a.v[w]);
  putchar(end);
}
static bool read_point(g1_affine& p) { return read_fe(p.x) && read_fe(p.y); }
// arkworks' form -> the internal canonical form of an MSM table's window-0 row (msm.hip: what lag_load reads)
static g1_affine to_table(const g1_affine& p) {
  g1a r;
  if (G1::is_inf(p)) {
    r.x = Fq29::zero();
    r.y = Fq29::zero();
  } else {
    r.x = Fq29::canonical(Fq29::from_ext(p.x));
    r.y = Fq29::canonical(Fq29::from_ext(p.y));
  }
  return G1L::store_affine(r);
}
static void print_out(const g1x& p) {  // as lag_finish writes a point
  g1_affine o;
  if (G1L::is_inf(p)) {
    o.x = Fq::zero();
    o.y = Fq::zero();
  } else {
    const g1a q = G1L::to_affine(p);
    o.x = Fq29::to_ext(q.x);
    o.y = Fq29::to_ext(q.y);
  }
  print_fe(o.x, ' ');
  print_fe(o.y, '\n');
}

static int run_scalar() {
  g1_affine p;
  fe form, k;
  while (read_point(p)) {
    if (!read_fe(form) || !read_fe(k)) return 2;
    g1x b = G1L::from_affine(G1L::load(to_table(p)));
    if (form.v[0] == 1) b = G1L::dbl(b);
    if (form.v[0] == 2) b.zz = b.zzz = Fq29::zero();
    b = G1L::load(G1L::store(b));
    print_out(Lag::scalar_mul(b, k));
  }
  return 0;
}

static int run_transform() {
  fe w;
  while (read_fe(w)) {
    const uint32_t log_n = w.v[0];
    if (log_n > 12) return 2;
    const uint32_t n = 1u << log_n;
    std::vector<g1_affine> srs(n + kLagBlind);
    for (auto& p : srs) {
      if (!read_point(p)) return 2;
      p = to_table(p);
    }
    std::vector<fe> tw(n / 2 ? n / 2 : 1);
    for (auto& t : tw)
      if (!read_fe(t)) return 2;
    fe n_inv;
    if (!read_fe(n_inv)) return 2;
    std::vector<g1_xyzz> a(n);
    for (uint32_t i = 0; i < n; i++) a[Lag::bitrev(i, log_n)] = Lag::load_point(srs[i]);  // lag_load
    for (uint32_t half = 1; half < n; half <<= 1) {                                        // one lag_stage launch each
      const uint32_t step = n / (2 * half);
      for (uint32_t t = 0; t < n / 2; t++) {
        const uint32_t j = t & (half - 1), i0 = ((t - j) << 1) + j, i1 = i0 + half;
        Lag::butterfly(a[i0], a[i1], tw[(size_t)j * step], j != 0, a[i0], a[i1]);
      }
    }
    for (uint32_t j = 0; j < n + kLagBlind; j++) {                                         // lag_finish
      g1_affine o;
      Lag::finish(a.data(), n, n_inv, srs.data(), j, o);
      print_fe(o.x, ' ');
      print_fe(o.y, '\n');
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "scalar")) return run_scalar();
  if (argc == 2 && !strcmp(argv[1], "transform")) return run_transform();
  fprintf(stderr, "usage: lagrange_check scalar|transform < records\n");
  return 2;
}
