// Host twin of the round kernels' arithmetic (cap_amd/csrc/round_elem29.hpp: the bodies of k_perm_numden, k_kx_columns,
// k_quotient<FOLD>, k_lincomb, and ColAcc) with the bound assertions of field29.hpp on, and the same templates on the
// bound-tracking field (bound29.hpp).  Driven by tests/test_round_elem_host.py:
//   round_elem_check envelope [SEVENTH]  every body with every operand at its contract's maximum - any 32-byte image - on
//                                        the bound field: the bound of every value that leaves, as JSON; exit code 2 if a
//                                        precondition failed.  SEVENTH = 1 adds a seventh product before ColAcc::reduce
//                                        (what the envelope exists to catch; the test expects it to fail)
//   round_elem_check run SCHED           rows on stdin, one per line (hex images, layouts below); the results on stdout
#define CAP_FL_CHECK 1
#include "../hip/elemcheck_ops.hpp"
#include "bound29.hpp"

#include <string>
#include <vector>

using namespace cap;
using capbound::bfe;
using capbound::bfl;
using BF = capbound::BoundFl<FrP29>;

// ---- envelope --------------------------------------------------------------------------------------------------------------------
static int envelope(bool seventh) {
  capbound::BoundLog::fatal() = false;
  const bfe any = BF::image_256();
  printf("{\"rounds\": {");
  capbound::BoundLog::where() = "k_perm_numden";
  {
    const bfe k[5] = {any, any, any, any, any};
    bfe num, den;
    perm_numden_row<BF, bfl, bfe>(any, any, any, k, [&](int) -> const bfe& { return any; },
                                  [&](int) -> const bfe& { return any; }, num, den);
    printf("\"k_perm_numden\": {\"num\": %llu, \"den\": %llu}", (unsigned long long)num.mag, (unsigned long long)den.mag);
  }
  capbound::BoundLog::where() = "k_kx_columns";
  printf(", \"k_kx_columns\": {\"out\": %llu}", (unsigned long long)kx_elem<BF, bfl, bfe>(any, BF::load(any)).mag);
  ChalT<bfe> ch = {any, any, any, any, any, any};
  QuotConstT<bfe> qc;
  qc.g = any;
  for (int i = 0; i < 5; i++) qc.k[i] = any;
  for (int i = 0; i < 8; i++) qc.zh_inv[i] = any;
  const PointT<bfe> at = {&any, &any, &any, 0};
  auto img = [&](int) -> const bfe& { return any; };
  capbound::BoundLog::where() = "k_quotient<true>";
  printf(", \"k_quotient_fold\": {\"out\": %llu}",
         (unsigned long long)quotient_point<true, BF, bfl, bfe>(img, img, at, ch, qc).mag);
  capbound::BoundLog::where() = "k_quotient<false>";
  printf(", \"k_quotient_direct\": {\"out\": %llu}",
         (unsigned long long)quotient_point<false, BF, bfl, bfe>(img, img, at, ch, qc).mag);
  capbound::BoundLog::where() = "k_lincomb";
  {
    // the prover's 29 terms, and 30: five full groups of six
    std::vector<bfe> s(30, any), v(30, any);
    std::vector<int> on(30, 1);
    const uint64_t a = lincomb_elem<BF, bfl, bfe>(29, TermsT<bfe>{s.data(), v.data(), on.data(), 29}).mag;
    const uint64_t b = lincomb_elem<BF, bfl, bfe>(30, TermsT<bfe>{s.data(), v.data(), on.data(), 30}).mag;
    printf(", \"k_lincomb\": {\"out_29_terms\": %llu, \"out_30_terms\": %llu}", (unsigned long long)a, (unsigned long long)b);
  }
  capbound::BoundLog::where() = "ColAcc";
  {
    ColAcc<BF, bfl> acc;
    acc.clear();
    const bfl x = BF::load(any);
    for (int i = 0; i < (seventh ? 7 : 6); i++) acc.mad(x, x);
    printf(", \"ColAcc\": {\"products\": %d, \"reduced\": %llu}", seventh ? 7 : 6, (unsigned long long)acc.reduce().mag);
  }
  printf("}}\n");
  return capbound::BoundLog::failures() ? 2 : 0;
}

// ---- run: concrete rows -------------------------------------------------------------------------------------------------------
// P beta gamma tw k[5] wire[5] sig[5]                              -> num den
// K k x                                                            -> k x
// Q fold zi sel[22] col[6] z_next x inv_nx1 chal[6] k[5] zh_inv[8] -> t
// L n (on scalar value)[n]                                         -> sum
// S n (a b)[n]   n <= 6 products of images through ColAcc          -> nine limbs of the reduced sum
static bool rd_img(fe& o) {
  char buf[80];
  if (scanf("%79s", buf) != 1) return false;
  const std::string h(buf);
  for (int w = 0; w < 8; w++) o.v[w] = 0;
  int nib = 0;
  for (int i = (int)h.size() - 1; i >= 0 && nib < 64; i--, nib++) {
    const char c = h[i];
    const uint32_t d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    o.v[nib / 8] |= d << (4 * (nib % 8));
  }
  return true;
}
static void pr_img(const fe& a) {
  for (int w = 7; w >= 0; w--) printf("%08x", a.v[w]);
}
template <class F>
static int run_rows() {
  char kind[4];
  while (scanf("%3s", kind) == 1) {
    if (kind[0] == 'P') {
      fe in[18], num, den;
      for (auto& x : in)
        if (!rd_img(x)) return 3;
      perm_numden_row<F, fl, fe>(in[0], in[1], in[2], in + 3, [&](int i) -> const fe& { return in[8 + i]; },
                                 [&](int i) -> const fe& { return in[13 + i]; }, num, den);
      pr_img(num);
      printf(" ");
      pr_img(den);
      printf("\n");
    } else if (kind[0] == 'K') {
      fe k, x;
      if (!rd_img(k) || !rd_img(x)) return 3;
      pr_img(kx_elem<F, fl, fe>(k, F::load(x)));
      printf("\n");
    } else if (kind[0] == 'Q') {
      int fold;
      uint32_t zi;
      if (scanf("%d %u", &fold, &zi) != 2 || zi > 7) return 3;
      fe in[50];
      for (auto& x : in)
        if (!rd_img(x)) return 3;
      const ChalT<fe> ch = {in[31], in[32], in[33], in[34], in[35], in[36]};
      QuotConstT<fe> qc;
      qc.g = in[0];
      for (int i = 0; i < 5; i++) qc.k[i] = in[37 + i];
      for (int i = 0; i < 8; i++) qc.zh_inv[i] = in[42 + i];
      const PointT<fe> at = {&in[28], &in[29], &in[30], zi};
      auto sel = [&](int s) -> const fe& { return in[s]; };
      auto col = [&](int j) -> const fe& { return in[22 + j]; };
      pr_img(fold ? quotient_point<true, F, fl, fe>(sel, col, at, ch, qc)
                  : quotient_point<false, F, fl, fe>(sel, col, at, ch, qc));
      printf("\n");
    } else if (kind[0] == 'L' || kind[0] == 'S') {
      uint32_t n;
      if (scanf("%u", &n) != 1 || n > 64) return 3;
      std::vector<fe> s(n + 1), v(n + 1);
      std::vector<int> on(n + 1, 1);
      for (uint32_t t = 0; t < n; t++) {
        if (kind[0] == 'L' && scanf("%d", &on[t]) != 1) return 3;
        if (!rd_img(s[t]) || !rd_img(v[t])) return 3;
      }
      if (kind[0] == 'L') {
        pr_img(lincomb_elem<F, fl, fe>(n, TermsT<fe>{s.data(), v.data(), on.data(), n}));
      } else {
        if (n > 6) return 3;
        ColAcc<F, fl> acc;
        acc.clear();
        for (uint32_t t = 0; t < n; t++) acc.mad(F::load(s[t]), F::load(v[t]));
        const fl r = acc.reduce();
        for (int i = 0; i < 9; i++) printf("%x ", r.v[i]);
      }
      printf("\n");
    } else {
      return 3;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "envelope") return envelope(argc > 2 && atoi(argv[2]) == 1);
  if (mode == "run" && argc == 3) return atoi(argv[2]) ? run_rows<Fl<FrP29, 1>>() : run_rows<Fl<FrP29, 0>>();
  fprintf(stderr, "usage: round_elem_check envelope [SEVENTH] | run SCHED\n");
  return 3;
}
