// Host twin of the NTT kernels' arithmetic (cap_amd/csrc/ntt_elem29.hpp) with the bound assertions of field29.hpp on,
// and the same templates on the bound-tracking field (bound29.hpp).  Driven by tests/test_ntt_elem_host.py:
//   ntt_elem_check envelope              the bound of every store to LDS and to memory per twiddle form, sub-transform
//                                        length and input class, as JSON; exit code 2 if a precondition failed
//   ntt_elem_check run SCHED SHOUP IN OUT   whole tile transforms and the element steps on the cases of file IN (32-bit
//                                        little-endian words, layout below); raw results and the largest value in the
//                                        tile after every stage to OUT
//   ntt_elem_check elem SCHED IN OUT     the records of tests/hip/elemcheck_ops.hpp (single butterflies, element steps):
//                                        the host's words for tests/test_gpu_elemcheck.py to compare the device's with
//   ntt_elem_check ops                   "op sched operand.." lines on stdin: the real operation and the bound
//                                        operation side by side (the per-operation check of the bound table)
#define CAP_FL_CHECK 1
#include "../hip/elemcheck_ops.hpp"
#include "bound29.hpp"

#include <cstring>
#include <string>
#include <vector>

using namespace cap;
using capbound::bfe;
using capbound::bfl;
using BF = capbound::BoundFl<FrP29>;

static const uint32_t kThreads = 256;  // as in ntt.hip; the stage functions see the same (tid, nthreads)

static uint32_t bitrev(uint32_t x, uint32_t bits) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
  return r;
}

// ---- whole tiles through the shared stage functions ---------------------------------------------------------------------
// after(stage) is called behind the input step and behind every barrier
template <class F, class V, bool SHOUP, class After>
static void run_stages(V* sh, const V* tw, uint32_t log_len, uint32_t log_c, After after) {
  const uint32_t s0 = log_len & 1;
  if (s0) {
    for (uint32_t tid = 0; tid < kThreads; tid++) ntt_stage_radix2<F, V>(sh, log_len, log_c, tid, kThreads);
    after();
  }
  for (uint32_t s = s0; s + 1 < log_len; s += 2) {
    for (uint32_t tid = 0; tid < kThreads; tid++) ntt_stage_radix4<F, V, SHOUP>(sh, tw, log_len, log_c, s, tid, kThreads);
    after();
  }
}

// the output forms of the plans (PassParams): column pass with / without the inter-pass product, row pass canonical,
// post-scaled (table or scalar: the same arithmetic, the scalar shared), lazy_out with and without the product
enum { OUT_COL_TW = 0, OUT_COL_TW_SCALED, OUT_ROW, OUT_ROW_POST, OUT_ROW_SCALAR, OUT_ROW_POST_LAZY, OUT_ROW_LAZY, OUT_FORMS };
static const char* kOutNames[OUT_FORMS] = {"col_tw", "col_tw_scaled", "row_canonical", "row_post_scale", "row_post_scalar",
                                           "row_post_scale_lazy_out", "row_lazy_out"};
template <class F, class V, class W>
static W out_step(int form, const V& x, bool first_row, const W& f) {
  switch (form) {
    case OUT_COL_TW: return ntt_out_col<F, V, W>(x, !first_row, f);  // exponent 0: no product, a weak reduction
    case OUT_COL_TW_SCALED: return ntt_out_col<F, V, W>(x, true, f);
    case OUT_ROW: return ntt_out_row<F, V, W>(x, false);
    case OUT_ROW_POST:
    case OUT_ROW_SCALAR: return ntt_out_row<F, V, W>(ntt_scale_elem<F, V, W>(x, f), false);
    case OUT_ROW_POST_LAZY: return ntt_out_row<F, V, W>(ntt_scale_elem<F, V, W>(x, f), true);
    default: return ntt_out_row<F, V, W>(x, true);
  }
}

// ---- run: concrete cases ------------------------------------------------------------------------------------------------------
// file IN:  ncases, then per case: log_len, log_c, in_form (0 none, 1 pre-scale, 2 pre-scale + fold), index;
//           plain canonical twiddles omega^i, i < len / 2 (8 words each); raw[c][j]; in_form >= 1: pre[c][j];
//           in_form == 2: fold_raw[c][j], fold_pre[c][j]; out_factor[k][c].  Element (k, c) leaves in output form
//           (k + c + index) mod 7.
// file OUT: per case: number of records n, n x 9 limbs (the largest value in the tile behind the input step and behind
//           every stage), then out[k][c] (8 words each)
static bool rd(FILE* f, void* p, size_t words) { return fread(p, 4, words, f) == words; }
static bool fl_less(const fl& a, const fl& b) {
  for (int i = 8; i >= 0; i--)
    if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
  return false;
}
template <class F, bool SHOUP>
static int run_cases(FILE* in, FILE* out) {
  uint32_t ncases;
  if (!rd(in, &ncases, 1)) return 3;
  for (uint32_t cs = 0; cs < ncases; cs++) {
    uint32_t h[4];
    if (!rd(in, h, 4)) return 3;
    const uint32_t log_len = h[0], log_c = h[1], in_form = h[2], index = h[3];
    if (log_len < 1 || log_len + log_c > 11 || in_form > 2) return 3;  // what fits the LDS tile of the kernels
    const uint32_t len = 1u << log_len, C = 1u << log_c, tile = len << log_c, cmask = C - 1;
    std::vector<fe> w(len / 2), raw(tile), pre, fraw, fpre, outf(tile);
    if (!rd(in, w.data(), 8 * w.size()) || !rd(in, raw.data(), 8 * (size_t)tile)) return 3;
    if (in_form >= 1) {
      pre.resize(tile);
      if (!rd(in, pre.data(), 8 * (size_t)tile)) return 3;
    }
    if (in_form == 2) {
      fraw.resize(tile);
      fpre.resize(tile);
      if (!rd(in, fraw.data(), 8 * (size_t)tile) || !rd(in, fpre.data(), 8 * (size_t)tile)) return 3;
    }
    if (!rd(in, outf.data(), 8 * (size_t)tile)) return 3;
    // tw_small as table_unpack (ntt.hip) builds it from the canonical internal-form table
    std::vector<fl> tw(w.size() * NttTw<F, fl, SHOUP>::kStride);
    for (size_t i = 0; i < w.size(); i++) {
      const fl t = F::canonical(F::to_mont(w[i]));
      if (SHOUP) {
        tw[2 * i] = F::load(F::from_mont(t));
        tw[2 * i + 1] = F::shoup_quotient(t);
      } else {
        tw[i] = t;
      }
    }
    std::vector<fl> sh(tile);
    fe dummy = raw[0];
    for (uint32_t e = 0; e < tile; e++) {
      const uint32_t c = e & cmask, j = e >> log_c;
      const size_t at = (size_t)c * len + j;
      sh[(bitrev(j, log_len) << log_c) + c] =
          ntt_in_elem<F, fl, fe>(raw[at], in_form >= 1, in_form >= 1 ? pre[at] : dummy, in_form == 2,
                                 in_form == 2 ? fraw.data() : &dummy, in_form == 2 ? at : 0, in_form == 2 ? fpre.data() : &dummy,
                                 in_form == 2 ? at : 0);
    }
    std::vector<fl> maxima;
    auto after = [&] {
      fl m = sh[0];
      for (uint32_t e = 1; e < tile; e++)
        if (fl_less(m, sh[e])) m = sh[e];
      maxima.push_back(m);
    };
    after();
    run_stages<F, fl, SHOUP>(sh.data(), tw.data(), log_len, log_c, after);
    const uint32_t n = (uint32_t)maxima.size();
    fwrite(&n, 4, 1, out);
    fwrite(maxima.data(), 36, n, out);
    for (uint32_t e = 0; e < tile; e++) {
      const uint32_t c = e & cmask, k = e >> log_c;
      const fe o = out_step<F, fl, fe>((int)((k + c + index) % OUT_FORMS), sh[e], k == 0, outf[e]);
      fwrite(&o, 32, 1, out);
    }
  }
  return 0;
}

// ---- envelope ------------------------------------------------------------------------------------------------------------------
struct InClass {
  const char* name;
  int kind;  // 0: image of magnitude mag; 1: pre-scaled; 2: pre-scaled + fold; 3: raw below, zero in the upper half
  uint64_t mag;
};
template <bool SHOUP>
static void envelope_form(bool first_form) {
  static const InClass classes[] = {{"packed_2p", 0, 2 * BF::U},   {"raw_256", 0, BF::C256 + 1},
                                    {"lazy_store", 0, 2 * BF::U},  {"pre_scaled", 1, BF::C256 + 1},
                                    {"pre_scaled_fold", 2, BF::C256 + 1}, {"zero_padded", 3, BF::C256 + 1}};
  printf("%s\"%s\": {", first_form ? "" : ", ", SHOUP ? "shoup" : "montgomery");
  for (uint32_t log_len = 1; log_len <= 11; log_len++) {
    printf("%s\"%u\": {", log_len > 1 ? ", " : "", log_len);
    const uint32_t len = 1u << log_len;
    std::vector<bfl> tw(len / 2 * NttTw<BF, bfl, SHOUP>::kStride);
    for (size_t i = 0; i < tw.size(); i++) tw[i] = (SHOUP && (i & 1)) ? BF::quotient() : BF::twiddle();
    for (size_t ci = 0; ci < sizeof(classes) / sizeof(classes[0]); ci++) {
      const InClass& cl = classes[ci];
      static char where[96];
      snprintf(where, sizeof(where), "%s log_len %u %s", SHOUP ? "shoup" : "montgomery", log_len, cl.name);
      capbound::BoundLog::where() = where;
      // pre-scale and post-scale factors: any 32 bytes (a caller's table); inter-pass twiddles: the domain's, canonical
      const bfe img = BF::image(cl.mag), any = BF::image(BF::C256 + 1), canon = BF::image(BF::U), none = bfe();
      std::vector<bfl> sh(len);
      for (uint32_t j = 0; j < len; j++) {
        const bool padded = cl.kind == 3 && j >= len / 2;
        sh[bitrev(j, log_len)] = ntt_in_elem<BF, bfl, bfe>(padded ? none : img, cl.kind == 1 || cl.kind == 2, any,
                                                           cl.kind == 2, &any, 0, &any, 0);
      }
      std::vector<uint64_t> lds;
      auto after = [&] {
        uint64_t m = 0;
        for (uint32_t e = 0; e < len; e++) m = sh[e].mag > m ? sh[e].mag : m;
        lds.push_back(m);
      };
      after();
      run_stages<BF, bfl, SHOUP>(sh.data(), tw.data(), log_len, 0, after);
      printf("%s\"%s\": {\"lds\": [", ci ? ", " : "", cl.name);
      for (size_t i = 0; i < lds.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)lds[i]);
      printf("], \"mem\": {");
      for (int form = 0; form < OUT_FORMS; form++) {
        uint64_t m = 0;
        for (uint32_t k = 0; k < len; k++) {
          const bfe o = out_step<BF, bfl, bfe>(form, sh[k], k == 0, form <= OUT_COL_TW_SCALED ? canon : any);
          m = o.mag > m ? o.mag : m;
        }
        printf("%s\"%s\": %llu", form ? ", " : "", kOutNames[form], (unsigned long long)m);
      }
      printf("}}");
    }
    printf("}");
  }
  printf("}");
}

// the radix-3 stage and the five-coset solve on the bound field, every operand any 32-byte image
struct BoundQuot5 {
  bfe odd[2][2], even[3][5], mt[5], d[5];
};
static void envelope_combine() {
  capbound::BoundLog::where() = "ntt3_combine";
  const bfe any = BF::image(BF::C256 + 1);
  bfl x0, x1, x2;
  ntt3_combine_elem<BF, bfl, bfe>(any, any, any, any, any, any, x0, x1, x2);
  printf(", \"ntt3_combine\": {\"x0\": %llu, \"x1\": %llu, \"x2\": %llu", (unsigned long long)x0.mag,
         (unsigned long long)x1.mag, (unsigned long long)x2.mag);
  const bfl xs[3] = {x0, x1, x2};
  uint64_t st = 0, fin = 0, fin_add = 0;
  for (int i = 0; i < 3; i++) {
    const uint64_t a = BF::store(xs[i]).mag, b = ntt3_finish_elem<BF, bfl, bfe>(xs[i], any, false, BF::zero()).mag,
                   c = ntt3_finish_elem<BF, bfl, bfe>(xs[i], any, true, BF::load(any)).mag;
    st = a > st ? a : st;
    fin = b > fin ? b : fin;
    fin_add = c > fin_add ? c : fin_add;
  }
  printf(", \"mem_store\": %llu, \"mem_post\": %llu, \"mem_post_add\": %llu}", (unsigned long long)st,
         (unsigned long long)fin, (unsigned long long)fin_add);
  capbound::BoundLog::where() = "ntt3_combine5";
  BoundQuot5 qc;
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2; j++) qc.odd[i][j] = any;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 5; j++) qc.even[i][j] = any;
  for (int j = 0; j < 5; j++) qc.mt[j] = qc.d[j] = any;
  using E = Ntt5Elem<BF, bfl, bfe, BoundQuot5>;
  const bfl v = ntt_scale_elem<BF, bfl, bfe>(BF::load(any), any), pi = BF::load(any), h = BF::load(any);
  uint64_t m5 = 0;
  for (int add = 0; add < 2; add++)
    for (int top = 0; top < 2; top++) {
      for (int jj = 0; jj < 2; jj++) {
        const uint64_t m = E::odd(jj, v, v, add, pi, top, h, qc).mag;
        m5 = m > m5 ? m : m5;
      }
      for (int jj = 0; jj < 3; jj++) {
        const uint64_t m = E::even(jj, v, v, v, v, v, add, pi, top, h, qc).mag;
        m5 = m > m5 ? m : m5;
      }
    }
  printf(", \"ntt3_combine5\": {\"unscaled\": %llu, \"mem\": %llu}", (unsigned long long)v.mag, (unsigned long long)m5);
}

// ---- ops: the real operation and the bound operation side by side ----------------------------------------------------------
// line: op sched n, then n operands "L v0 .. v8 lo hi mag zero" (limbs) or "E w0 .. w7 mag zero" (image), all hex.
// prints "L v0 .. v8 lo hi mag" or "E w0 .. w7 mag" (hex)
struct Operand {
  fl l;
  fe e;
  bfl bl;
  bfe be;
};
template <class F>
static bool one_op(const std::string& op, const Operand* x) {
  fl r;
  bfl br;
  fe re;
  bfe bre;
  bool image = false;
#define OP1(name) if (op == #name) { r = F::name(x[0].l); br = BF::name(x[0].bl); } else
#define OP2(name) if (op == #name) { r = F::name(x[0].l, x[1].l); br = BF::name(x[0].bl, x[1].bl); } else
  OP1(normalize) OP1(weak_reduce) OP1(canonical) OP1(neg) OP1(sqr) OP1(neg_lazy) OP1(neg2p_lazy) OP1(neg4p_lazy)
  OP2(add) OP2(add_norm) OP2(sub) OP2(sub2p) OP2(sub2p_lazy) OP2(sub8p) OP2(sub8p_lazy) OP2(sub_from_lazy) OP2(mul)
  if (op == "mul_shoup") {
    // x[1] the plain canonical constant; its pair as the tables derive it
    const fl t = F::canonical(F::to_mont(F::pack(x[1].l)));
    r = F::mul_shoup(x[0].l, x[1].l, F::shoup_quotient(t));
    br = BF::mul_shoup(x[0].bl, x[1].bl, BF::quotient());
  } else if (op == "mul_add_mul") {
    r = F::mul_add_mul(x[0].l, x[1].l, x[2].l, x[3].l);
    br = BF::mul_add_mul(x[0].bl, x[1].bl, x[2].bl, x[3].bl);
  } else if (op == "load") {
    r = F::load(x[0].e);
    br = BF::load(x[0].be);
  } else if (op == "from_ext") {
    r = F::from_ext(x[0].e);
    br = BF::from_ext(x[0].be);
  } else if (op == "pack") {
    re = F::pack(x[0].l);
    bre = BF::pack(x[0].bl);
    image = true;
  } else if (op == "store") {
    re = F::store(x[0].l);
    bre = BF::store(x[0].bl);
    image = true;
  } else if (op == "to_ext") {
    re = F::to_ext(x[0].l);
    bre = BF::to_ext(x[0].bl);
    image = true;
  } else {
    return false;
  }
#undef OP1
#undef OP2
  if (image) {
    printf("E");
    for (int i = 0; i < 8; i++) printf(" %x", re.v[i]);
    printf(" %llx\n", (unsigned long long)bre.mag);
  } else {
    printf("L");
    for (int i = 0; i < 9; i++) printf(" %x", r.v[i]);
    printf(" %llx %llx %llx\n", (unsigned long long)br.lo, (unsigned long long)br.hi, (unsigned long long)br.mag);
  }
  return true;
}
static int run_ops() {
  char op[32];
  int sched, n;
  while (scanf("%31s %d %d", op, &sched, &n) == 3) {
    Operand x[4];
    if (n < 1 || n > 4) return 3;
    for (int i = 0; i < n; i++) {
      char kind[4];
      unsigned long long lo, hi, mag;
      int z;
      if (scanf("%3s", kind) != 1) return 3;
      if (kind[0] == 'L') {
        for (int k = 0; k < 9; k++)
          if (scanf("%x", &x[i].l.v[k]) != 1) return 3;
        if (scanf("%llx %llx %llx %d", &lo, &hi, &mag, &z) != 4) return 3;
        x[i].bl.lo = lo, x[i].bl.hi = hi, x[i].bl.mag = mag, x[i].bl.zero = z != 0;
      } else {
        for (int k = 0; k < 8; k++)
          if (scanf("%x", &x[i].e.v[k]) != 1) return 3;
        if (scanf("%llx %d", &mag, &z) != 2) return 3;
        x[i].be.mag = mag, x[i].be.zero = z != 0;
      }
    }
    const bool ok = sched ? one_op<Fl<FrP29, 1>>(op, x) : one_op<Fl<FrP29, 0>>(op, x);
    if (!ok) {
      fprintf(stderr, "unknown op %s\n", op);
      return 3;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "envelope") {
    capbound::BoundLog::fatal() = false;  // list every violated precondition, then fail
    printf("{\"unit_per_p\": %llu, \"constants\": {\"C256\": %llu, \"C261\": %llu, \"C262\": %llu, \"RT\": %llu, \"RQ\": %llu}, "
           "\"ntt\": {",
           (unsigned long long)BF::U, (unsigned long long)BF::C256, (unsigned long long)BF::C261,
           (unsigned long long)BF::C262, (unsigned long long)BF::RT, (unsigned long long)BF::RQ);
    envelope_form<true>(true);
    envelope_form<false>(false);
    printf("}");
    envelope_combine();
    printf("}\n");
    return capbound::BoundLog::failures() ? 2 : 0;
  }
  if (mode == "run" && argc == 6) {
    const int sched = atoi(argv[2]), shoup = atoi(argv[3]);
    FILE* in = fopen(argv[4], "rb");
    FILE* out = fopen(argv[5], "wb");
    if (!in || !out) return 3;
    int rc;
    if (sched == 0) rc = shoup ? run_cases<Fl<FrP29, 0>, true>(in, out) : run_cases<Fl<FrP29, 0>, false>(in, out);
    else rc = shoup ? run_cases<Fl<FrP29, 1>, true>(in, out) : run_cases<Fl<FrP29, 1>, false>(in, out);
    fclose(in);
    if (fclose(out) != 0) return 3;
    return rc;
  }
  if (mode == "elem" && argc == 5) {
    const std::vector<ElemRec> recs = elem_read(argv[3]);
    std::vector<ElemOut> outs(recs.size());
    for (size_t i = 0; i < recs.size(); i++) {
      if (atoi(argv[2]) == 0) elem_apply<Fl<FrP29, 0>>(recs[i], outs[i]);
      else elem_apply<Fl<FrP29, 1>>(recs[i], outs[i]);
    }
    elem_write(argv[4], outs);
    return 0;
  }
  if (mode == "ops") return run_ops();
  fprintf(stderr, "usage: ntt_elem_check envelope | run SCHED SHOUP IN OUT | elem SCHED IN OUT | ops\n");
  return 3;
}
