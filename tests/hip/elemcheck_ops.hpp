// One record = one call of a function of cap_amd/csrc/ntt_elem29.hpp or round_elem29.hpp, for tests/hip/elemcheck.hip (one lane per record,
// gfx950, the product's flags) and for the host twin (tests/cpp/ntt_elem_check.cpp, mode "elem", bound assertions on).
// The two must produce the same words: the device build takes mul_lo32 and mad_wide through inline v_mad_u64_u32, the
// host does not.  Vectors: tests/elemcheck_vectors.py.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cap_amd/csrc/ntt_elem29.hpp"
#include "../../cap_amd/csrc/round_elem29.hpp"

namespace cap {

constexpr uint32_t kElemMagicIn = 0x454c4d49u, kElemMagicOut = 0x454c4d4fu;
constexpr int kElemSlots = 52, kElemOuts = 4;
struct ElemRec {
  uint32_t op, a0, a1, pad;
  uint32_t in[kElemSlots][9];  // limbs of an fl, or the 8 words of a 32-byte image (word 8 unused)
};
struct ElemOut {
  uint32_t w[kElemOuts][9];
};
enum ElemOp {
  EL_RADIX2 = 0,     // in 0, 1 -> out 0, 1
  EL_RADIX4_SHOUP,   // in 0 .. 3; twiddle pairs of table entries 1, 2, 3 in slots 4 .. 9 (log_len 3, s 1, pos 1) -> out 0 .. 3
  EL_RADIX4_MONT,    // the same with internal-form twiddles in slots 4 .. 6
  EL_FIRST4_SHOUP,   // the s == 0 round: in 0 .. 3, the pair of omega_4 in slots 4, 5 (log_len 2) -> out 0 .. 3
  EL_FIRST4_MONT,    // omega_4 in slot 4
  EL_IN,             // images raw, pre, fold_raw, fold_pre in 0 .. 3; a0 bit 0 scaled, bit 1 fold -> out 0
  EL_OUT,            // fl in 0, image factor in 1; a0 the output form, a1 first row -> image out 0
  EL_COMBINE3,       // images y0, y1, tw1, y2, tw2, w3 in 0 .. 5 -> x0, x1, x2 in out 0 .. 2
  EL_FINISH3,        // fl x in 0, images post, add in 1, 2; a0: 0 store, 1 post, 2 post + add -> image out 0
  EL_COMBINE5,       // images y (5) in 0 .. 4, their un-scale factors in 5 .. 9, pi, top in 10, 11; a0 = jj + 16 * even,
                     // a1 bit 0 add, bit 1 top.  odd: odd[jj] in 12, 13, d_j in 14, mt_j = slot 7.  even: even[jj][0 .. 2]
                     // in 12 .. 14, [3], [4], d_j, mt_j = slots 5 .. 8 (every slot is an arbitrary image) -> image out 0
  EL_PERM,           // images beta gamma tw k[5] wire[5] sig[5] in 0 .. 17 -> images num, den in out 0, 1
  EL_KX,             // images k, x in 0, 1 -> image out 0
  EL_QUOT_FOLD,      // images sel[22] col[6] z_next x inv_nx1 chal[6] k[5] zh_inv[8] in 0 .. 49; a0 = zi < 8 -> image out 0
  EL_QUOT_DIRECT,    // the same through k_quotient<false>'s body
  EL_LINCOMB,        // a0 = n <= 25 terms, a1 = mask of the terms that reach; (scalar, value) images in 2t, 2t + 1 -> out 0
  EL_OPS
};
struct ElemQuot5 {
  fe odd[2][2], even[3][5], mt[5], d[5];
};

// the kernels' Chal, QuotConst and the accessors they hand to the bodies of round_elem29.hpp, over any image type
template <class W>
struct ChalT {
  W beta, gamma, alpha, alpha2, beta_inv, alpha_beta5;
};
template <class W>
struct QuotConstT {
  W g, k[5], zh_inv[8];
};
template <class W>
struct PointT {
  const W *zn, *xi, *inx;
  uint32_t zi;
  CAP_HD const W& z_next() const { return *zn; }
  CAP_HD const W& x() const { return *xi; }
  CAP_HD const W& inv() const { return *inx; }
  CAP_HD const W& zh_inv(const QuotConstT<W>& q) const { return q.zh_inv[zi]; }
};
template <class W>
struct TermsT {
  const W *s, *v;
  const int* on;
  uint32_t n;
  CAP_HD bool active(uint32_t t) const { return t < n && on[t]; }
  CAP_HD const W& scalar(uint32_t t) const { return s[t]; }
  CAP_HD const W& value(uint32_t t) const { return v[t]; }
};
static CAP_HD fl elem_fl(const uint32_t (&w)[9]) {
  fl r;
  for (int i = 0; i < 9; i++) r.v[i] = w[i];
  return r;
}
static CAP_HD fe elem_fe(const uint32_t (&w)[9]) {
  fe r;
  for (int i = 0; i < 8; i++) r.v[i] = w[i];
  return r;
}
static CAP_HD void elem_put(ElemOut& o, int k, const fl& v) {
  for (int i = 0; i < 9; i++) o.w[k][i] = v.v[i];
}
static CAP_HD void elem_put(ElemOut& o, int k, const fe& v) {
  for (int i = 0; i < 8; i++) o.w[k][i] = v.v[i];
  o.w[k][8] = 0;
}

// the output forms of the plans, in the order of tests/cpp/ntt_elem_check.cpp
template <class F>
static CAP_HD fe elem_out_step(uint32_t form, const fl& x, bool first_row, const fe& f) {
  switch (form) {
    case 0: return ntt_out_col<F, fl, fe>(x, !first_row, f);
    case 1: return ntt_out_col<F, fl, fe>(x, true, f);
    case 2: return ntt_out_row<F, fl, fe>(x, false);
    case 3:
    case 4: return ntt_out_row<F, fl, fe>(ntt_scale_elem<F, fl, fe>(x, f), false);
    case 5: return ntt_out_row<F, fl, fe>(ntt_scale_elem<F, fl, fe>(x, f), true);
    default: return ntt_out_row<F, fl, fe>(x, true);
  }
}

template <class F>
static CAP_HD void elem_apply(const ElemRec& r, ElemOut& o) {
  for (int k = 0; k < kElemOuts; k++)
    for (int i = 0; i < 9; i++) o.w[k][i] = 0;
  switch (r.op) {
    case EL_RADIX2: {
      fl x0 = elem_fl(r.in[0]), x1 = elem_fl(r.in[1]);
      ntt_radix2_butterfly<F, fl>(x0, x1);
      elem_put(o, 0, x0);
      elem_put(o, 1, x1);
      break;
    }
    case EL_RADIX4_SHOUP:
    case EL_RADIX4_MONT:
    case EL_FIRST4_SHOUP:
    case EL_FIRST4_MONT: {
      fl x0 = elem_fl(r.in[0]), x1 = elem_fl(r.in[1]), x2 = elem_fl(r.in[2]), x3 = elem_fl(r.in[3]);
      fl tw[8];
      for (int i = 0; i < 8; i++) tw[i] = F::zero();
      if (r.op == EL_RADIX4_SHOUP) {  // entries 1, 2, 3 of a table of pairs; entry 0 is not read at pos 1
        for (int i = 0; i < 6; i++) tw[2 + i] = elem_fl(r.in[4 + i]);
        ntt_radix4_butterfly<F, fl, true>(x0, x1, x2, x3, tw, 3, 1, 1);
      } else if (r.op == EL_RADIX4_MONT) {
        for (int i = 0; i < 3; i++) tw[1 + i] = elem_fl(r.in[4 + i]);
        ntt_radix4_butterfly<F, fl, false>(x0, x1, x2, x3, tw, 3, 1, 1);
      } else if (r.op == EL_FIRST4_SHOUP) {  // entry 1 = omega_4
        tw[2] = elem_fl(r.in[4]);
        tw[3] = elem_fl(r.in[5]);
        ntt_radix4_butterfly<F, fl, true>(x0, x1, x2, x3, tw, 2, 0, 0);
      } else {
        tw[1] = elem_fl(r.in[4]);
        ntt_radix4_butterfly<F, fl, false>(x0, x1, x2, x3, tw, 2, 0, 0);
      }
      elem_put(o, 0, x0);
      elem_put(o, 1, x1);
      elem_put(o, 2, x2);
      elem_put(o, 3, x3);
      break;
    }
    case EL_IN: {
      const fe raw = elem_fe(r.in[0]), pre = elem_fe(r.in[1]), fr = elem_fe(r.in[2]), fp = elem_fe(r.in[3]);
      elem_put(o, 0, ntt_in_elem<F, fl, fe>(raw, (r.a0 & 1) != 0, pre, (r.a0 & 2) != 0, &fr, 0, &fp, 0));
      break;
    }
    case EL_OUT:
      elem_put(o, 0, elem_out_step<F>(r.a0, elem_fl(r.in[0]), r.a1 != 0, elem_fe(r.in[1])));
      break;
    case EL_COMBINE3: {
      fl x0, x1, x2;
      ntt3_combine_elem<F, fl, fe>(elem_fe(r.in[0]), elem_fe(r.in[1]), elem_fe(r.in[2]), elem_fe(r.in[3]),
                                   elem_fe(r.in[4]), elem_fe(r.in[5]), x0, x1, x2);
      elem_put(o, 0, x0);
      elem_put(o, 1, x1);
      elem_put(o, 2, x2);
      break;
    }
    case EL_FINISH3: {
      const fl x = elem_fl(r.in[0]);
      if (r.a0 == 0) elem_put(o, 0, F::store(x));
      else elem_put(o, 0, ntt3_finish_elem<F, fl, fe>(x, elem_fe(r.in[1]), r.a0 == 2, F::load(elem_fe(r.in[2]))));
      break;
    }
    case EL_COMBINE5: {
      using E = Ntt5Elem<F, fl, fe, ElemQuot5>;
      fl v[5];
      for (int i = 0; i < 5; i++) v[i] = ntt_scale_elem<F, fl, fe>(F::load(elem_fe(r.in[i])), elem_fe(r.in[5 + i]));
      const fl pi = F::load(elem_fe(r.in[10])), h = F::load(elem_fe(r.in[11]));
      const int jj = (int)(r.a0 & 15u);
      const bool even = (r.a0 & 16u) != 0, add = (r.a1 & 1u) != 0, top = (r.a1 & 2u) != 0;
      ElemQuot5 qc;
      const fe z = elem_fe(r.in[15]);  // every entry the call does not read
      for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) qc.odd[i][j] = z;
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 5; j++) qc.even[i][j] = z;
      for (int j = 0; j < 5; j++) qc.mt[j] = qc.d[j] = z;
      if (even) {  // slots 12, 13, 14: even[jj][0 .. 2]; [3], [4], d_j and mt_j reuse the un-scale factors 5 .. 8
        if (jj > 2) break;
        for (int j = 0; j < 3; j++) qc.even[jj][j] = elem_fe(r.in[12 + j]);
        qc.even[jj][3] = elem_fe(r.in[5]);
        qc.even[jj][4] = elem_fe(r.in[6]);
        qc.d[2 * jj] = elem_fe(r.in[7]);
        qc.mt[2 * jj] = elem_fe(r.in[8]);
        elem_put(o, 0, E::even(jj, v[0], v[1], v[2], v[3], v[4], add, pi, top, h, qc));
      } else {
        if (jj > 1) break;
        qc.odd[jj][0] = elem_fe(r.in[12]);
        qc.odd[jj][1] = elem_fe(r.in[13]);
        qc.d[2 * jj + 1] = elem_fe(r.in[14]);
        qc.mt[2 * jj + 1] = elem_fe(r.in[7]);
        elem_put(o, 0, E::odd(jj, v[1], v[3], add, pi, top, h, qc));
      }
      break;
    }
    case EL_PERM: {
      fe img[18], num, den;
      for (int i = 0; i < 18; i++) img[i] = elem_fe(r.in[i]);
      const fe* wires = img + 8;
      const fe* sigs = img + 13;
      perm_numden_row<F, fl, fe>(img[0], img[1], img[2], img + 3, [&](int i) -> const fe& { return wires[i]; },
                                 [&](int i) -> const fe& { return sigs[i]; }, num, den);
      elem_put(o, 0, num);
      elem_put(o, 1, den);
      break;
    }
    case EL_KX:
      elem_put(o, 0, kx_elem<F, fl, fe>(elem_fe(r.in[0]), F::load(elem_fe(r.in[1]))));
      break;
    case EL_QUOT_FOLD:
    case EL_QUOT_DIRECT: {
      if (r.a0 > 7) break;
      fe img[50];
      for (int i = 0; i < 50; i++) img[i] = elem_fe(r.in[i]);
      const ChalT<fe> ch = {img[31], img[32], img[33], img[34], img[35], img[36]};
      QuotConstT<fe> qc;
      qc.g = img[0];
      for (int i = 0; i < 5; i++) qc.k[i] = img[37 + i];
      for (int i = 0; i < 8; i++) qc.zh_inv[i] = img[42 + i];
      const PointT<fe> at = {&img[28], &img[29], &img[30], r.a0};
      const fe* im = img;
      auto sel = [&](int s) -> const fe& { return im[s]; };
      auto col = [&](int j) -> const fe& { return im[22 + j]; };
      if (r.op == EL_QUOT_FOLD) elem_put(o, 0, quotient_point<true, F, fl, fe>(sel, col, at, ch, qc));
      else elem_put(o, 0, quotient_point<false, F, fl, fe>(sel, col, at, ch, qc));
      break;
    }
    case EL_LINCOMB: {
      if (r.a0 > 25) break;
      fe sc[25], va[25];
      int on[25];
      for (uint32_t t = 0; t < 25; t++) {
        sc[t] = elem_fe(r.in[2 * t]);
        va[t] = elem_fe(r.in[2 * t + 1]);
        on[t] = (int)((r.a1 >> t) & 1u);
      }
      elem_put(o, 0, lincomb_elem<F, fl, fe>(r.a0, TermsT<fe>{sc, va, on, r.a0}));
      break;
    }
    default: break;
  }
}

// file of records: magic, count, records; file of results: magic, count, one ElemOut per record
static inline std::vector<ElemRec> elem_read(const char* path) {
  FILE* f = fopen(path, "rb");
  uint32_t h[2];
  if (!f || fread(h, 4, 2, f) != 2 || h[0] != kElemMagicIn || h[1] > (1u << 20)) {
    fprintf(stderr, "elemcheck: cannot read %s\n", path);
    exit(3);
  }
  std::vector<ElemRec> v(h[1]);
  if (fread(v.data(), sizeof(ElemRec), v.size(), f) != v.size()) {
    fprintf(stderr, "elemcheck: %s is truncated\n", path);
    exit(3);
  }
  fclose(f);
  return v;
}
static inline void elem_write(const char* path, const std::vector<ElemOut>& o) {
  FILE* f = fopen(path, "wb");
  const uint32_t h[2] = {kElemMagicOut, (uint32_t)o.size()};
  if (!f || fwrite(h, 4, 2, f) != 2 || fwrite(o.data(), sizeof(ElemOut), o.size(), f) != o.size() || fclose(f) != 0) {
    fprintf(stderr, "elemcheck: cannot write %s\n", path);
    exit(3);
  }
}

}  // namespace cap
