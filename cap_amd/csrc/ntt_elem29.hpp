// The arithmetic of the NTT kernels (ntt.hip) where a host compiler can reach it: the barrier-delimited stages of
// lds_ntt, the per-element input and output steps of the column and row passes, and the element bodies of ntt3_combine
// and ntt3_combine5.  The kernels keep the addressing, the loads and stores, the stage loop and the barriers.
//
// Every function takes the field class F and its value type V (Fr29 and fl in the kernels); the element steps also
// take the type W of a 32-byte memory image (fe).  Two other instantiations exist:
//   * tests/cpp/ntt_elem_check.cpp runs them on the host with the bound assertions of field29.hpp switched on
//     (CAP_FL_CHECK), threads emulated as a loop over tid between the stages;
//   * tests/cpp/bound29.hpp substitutes a field whose values are upper bounds (limbs and magnitude), so that the
//     preconditions are checked for every input of a class, not for the tested ones (tests/golden/lazy_envelope.json).
// tests/hip/elemcheck.hip compiles them for the device, one lane per butterfly / element, against the host's words.
#pragma once
#include "field29.hpp"

namespace cap {

static CAP_HD uint32_t fl_any(const fl& a) {
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) o |= a.v[k];
  return o;
}
static CAP_HD uint32_t fe_any(const fe& a) {
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) o |= a.v[k];
  return o;
}

// The twiddle product of the butterflies and the subtractions that go with its bound.  SHOUP: tw_small holds PAIRS -
// entry i at [2i] the plain canonical twiddle, at [2i + 1] its quotient floor(w 2^261 / p) - the product is below 5p
// and the subtractions add 8p; otherwise entry i is the twiddle in the internal form, the product is a Montgomery
// product (< 1.2p for the values that occur) and the subtractions add 2p.
template <class F, class V, bool SHOUP>
struct NttTw {
  static constexpr int kStride = SHOUP ? 2 : 1;
  static CAP_HD V mul(const V& x, const V* __restrict__ tw_small, uint32_t idx) {
    if constexpr (SHOUP) return F::mul_shoup(x, tw_small[2 * idx], tw_small[2 * idx + 1]);
    else return F::mul(x, tw_small[idx]);
  }
  static CAP_HD V sub(const V& u, const V& t) {  // normalized
    if constexpr (SHOUP) return F::sub8p(u, t);
    else return F::sub2p(u, t);
  }
  static CAP_HD V sub_lazy(const V& u, const V& t) {  // no carry: only added to / subtracted from afterwards
    if constexpr (SHOUP) return F::sub8p_lazy(u, t);
    else return F::sub2p_lazy(u, t);
  }
};

// ---- the stages of lds_ntt on sh[len][C] (rows written bit-reversed: natural order out) ------------------------------
// One call does the work of thread tid of nthreads; the caller synchronises between two calls.

// The lone radix-2 stage of an odd stage count: every twiddle is omega^0 = 1.
template <class F, class V>
static CAP_HD void ntt_radix2_butterfly(V& x0, V& x1) {
  const V u = x0, v = x1;
  if (fl_any(v) == 0) {  // zero padding: the butterfly is a copy
    x1 = u;
    return;
  }
  const V t = F::weak_reduce(v);
  x0 = F::normalize(F::add(u, t));
  x1 = F::sub2p(u, t);
}
template <class F, class V>
static CAP_HD void ntt_stage_radix2(V* sh, uint32_t log_len, uint32_t log_c, uint32_t tid, uint32_t nthreads) {
  const uint32_t half_tile = 1u << (log_len + log_c - 1);
  const uint32_t cmask = (1u << log_c) - 1;
  for (uint32_t b = tid; b < half_tile; b += nthreads) {
    const uint32_t c = b & cmask, bb = b >> log_c;
    const uint32_t i0 = ((bb << 1) << log_c) + c, i1 = i0 + (1u << log_c);
    ntt_radix2_butterfly<F, V>(sh[i0], sh[i1]);
  }
}

// One radix-4 round (stages s, s + 1) on the four rows j, j + h, j + 2h, j + 3h, h = 2^s; pos = j mod h.
// Carries are propagated only where a value becomes a multiplicand (limbs < 2^30 needed) or goes back to LDS:
// a1, c1 = x + t have limbs < 2^30 as they are; b1 = a - t + 2p (8p) is only added to afterwards.
// s == 0: w1 = 1, so t = b, d themselves (weakly reduced for the subtraction), and zero operands make the butterfly a
// copy; the second-level twiddle of the (a1, c1) pair is omega^0 = 1 as well, that of (b1, d1) is omega_4.
template <class F, class V, bool SHOUP>
static CAP_HD void ntt_radix4_butterfly(V& x0, V& x1, V& x2, V& x3, const V* __restrict__ tw_small, uint32_t log_len,
                                        uint32_t s, uint32_t pos) {
  using T = NttTw<F, V, SHOUP>;
  const uint32_t h = 1u << s;
  V a = x0, b = x1, cc = x2, d = x3;
  V a1, b1, c1, d1, t;
  if (s == 0) {
    if (fl_any(b)) {
      t = F::weak_reduce(b);
      a1 = F::add(a, t);
      b1 = F::sub2p_lazy(a, t);
    } else {
      a1 = a;
      b1 = a;
    }
    if (fl_any(d)) {
      t = F::weak_reduce(d);
      c1 = F::normalize(F::add(cc, t));
      d1 = F::sub2p(cc, t);
    } else {
      c1 = cc;
      d1 = cc;
    }
    t = F::weak_reduce(c1);  // second-level twiddle of the (a1, c1) pair: omega^0 = 1
  } else {
    const uint32_t i_w1 = pos << (log_len - 1 - s);
    t = T::mul(b, tw_small, i_w1);
    a1 = F::add(a, t);
    b1 = T::sub_lazy(a, t);
    t = T::mul(d, tw_small, i_w1);
    c1 = F::add(cc, t);
    d1 = T::sub(cc, t);
    t = T::mul(c1, tw_small, pos << (log_len - 2 - s));
  }
  x0 = F::normalize(F::add(a1, t));
  x2 = T::sub(a1, t);
  t = T::mul(d1, tw_small, (pos + h) << (log_len - 2 - s));
  x1 = F::normalize(F::add(b1, t));
  x3 = T::sub(b1, t);
}
template <class F, class V, bool SHOUP>
static CAP_HD void ntt_stage_radix4(V* sh, const V* __restrict__ tw_small, uint32_t log_len, uint32_t log_c, uint32_t s,
                                    uint32_t tid, uint32_t nthreads) {
  const uint32_t quarter_tile = (1u << (log_len + log_c - 1)) >> 1;
  const uint32_t cmask = (1u << log_c) - 1;
  const uint32_t h = 1u << s;
  const uint32_t step = h << log_c;
  for (uint32_t g = tid; g < quarter_tile; g += nthreads) {
    const uint32_t c = g & cmask;
    const uint32_t gg = g >> log_c;
    const uint32_t pos = gg & (h - 1);
    const uint32_t j = ((gg >> s) << (s + 2)) + pos;
    const uint32_t i0 = (j << log_c) + c, i1 = i0 + step, i2 = i1 + step, i3 = i2 + step;
    ntt_radix4_butterfly<F, V, SHOUP>(sh[i0], sh[i1], sh[i2], sh[i3], tw_small, log_len, s, pos);
  }
}

// ---- per-element input and output steps of col_tile / row_tile ----------------------------------------------------------
// Input: the 32-byte image as it is (any value < 2^256), times its coset / pre-scale factor where there is one (a
// Montgomery product of two values < 2^256: < 1.17p; zero padding needs no scaling); fold: the coefficient in_fold
// positions further on, scaled by its own factor, is added in (normalized, < 2.4p).  in[fold_at] and pre_scale[pre_at] are
// formed and read only with fold set.  (One function for both steps: taken apart, ntt_row_pass<true> allocates one register less.)
template <class F, class V, class W>
static CAP_HD V ntt_in_elem(const W& raw, bool scaled, const W& pre, bool fold, const W* in, size_t fold_at,
                            const W* pre_scale, size_t pre_at) {
  const uint32_t nz = fe_any(raw);
  V v = F::load(raw);
  if (scaled && nz) v = F::mul(v, F::load(pre));
  if (fold) v = F::add_norm(v, F::mul(F::load(in[fold_at]), F::load(pre_scale[pre_at])));
  return v;
}
// Column pass output: times the inter-pass twiddle (has_tw; always with the 1/n-scaled table), else weakly reduced:
// either way below 2p, which fits the 32-byte image.
template <class F, class V, class W>
static CAP_HD W ntt_out_col(const V& x, bool has_tw, const W& tw) {
  const V v = has_tw ? F::mul(x, F::load(tw)) : F::weak_reduce(x);
  return F::pack(v);
}
// Row pass output: after the post-scale product, if any (ntt_scale_elem), canonical (< r) or, lazy_out, stored weakly
// reduced (< 2r; the reader takes any representative below 2^256).
template <class F, class V, class W>
static CAP_HD V ntt_scale_elem(const V& x, const W& w) {
  return F::mul(x, F::load(w));
}
template <class F, class V, class W>
static CAP_HD W ntt_out_row(const V& v, bool lazy_out) {
  return lazy_out ? F::store(v) : F::pack(F::canonical(v));
}

// ---- radix-3 stage of the N = 3 M transforms (ntt3_combine) ---------------------------------------------------------------
//   X[k] = Y0 + T1 + T2,  X[k + M] = Y0 - T2 + D,  X[k + 2M] = Y0 - T1 - D,  D = w3 (T1 - T2)
// y0 .. y2 any images < 2^256; t1, t2, d products of such (< 1.2p, d < 1.6p); x0, x1, x2 normalized, < 40p.
template <class F, class V, class W>
static CAP_HD void ntt3_combine_elem(const W& y0r, const W& y1r, const W& tw1, const W& y2r, const W& tw2, const W& w3,
                                     V& x0, V& x1, V& x2) {
  const V y0 = F::load(y0r);
  const V t1 = F::mul(F::load(y1r), F::load(tw1));
  const V t2 = F::mul(F::load(y2r), F::load(tw2));
  const V d = F::mul(F::sub(t1, t2), F::load(w3));
  x0 = F::normalize(F::add(F::add(y0, t1), t2));
  x1 = F::normalize(F::add(F::sub(y0, t2), d));
  x2 = F::sub(F::sub(y0, t1), d);
}
// inverse transform: times post (an arkworks-form integer table), plus the addend where there is one, canonical
// (products < 2p plus a value < 2^256: normalized and well inside what canonical takes)
template <class F, class V, class W>
static CAP_HD W ntt3_finish_elem(const V& x, const W& ps, bool has_add, const V& a) {
  V v = F::mul(x, F::load(ps));
  if (has_add) v = F::add_norm(v, a);
  return F::pack(F::canonical(v));
}

// ---- the solve of the five-coset inverse (ntt3_combine5); QC is Quot5Const --------------------------------------------------
template <class F, class V, class W, class QC>
struct Ntt5Elem {
  // sums of at most four reduced values (< 2p each, normalized): limbs < 2^31, well inside what normalize and canonical take
  static CAP_HD W finish(V v, int j, bool has_add, const V& pi, bool has_top, const V& h, const QC& qc) {
    if (has_add) v = F::add(v, F::mul(pi, F::load(qc.d[j])));
    if (has_top) v = F::add(v, F::mul(h, F::load(qc.mt[j])));
    return F::pack(F::canonical(F::normalize(v)));
  }
  static CAP_HD W odd(int jj, const V& o0, const V& o1, bool has_add, const V& pi, bool has_top, const V& h, const QC& qc) {
    return finish(F::mul_add_mul(o0, F::load(qc.odd[jj][0]), o1, F::load(qc.odd[jj][1])), 2 * jj + 1, has_add, pi, has_top,
                  h, qc);
  }
  static CAP_HD W even(int jj, const V& e0, const V& o0, const V& e1, const V& o1, const V& r, bool has_add, const V& pi,
                       bool has_top, const V& h, const QC& qc) {
    const V a = F::mul_add_mul(e0, F::load(qc.even[jj][0]), o0, F::load(qc.even[jj][1]));
    const V b = F::mul_add_mul(e1, F::load(qc.even[jj][2]), o1, F::load(qc.even[jj][3]));
    return finish(F::add(F::add(a, b), F::mul(r, F::load(qc.even[jj][4]))), 2 * jj, has_add, pi, has_top, h, qc);
  }
};

}  // namespace cap
