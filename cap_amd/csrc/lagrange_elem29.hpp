// The arithmetic of the Lagrange key builder (lagrange.hip: lag_load, lag_stage, lag_finish) where a host compiler can
// reach it: the per-lane bodies as host+device functions templated on the multiplication schedule.  The kernels keep
// the thread index, the bounds test and the loads and stores of their own lane.
// tests/cpp/lagrange_check.cpp runs the same functions on the host with the bound assertions of field29.hpp switched on
// (CAP_FL_CHECK), one loop iteration per lane, the points passing through the g1_xyzz memory image between the stages
// as they do on the device.
#pragma once
#include "curve29.hpp"

namespace cap {

constexpr uint32_t kLagBlind = 3;  // blinding points behind the n Lagrange points

// scalar_mul is a chain of ~380 dependent point operations: the kernels call it, they do not inline it
#if defined(__HIPCC__)
#define CAP_LAG_CALL __host__ __device__ __noinline__
#else
#define CAP_LAG_CALL inline
#endif

// The group law a schedule number selects: 0 and 1 are G1LT on the two multiplication schedules of Fl, what the kernels
// use; tests/cpp/bound_curve29.hpp adds a number of its own for the law on the field whose values are bounds, so that
// the same LagT runs on it while LagT<0> and LagT<1> keep their names and their out-of-line scalar_mul.
template <int SCHED>
struct LagCurve {
  using C = G1LT<SCHED>;
};

template <int SCHED>
struct LagT {
  using C = typename LagCurve<SCHED>::C;
  using F = typename C::F;
  using g1a = typename C::g1a;
  using g1x = typename C::g1x;
  using g1_affine = typename C::g1_affine;
  using g1_xyzz = typename C::g1_xyzz;

  static CAP_HD g1x neg_pt(const g1x& p) {
    g1x r = p;
    r.y = F::weak_reduce(F::neg(p.y));
    return r;
  }

  // [k] B, k a canonical 256-bit integer: two bits per step from the top (B, 2B, 3B held in registers)
  static CAP_LAG_CALL g1x scalar_mul(const g1x& b, const fe& k) {
    int top = -1;
    for (int i = 7; i >= 0 && top < 0; i--)
      if (k.v[i]) top = 32 * i + C::top_bit(k.v[i]);
    if (top < 0 || C::is_inf(b)) return C::inf();
    const g1x b2 = C::dbl(b);
    const g1x b3 = C::add(b2, b);
    g1x acc = C::inf();
    for (int pos = top | 1; pos >= 1; pos -= 2) {  // digit = bits pos, pos - 1
      acc = C::dbl(C::dbl(acc));
      const uint32_t d = (k.v[(pos - 1) >> 5] >> ((pos - 1) & 31)) & 3u;
      if (d) acc = C::add(acc, d == 1 ? b : (d == 2 ? b2 : b3));
    }
    return acc;
  }

  static CAP_HD uint32_t bitrev(uint32_t i, uint32_t log_n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return log_n ? __brev(i) >> (32 - log_n) : 0;
#else
    uint32_t r = 0;
    for (uint32_t b = 0; b < log_n; b++) r |= ((i >> b) & 1u) << (log_n - 1 - b);
    return r;
#endif
  }
  // lag_load: one SRS point (the window-0 rows of the SRS table: internal form, canonical) as the transform holds it
  static CAP_HD g1_xyzz load_point(const g1_affine& p) { return C::store(C::from_affine(C::load(p))); }

  // lag_stage: (A, B) -> (A + [k] B, A - [k] B); has_k false stands for k = 1
  static CAP_HD void butterfly(const g1_xyzz& a_in, const g1_xyzz& b_in, const fe& k, bool has_k, g1_xyzz& lo,
                               g1_xyzz& hi) {
    const g1x A = C::load(a_in);
    g1x B = C::load(b_in);
    if (has_k) B = scalar_mul(B, k);
    lo = C::store(C::add(A, B));
    hi = C::store(C::add(A, neg_pt(B)));
  }

  // lag_finish: out[j] = [1/n] a[j] in arkworks' affine form, j < n; out[n + e] = [tau^(n + e)] G - [tau^e] G
  static CAP_HD void finish(const g1_xyzz* __restrict__ a, uint32_t n, const fe& n_inv, const g1_affine* __restrict__ srs,
                            uint32_t j, g1_affine& out) {
    g1x p;
    if (j < n) {
      p = scalar_mul(C::load(a[j]), n_inv);
    } else {  // e = j - n
      p = C::add_mixed(C::from_affine(C::load(srs[j])), C::load(srs[j - n]), true);
    }
    g1_affine o;
    if (C::is_inf(p)) {
      o.x = G1Types<typename C::fl>::ext_zero();
      o.y = G1Types<typename C::fl>::ext_zero();
    } else {
      const g1a q = C::to_affine(p);
      o.x = F::to_ext(q.x);
      o.y = F::to_ext(q.y);
    }
    out = o;
  }
};
using Lag = LagT<CAP_FL_SCHED>;

}  // namespace cap
