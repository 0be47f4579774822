// The G1 law of cap_amd/csrc/curve29.hpp (G1Law<F, V>) on the bound-tracking field of bound29.hpp: the register points,
// the memory images and the C ABI's constants for V = capbound::bfl, and the classes of points the headers name.
// A coordinate is a bound (bfl); a point is at infinity when its zz is KNOWN to be zero - any other point takes the
// finite side of every is_inf test, and the callers run the infinity paths with such a point.
#pragma once
#include "bound29.hpp"

#include "../../cap_amd/csrc/curve29.hpp"
#include "../../cap_amd/csrc/lagrange_elem29.hpp"

namespace capbound {

struct bg1a {
  bfl x, y;
};
struct bg1x {
  bfl x, y, zz, zzz;
};
struct bg1_affine {
  bfe x, y;
};
struct bg1_xyzz {
  bfe x, y, zz, zzz;
};
struct bg1_jac {
  bfe x, y, z;
};
static inline bool limbs_all_zero(const bfl& a) { return a.zero; }

}  // namespace capbound

namespace cap {
template <>
struct G1Types<capbound::bfl> {
  using A = capbound::bg1a;
  using X = capbound::bg1x;
  using MA = capbound::bg1_affine;
  using MX = capbound::bg1_xyzz;
  using MJ = capbound::bg1_jac;
  static capbound::bfe ext_one() {  // canonical
    capbound::bfe r;
    r.mag = 1u << 20;
    r.zero = false;
    return r;
  }
  static capbound::bfe ext_zero() { return capbound::bfe(); }
};
}  // namespace cap

namespace cap {
constexpr int kBoundSched = -29;  // the "schedule" that selects the law on the bound field in LagT
template <>
struct LagCurve<kBoundSched> {
  using C = G1Law<capbound::BoundFl<FqP29>, capbound::bfl>;
};
}  // namespace cap
