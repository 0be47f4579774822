// The pairing tower of cap_amd/csrc/pairing29.hpp (Tower<SCHED>, TowerField<SCHED>) on the bound-tracking field of bound29.hpp: the
// element types for V = capbound::bfl and the instantiation the envelope check runs (tests/cpp/tower_envelope_check.cpp).
#pragma once
#include "bound29.hpp"

#include "../../cap_amd/csrc/pairing29.hpp"

namespace capbound {
struct bf2 {
  bfl c0, c1;
};
struct bf6 {
  bf2 c0, c1, c2;
};
struct bf12 {
  bf6 c0, c1;
};
struct bline {
  bfe m0, m1, mu0, mu1;
};
}  // namespace capbound

namespace cap {
namespace p29 {
constexpr int kBoundSched = -29;  // the "schedule" that selects the bound field
template <>
struct TowerField<kBoundSched> {
  using F = capbound::BoundFl<FqP29>;
  using V = capbound::bfl;
  using E2 = capbound::bf2;
  using E6 = capbound::bf6;
  using E12 = capbound::bf12;
  using Line = capbound::bline;
};
}  // namespace p29
}  // namespace cap

namespace capbound {
using BoundTower = cap::p29::Tower<cap::p29::kBoundSched>;
}  // namespace capbound
