// The DEFERRED form of the witness solver's schedule (capgpu_plonk_key_set_solve_form): the plan of solve_plan.hpp, regrouped
// so that the inversions of a chain of OUT_INV rows happen together.  Host code without HIP and without field arithmetic,
// like solve_plan.hpp, which stays as it is: a key in the direct form keeps its plan, byte for byte.
// tests/cpp/solve_defer_check.cpp runs this under ASan + UBSan; tests/solve_defer_model.py is the same rule in Python.
//
// A value defined by a FRAC row is carried as a pair (numerator, denominator): the numerator where the variable's value
// will stand, the denominator in a side buffer at the variable's DEFERRED SLOT.  A FLUSH item turns up to kGroup such pairs
// into plain values with one inversion (prefix products, one inverse, walk back).
//
// The rule.  The direct plan's levels in ascending order, PENDING = the deferred variables without a plain value, empty at
// first.  At level l:
//   1. an item NEEDS A PLAIN VALUE of a pending variable when it is
//        a ROOT5 or LIN row that holds one in any cell,
//        an OUT row that holds one on a cell i < 4 with q_hash_i != 0,
//        a hint item (BITS, ISZERO, INV0) whose source is one.
//      If any item of the level does, a FLUSH LEVEL goes in front of it: ceil(|PENDING| / kGroup) flush items that resolve
//      ALL of PENDING in the order of their slots; PENDING is then empty and the slots start again at 0.
//   2. the level's items, with the PENDING that is left:
//        OUT_INV                              a FRAC row, whatever its inputs are
//        OUT_MUL with a pending input         a FRAC row
//        anything else                        the direct item
//      A FRAC row carries the mask of its cells i < 4 that hold a pending variable; the variable it defines takes the next
//      slot and joins PENDING behind the level.
// Behind the last level a final flush level resolves what is left.  Every deferred variable is resolved exactly once.
// Inside a level the items are ordered: direct OUT_MUL, LIN, FRAC OUT_MUL, FRAC OUT_INV, ROOT5, INV0, ISZERO, BITS; inside
// a kind as the direct plan has them.
//
// The items as the kernels read them (sp::Row):
//   a direct item    the direct plan's record
//   a FRAC row       row; kw = kind | kFrac | mask << 8      (the target is wire 4)
//   a FLUSH item     row = the offset of its group in flush_vars; kw = FLUSH | count << 8
#pragma once
#include "solve_plan.hpp"

namespace cap {
namespace sd {

constexpr uint32_t kFrac = 0x80;  // in the kind byte of kw
constexpr uint32_t FLUSH = 7;     // behind sp::LIN
#ifndef CAP_DEFER_GROUP
#define CAP_DEFER_GROUP 32  // (an A/B build may set another: make EXTRA=-DCAP_DEFER_GROUP=8 OUT=... OBJDIR=...)
#endif
constexpr uint32_t kGroup = CAP_DEFER_GROUP;  // pairs per flush item (DESIGN.md 9 has the choice)
constexpr uint32_t kNoSrc = ~0u;

struct Sched {
  std::vector<sp::Row> rows;         // the items, level by level
  std::vector<uint32_t> src;         // per item: its index in the direct plan's rows (its constant is that one's); kNoSrc: a flush item
  std::vector<uint32_t> level_off;   // levels + 1 offsets into rows
  std::vector<uint8_t> flush_level;  // per level: 1 for a flush level
  std::vector<int32_t> dslot;        // [num_vars]: the deferred slot, -1 for a variable that is never deferred
  std::vector<uint32_t> flush_vars;  // the flush items' variables, group after group
  uint64_t slots = 0;                // the largest PENDING: slots of the side buffer per witness
  // capgpu_solve_form_info's figures
  uint64_t deferred_vars = 0, frac_rows = 0, flush_levels = 0, flush_items = 0, levels = 0, inv_levels_direct = 0,
           inv_levels_deferred = 0;
};

inline uint32_t defer_rank(uint32_t kind8) {
  const uint32_t kind = kind8 & 0x7fu;
  if (kind8 & kFrac) return kind == sp::OUT_MUL ? 2u : 3u;
  return kind == sp::OUT_MUL ? 0u : kind == sp::LIN ? 1u : kind + 2;  // ROOT5 4, INV0 5, ISZERO 6, BITS 7
}

// P: a plan solve_plan_rules accepted for this table and these selector zeros (any hints, any flags).  P is only read.
inline void defer_plan(const sp::Plan& P, size_t n, const uint32_t* wire_vars, const uint8_t* sel_zero, Sched* out) {
  Sched& S = *out;
  S = Sched();
  S.dslot.assign(P.slot.size(), -1);
  S.level_off.push_back(0);
  std::vector<uint8_t> pend(P.slot.size(), 0);
  std::vector<uint32_t> pending;  // in slot order
  auto flush = [&]() {
    for (size_t at = 0; at < pending.size(); at += kGroup) {
      const uint32_t cnt = (uint32_t)std::min<size_t>(kGroup, pending.size() - at);
      S.rows.push_back(sp::Row{(uint32_t)S.flush_vars.size(), FLUSH | cnt << 8});
      S.src.push_back(kNoSrc);
      for (uint32_t i = 0; i < cnt; i++) S.flush_vars.push_back(pending[at + i]);
      S.flush_items++;
    }
    for (uint32_t v : pending) pend[v] = 0;
    pending.clear();
    S.level_off.push_back((uint32_t)S.rows.size());
    S.flush_level.push_back(1);
    S.flush_levels++;
  };
  struct Item {
    sp::Row r;
    uint32_t src, rank;
  };
  std::vector<Item> items;
  for (size_t l = 0; l + 1 < P.level_off.size(); l++) {
    bool need = false, inv_direct = false, inv0 = false;
    for (uint32_t k = P.level_off[l]; k < P.level_off[l + 1]; k++) {
      const sp::Row& r = P.rows[k];
      const uint32_t kind = sp::row_kind(r);
      if (kind == sp::OUT_INV || kind == sp::INV0) inv_direct = true;
      if (kind == sp::INV0) inv0 = true;
      if (sp::is_hint_kind(kind)) {
        need |= pend[P.hints[r.row].src] != 0;
        continue;
      }
      for (int i = 0; i < sp::kWires; i++) {
        const uint32_t v = wire_vars[(size_t)i * n + r.row];
        if (!pend[v]) continue;
        if (kind == sp::ROOT5 || kind == sp::LIN) need = true;
        else if (i < 4 && !sel_zero[(size_t)(sp::Q_HASH + i) * n + r.row]) need = true;
      }
    }
    S.inv_levels_direct += inv_direct;
    S.inv_levels_deferred += inv0;
    if (need && !pending.empty()) flush();
    items.clear();
    for (uint32_t k = P.level_off[l]; k < P.level_off[l + 1]; k++) {
      sp::Row r = P.rows[k];
      const uint32_t kind = sp::row_kind(r);
      if (kind == sp::OUT_MUL || kind == sp::OUT_INV) {
        uint32_t mask = 0;
        for (int i = 0; i < 4; i++) mask |= (uint32_t)pend[wire_vars[(size_t)i * n + r.row]] << i;
        if (kind == sp::OUT_INV || mask) r.kw = kind | kFrac | mask << 8;
      }
      items.push_back(Item{r, k, defer_rank(r.kw & 0xffu)});
    }
    std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.rank < b.rank; });
    const size_t before = pending.size();
    for (const Item& it : items) {
      S.rows.push_back(it.r);
      S.src.push_back(it.src);
      if (it.r.kw & kFrac) {
        const uint32_t v = wire_vars[(size_t)4 * n + it.r.row];
        S.dslot[v] = (int32_t)pending.size();
        pending.push_back(v);
        S.frac_rows++;
      }
    }
    for (size_t i = before; i < pending.size(); i++) pend[pending[i]] = 1;  // (behind the level: its rows are independent)
    S.slots = std::max<uint64_t>(S.slots, pending.size());
    S.level_off.push_back((uint32_t)S.rows.size());
    S.flush_level.push_back(0);
  }
  if (!pending.empty()) flush();
  S.deferred_vars = S.frac_rows;
  S.levels = S.level_off.size() - 1;
  S.inv_levels_deferred += S.flush_levels;
}

}  // namespace sd
}  // namespace cap
