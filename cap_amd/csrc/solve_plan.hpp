// The plan of the witness solver (capgpu_plonk_key_set_given): which rows of a circuit DEFINE a variable, by which rule and
// in which order.  Host code without HIP and without field arithmetic - it sees the wire -> variable table, which selector
// VALUES are zero mod r, and the list of given variables; tests/cpp/solve_plan_check.cpp runs it under ASan + UBSan.
//
// The rule (include/capgpu.h has the full text).  V = the valued variables, at first the given ones.  Rows j = 0 .. n-1
// in ascending order; U = the distinct variables of the row's five cells that are not in V:
//   |U| = 0                      a constraint: defines nothing
//   j < num_inputs, |U| > 0      refused (a public-input variable must be given)
//   |U| >= 2                     refused
//   U = {u}, OUT                 u in wire 4 only and (q_o != 0 or q_ecc != 0):  w4 = rest / (q_o - q_ecc w0 w1 w2 w3)
//   U = {u}, ROOT5               u in exactly one wire i < 4, q_hash_i != 0, q_lc_i = 0, the q_mul of its pair = 0, q_ecc = 0:
//                                w_i = ((q_o w4 - rest without q_hash_i w_i^5) / q_hash_i)^(1/5)
//   any other shape              refused
// level(given) = 0, level(u) = 1 + the largest level among the other variables of its row: rows of one level are
// independent, so the kernel walks the levels and spreads a level's rows over its lanes.  Inside a level the rows are
// ordered by kind, then by row, so that a wavefront meets one kind wherever the level is wide enough.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

namespace cap {
namespace sp {

constexpr int kWires = 5;
constexpr int kSelectors = 13;
constexpr int Q_LC = 0, Q_MUL = 4, Q_HASH = 6, Q_O = 10, Q_C = 11, Q_ECC = 12;  // gatecheck29.hpp's order

enum Kind : uint32_t {
  OUT_MUL = 0,  // q_ecc = 0: w4 = rest * (1 / q_o), the constant made at set-up
  OUT_INV = 1,  // q_ecc != 0: one inversion per witness
  ROOT5 = 2,    // a fifth root on wire (kw >> 8)
};

// one defining row as the kernel reads it
struct Row {
  uint32_t row;
  uint32_t kw;  // kind | target wire << 8
};
inline uint32_t row_kind(const Row& r) { return r.kw & 0xffu; }
inline uint32_t row_wire(const Row& r) { return r.kw >> 8; }

struct Plan {
  std::vector<Row> rows;            // ordered by (level, kind, row)
  std::vector<uint32_t> level_off;  // levels + 1 offsets into rows: level l (1-based l + 1) is rows[level_off[l] .. level_off[l + 1])
  std::vector<int32_t> slot;        // [num_vars]: index in the given list, -1 for a variable that is not given
  uint64_t num_given = 0, num_defined = 0, levels = 0, widest_level = 0, inv_rows = 0, root_rows = 0;
  std::string error;  // empty: the plan stands
};

inline std::string fmt(const char* f, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, f, a, b, c);
  return buf;
}

// wire_vars: [5][n] ids below num_vars; sel_zero: [13][n], non-zero where the selector's value is 0 mod r.
// Returns false with Plan::error set when the circuit or the list is refused.
inline bool solve_plan(size_t n, size_t num_inputs, size_t num_vars, const uint32_t* wire_vars, const uint8_t* sel_zero,
                       const uint32_t* given, size_t num_given, Plan* out) {
  Plan& P = *out;
  P = Plan();
  P.slot.assign(num_vars, -1);
  for (size_t k = 0; k < num_given; k++) {
    const uint32_t v = given[k];
    if (v >= num_vars) {
      P.error = fmt("given_vars[%llu] = %llu, num_vars is %llu", k, v, num_vars);
      return false;
    }
    if (P.slot[v] >= 0) {
      P.error = fmt("variable %llu is given twice (given_vars[%llu] and given_vars[%llu])", v, (unsigned long long)P.slot[v], k);
      return false;
    }
    P.slot[v] = (int32_t)k;
  }
  P.num_given = num_given;
  // level per variable: 0 given, > 0 defined, -1 without a value so far
  std::vector<int32_t> level(num_vars, -1);
  for (size_t k = 0; k < num_given; k++) level[given[k]] = 0;
  struct Item {
    uint32_t level, kind, row, wire;
  };
  std::vector<Item> items;
  auto zero = [&](int s, size_t j) { return sel_zero[(size_t)s * n + j] != 0; };
  for (size_t j = 0; j < n; j++) {
    uint32_t v[kWires];
    for (int i = 0; i < kWires; i++) v[i] = wire_vars[(size_t)i * n + j];
    uint32_t u[2];
    int nu = 0;
    int32_t deepest = 0;
    for (int i = 0; i < kWires; i++) {
      if (level[v[i]] >= 0) {
        deepest = std::max(deepest, level[v[i]]);
        continue;
      }
      if (nu >= 1 && u[0] == v[i]) continue;
      if (nu >= 2 && u[1] == v[i]) continue;
      if (nu < 2) u[nu] = v[i];
      nu++;
    }
    if (nu == 0) continue;
    if (j < num_inputs) {
      P.error = fmt("row %llu is a public-input row and its variable %llu is not given", j, u[0]);
      return false;
    }
    if (nu >= 2) {
      P.error = fmt("row %llu holds two variables without a value, %llu and %llu", j, u[0], u[1]);
      return false;
    }
    int cells = 0, wire = -1;
    for (int i = 0; i < kWires; i++)
      if (v[i] == u[0]) {
        cells++;
        wire = i;
      }
    Item it{(uint32_t)deepest + 1, 0, (uint32_t)j, (uint32_t)wire};
    if (cells == 1 && wire == 4 && (!zero(Q_O, j) || !zero(Q_ECC, j))) {
      it.kind = zero(Q_ECC, j) ? OUT_MUL : OUT_INV;
    } else if (cells == 1 && wire < 4 && !zero(Q_HASH + wire, j) && zero(Q_LC + wire, j) && zero(Q_MUL + wire / 2, j) &&
               zero(Q_ECC, j)) {
      it.kind = ROOT5;
    } else {
      P.error = fmt("row %llu cannot define its variable %llu: it is neither an output on wire 4 alone (q_o or q_ecc set) nor a "
                    "fifth root on one of wires 0..3",
                    j, u[0]);
      return false;
    }
    level[u[0]] = (int32_t)it.level;
    items.push_back(it);
  }
  std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
    if (a.level != b.level) return a.level < b.level;
    if (a.kind != b.kind) return a.kind < b.kind;
    return a.row < b.row;
  });
  P.level_off.push_back(0);
  for (size_t k = 0; k < items.size(); k++) {
    const Item& it = items[k];
    while (P.level_off.size() < it.level) P.level_off.push_back((uint32_t)k);  // (levels are dense: this adds one at a time)
    P.rows.push_back(Row{it.row, it.kind | it.wire << 8});
    if (it.kind == OUT_INV) P.inv_rows++;
    if (it.kind == ROOT5) P.root_rows++;
  }
  if (!items.empty()) P.level_off.push_back((uint32_t)items.size());
  P.levels = P.level_off.size() - 1;
  P.num_defined = items.size();
  for (size_t l = 0; l + 1 < P.level_off.size(); l++)
    P.widest_level = std::max<uint64_t>(P.widest_level, P.level_off[l + 1] - P.level_off[l]);
  return true;
}

}  // namespace sp
}  // namespace cap
