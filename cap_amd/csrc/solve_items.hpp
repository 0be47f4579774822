// The item functions the solver's kernels share (solve_kernels.hpp, compiled in solve.hip; solve_defer_kernels.hpp, compiled in
// solve_defer.hip): a hint item, the ids of an item on the rows' path, and one item of a schedule with LIN rows.  Device code
// only; every function is inlined into the kernel that calls it.
#pragma once
#include <hip/hip_runtime.h>

#include "solve.hpp"
#include "solve29.hpp"

namespace cap {
namespace pk {

// A hint item of kind ISZERO or BITS (the rules: solve29.hpp): the source's image is read from the witness's variables, the
// targets' images are stored there.  A BITS item stores min(32, count - 32 chunk) images - a bound of the plan, not of the
// witness - each the image of 1 times its bit; nothing here branches on, or addresses by, a value.  (An INV0 item takes the
// rows' path: solve_item_ids.)
__device__ __forceinline__ void solve_hint_item(const SolveHints& t, uint32_t kind, uint32_t hint, uint32_t chunk, fe* vars) {
  using S = sv29::Solve<>;
  const sp::Hint h = t.hints[hint];
  const fe plain = S::hint_plain(vars[h.src]);  // (ids below num_vars: checked when the key took the hints)
  const uint32_t* tg = t.targets + h.first;
  const bool bits = kind == sp::BITS;
  const uint32_t word = bits ? S::word_of(plain, chunk) : S::zero_bit(plain), base = chunk * 32;  // (an ISZERO item: chunk 0)
  const uint32_t nb = !bits ? 1 : h.count - base < 32 ? h.count - base : 32;
#pragma unroll 1
  for (uint32_t b = 0; b < nb; b++) vars[tg[base + b]] = S::bit_image((word >> b) & 1);
}

// Whether any active lane of the wavefront holds an ISZERO or BITS item: a condition in a scalar register, so that a
// wavefront of rows alone - every wavefront of a key without hints - branches round that code.
__device__ __forceinline__ bool solve_any_lane(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

// The variable ids of an item on the rows' path and its target: a row's five cells; an INV0 item's source in every cell
// (row_value reads cell 0 alone) and the hint's one target.  *j: the row whose selectors the value reads - an INV0 item's
// value reads none, row 0 stands in.
__device__ __forceinline__ uint32_t solve_item_ids(const SolveRowTables& t, const SolveHints& hp, const sp::Row& r, uint32_t kind,
                                                   uint32_t wire, uint32_t* ids, size_t* j) {
  if (kind == sp::INV0) {
    const sp::Hint h = hp.hints[r.row];
#pragma unroll
    for (int i = 0; i < wc29::kWires; i++) ids[i] = h.src;
    *j = 0;
    return hp.targets[h.first];
  }
  *j = r.row;
  uint32_t target = 0;
#pragma unroll
  for (int i = 0; i < wc29::kWires; i++) {
    ids[i] = t.wire_vars[(size_t)i * t.n + r.row];  // (below num_vars: checked when the key took the table)
    if (wire == (uint32_t)i) target = ids[i];
  }
  return target;
}

// One item of a schedule with LIN rows (k_solve_vars_lin, k_solve_vars_packed_lin<W>: solve_kernels.hpp) for the witness whose variables are `vars`:
template <int INV>
__device__ __forceinline__ void solve_item_lin(const SolveRowTables& t, const SolveHints& hp, const sv29::Exps& ex, uint32_t k,
                                               fe* vars, unsigned long long* status_word) {
  using S = sv29::Solve<CAP_FL_SCHED, INV>;
  using F = typename S::F;
  const sp::Row r = t.rows[k];
  const uint32_t kind = r.kw & 0xffu, wire = r.kw >> 8;
  const bool hint = kind == sp::ISZERO || kind == sp::BITS;  // (LIN's number lies behind the hint kinds)
  if (solve_any_lane(hint)) {
    if (hint) solve_hint_item(hp, kind, r.row, wire, vars);
  }
  if (hint) return;
  size_t j;
  uint32_t ids[wc29::kWires];
  const uint32_t target = solve_item_ids(t, hp, r, kind, wire, ids, &j);
  fl w[wc29::kWires];
#pragma unroll
  for (int i = 0; i < wc29::kWires; i++) w[i] = F::from_ext(vars[ids[i]]);
  const fe* sel = t.sel + j;
  const size_t n = t.n;
  bool zero_den;
  const fl val = S::template row_value<true, true>([&](int s) { return F::load(sel[(size_t)s * n]); }, kind, wire, w,
                                                   F::load(t.konst[k]), ex, &zero_den);
  if (zero_den) atomicMin(status_word, (unsigned long long)j);
  vars[target] = F::to_ext(val);
}

}  // namespace pk
}  // namespace cap
