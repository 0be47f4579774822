// Kernels of the witness solver's DEFERRED form (capgpu_plonk_key_set_solve_form; the rule: solve_defer.hpp, the field code:
// solve_defer29.hpp).  k_solve_vars_defer and k_solve_vars_packed_defer<W> are the walks of k_solve_vars_lin and
// k_solve_vars_packed_lin<W> (solve_kernels.hpp) - hint-capable, the LIN case compiled in, one __syncthreads() per level, the
// packed item decode of solve_pack.hpp - over a deferred schedule: an item is a direct item (solve_item_lin, as it is), a
// FRAC row or a FLUSH item.
// THE SIDE BUFFER.  Entry e of a launch owns 2 * slots images at side + e * 2 * slots: [slot] the denominator of the
// pending variable at that deferred slot (internal form), [slots + slot] the prefix product a flush item keeps for it
// between its two passes.  It is indexed by deferred slot, not by variable: the transfer models have some thousands of
// deferred variables out of ~20 000.  A pending variable's NUMERATOR stands in vars_out where its value will, in the
// variables' own form; after the last level - a flush - vars_out holds plain canonical words everywhere.
// A FRAC row of level l is read at level l + 1 by other wavefronts of the workgroup through vars_out and the side buffer,
// behind the barrier, like a value in the direct form: neither is `const` or `__restrict__` here.
// Compiled in solve_defer.hip, a translation unit of its own: solve.hip's and plonk.hip's kernels keep the code they had.
#pragma once
#include <hip/hip_runtime.h>

#include "solve_defer.hpp"
#include "solve_defer29.hpp"
#include "solve_items.hpp"
#include "solve_pack.hpp"

namespace cap {
namespace pk {

// the deferred schedule's own tables (device pointers, owned by the key) and the launch's side buffer
struct SolveDefer {
  const int32_t* dslot;        // [num_vars]: deferred slot; read only for a variable the plan says is pending
  const uint32_t* flush_vars;  // the flush items' variables, group after group
  fe* side;                    // [count][2 * slots]
  size_t slots;
};

template <int INV>
__device__ __forceinline__ void solve_item_defer(const SolveRowTables& t, const SolveHints& hp, const SolveDefer& dt,
                                                 const sv29::Exps& ex, uint32_t k, fe* vars, fe* side,
                                                 unsigned long long* status_word) {
  using D = sv29::Defer<CAP_FL_SCHED, INV>;
  using F = typename D::F;
  const sp::Row r = t.rows[k];
  const uint32_t kind8 = r.kw & 0xffu;
  if (kind8 == sd::FLUSH) {
    // (count <= sd::kGroup and the ids and slots are the plan's: checked when the key took the form)
    const uint32_t count = r.kw >> 8;
    const uint32_t* fv = dt.flush_vars + r.row;
    fe* den = side + dt.dslot[fv[0]];  // a group's slots are consecutive
    fe* pre = den + dt.slots;
    D::flush_group(
        count, [&](uint32_t i) { return F::load(den[i]); }, [&](uint32_t i) { return F::from_ext(vars[fv[i]]); },
        [&](uint32_t i, const fl& x) { pre[i] = F::store(x); }, [&](uint32_t i) { return F::load(pre[i]); },
        [&](uint32_t i, const fl& v) { vars[fv[i]] = F::to_ext(v); }, ex);
    return;
  }
  if (kind8 & sd::kFrac) {
    const size_t j = r.row, n = t.n;
    const uint32_t mask = r.kw >> 8;
    fl num[4], den[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t id = t.wire_vars[(size_t)i * n + j];  // (below num_vars: checked when the key took the table)
      num[i] = F::from_ext(vars[id]);
      den[i] = F::one();
      if ((mask >> i) & 1) den[i] = F::load(side[dt.dslot[id]]);  // (the plan's mask: no value decides it)
    }
    const uint32_t target = t.wire_vars[(size_t)4 * n + j];
    const fe* sel = t.sel + j;
    fl n4, d4;
    const bool zero_den = D::row_value_frac([&](int s) { return F::load(sel[(size_t)s * n]); }, kind8 & 0x7fu, num, den,
                                            F::load(t.konst[k]), &n4, &d4);
    if (zero_den) atomicMin(status_word, (unsigned long long)j);
    vars[target] = F::to_ext(n4);
    side[dt.dslot[target]] = F::store(d4);
    return;
  }
  solve_item_lin<INV>(t, hp, ex, k, vars, status_word);
}

template <int INV>
__global__ __launch_bounds__(kSolveThreads) void k_solve_vars_defer(const fe* __restrict__ given /*[count][num_given]*/,
                                                                   SolveRowTables t, sv29::Exps ex, fe* vars_out,
                                                                   unsigned long long* __restrict__ status, SolveHints hp,
                                                                   SolveDefer dt) {
  const size_t p = blockIdx.x;
  fe* vars = vars_out + p * t.num_vars;
  fe* side = dt.side + p * 2 * dt.slots;
  const fe* giv = given + p * t.num_given;
  for (size_t v = threadIdx.x; v < t.num_vars; v += kSolveThreads) {
    const int32_t s = t.slot[v];
    fe x;
#pragma unroll
    for (int i = 0; i < 8; i++) x.v[i] = 0;
    if (s >= 0) x = giv[s];
    vars[v] = x;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t l = 0; l < t.levels; l++) {
    const uint32_t end = t.level_off[l + 1];
#pragma unroll 1
    for (uint32_t k = t.level_off[l] + threadIdx.x; k < end; k += kSolveThreads)
      solve_item_defer<INV>(t, hp, dt, ex, k, vars, side, &status[p]);
    __syncthreads();
  }
}

// (the side buffer goes by the launch's ENTRY, not by the witness: a launch over a witness list needs no more than its own
// count of rows)
template <int W, int INV>
__global__ __launch_bounds__(kSolveThreads) void k_solve_vars_packed_defer(const fe* __restrict__ given, size_t given_stride,
                                                                          SolveRowTables t, sv29::Exps ex, fe* vars_out,
                                                                          size_t vars_stride,
                                                                          unsigned long long* __restrict__ status /*per witness*/,
                                                                          const uint32_t* __restrict__ which, uint32_t count,
                                                                          SolveHints hp, SolveDefer dt) {
#pragma unroll 1
  for (uint32_t s = 0; s < (uint32_t)W; s++) {
    const uint32_t entry = spk::slot_entry(blockIdx.x, s, W);
    if (entry >= count) break;  // (uniform over the workgroup, and no barrier inside this loop)
    const size_t p = spk::entry_witness(which, entry);
    fe* vars = vars_out + p * vars_stride;
    const fe* giv = given + p * given_stride;
    for (size_t v = threadIdx.x; v < t.num_vars; v += kSolveThreads) {
      const int32_t sl = t.slot[v];
      fe x;
#pragma unroll
      for (int i = 0; i < 8; i++) x.v[i] = 0;
      if (sl >= 0) x = giv[sl];
      vars[v] = x;
    }
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t l = 0; l < t.levels; l++) {
    const uint32_t begin = t.level_off[l], items = spk::level_items(t.level_off[l + 1] - begin, W);
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < items; i += kSolveThreads) {
      const spk::Item it = spk::item_decode(begin, i, W);
      const uint32_t entry = spk::slot_entry(blockIdx.x, it.slot, W);
      if (entry < count) {
        const size_t p = spk::entry_witness(which, entry);
        solve_item_defer<INV>(t, hp, dt, ex, it.k, vars_out + p * vars_stride, dt.side + (size_t)entry * 2 * dt.slots, &status[p]);
      }
    }
    __syncthreads();
  }
}

}  // namespace pk
}  // namespace cap
