// Kernel of the witness solver (capgpu_plonk_solve_vars*): completes `count` variable assignments from their given values
// through the schedule a key got from capgpu_plonk_key_set_given (the plan: solve_plan.hpp, the row rule: solve29.hpp).
//   k_solve_vars   one workgroup of 256 lanes per witness.  The given values are scattered into the witness's row of
//                  vars_out and every other variable is zeroed; then the levels are walked in order, the lanes striding
//                  over a level's rows, one __syncthreads() between levels.
//   k_solve_vars_packed<W>   one workgroup per W witnesses (W = 2, 4, 8, 16): the same walk, the lanes striding over a
//                  level's (row, witness slot) items, so that a level narrower than the workgroup keeps W times as many
//                  lanes busy.  (W = 1 is instantiated too: k_solve_vars with a witness list and row strides.)
// A value written at level l is read by other wavefronts of the same workgroup at level l + 1 through vars_out in global
// memory, behind the barrier: vars_out is therefore neither `const` nor `__restrict__` here and never read through a
// read-only path.  The tables (selector values, wire -> variable ids, rows, constants) are read-only for the launch.
// A row whose denominator is 0 mod r leaves its variable 0 and enters its row number into the witness's status word by
// atomicMin (preset to all ones): the smallest such row, whatever order the lanes arrive in.
// Rows of a level are ordered by kind, so a wavefront pays the fixed exponentiation (254 squarings) only where its 64
// rows hold an OUT row with q_ecc or a fifth root.
// A level's items are its defining rows and its HINT items (kinds INV0, ISZERO, BITS behind the rows' three, INV0 first:
// next to the other exponentiations): an entry of the level like a row, so the packed decode does not know of them.
// k_solve_vars_lin / k_solve_vars_packed_lin<W>: the same walks for a schedule that holds LIN rows (capgpu_plonk_key_set_solver's
// CAPGPU_SOLVER_LINEAR), kernels of their own so that the ones above keep their code.
// k_pub_inputs: the public inputs of completed assignments, one lane per (witness, row) (capgpu_plonk_pub_inputs*,
// capgpu_plonk_prove_given_io*).
// k_fr_inverse: the field inversion alone, one element per lane (capgpu_fr_inverse_batch*).
// Compiled in solve.hip, a translation unit of its own: the prover's kernels in plonk.hip keep the code they had.
#pragma once
#include <hip/hip_runtime.h>

#include "solve.hpp"
#include "solve29.hpp"
#include "solve_items.hpp"
#include "solve_pack.hpp"

namespace cap {
namespace pk {

// HINTS: whether the key's schedule holds hint items.  A key without hints runs the instantiations without the hint code:
// with it inlined beside the rows' path the compiler keeps ~190 more scalar values in spill lanes (25 without), which a
// launch bound by the latency of one dependent chain pays for on every row.  Their item loop is the one from before hints,
// kept to the letter, and the hint tables travel as the LAST kernel argument (SolveHints; unused there), so that those
// instantiations are the code they were.
// INV: the form of the inversions of kinds OUT_INV and INV0 (solve29.hpp) - sv29::kInvFermat, the default, or sv29::kInvGcd
// (capgpu_fr_set_inverse_form).  The form is a parameter of the row rule's struct alone: the kernels' text is one.
template <bool HINTS, int INV = sv29::kInvFermat>
__global__ __launch_bounds__(kSolveThreads) void k_solve_vars(const fe* __restrict__ given /*[count][num_given]*/, SolveRowTables t,
                                                         sv29::Exps ex, fe* vars_out /*[count][num_vars]*/,
                                                         unsigned long long* __restrict__ status /*[count]*/, SolveHints hp) {
  using S = sv29::Solve<CAP_FL_SCHED, INV>;
  using F = typename S::F;
  const size_t p = blockIdx.x;
  fe* vars = vars_out + p * t.num_vars;
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
    for (uint32_t k = t.level_off[l] + threadIdx.x; k < end; k += kSolveThreads) {
      const sp::Row r = t.rows[k];
      const uint32_t kind = r.kw & 0xffu, wire = r.kw >> 8;
      if constexpr (!HINTS) {  // the loop as it was before hints, to the letter: the compiler gives it the code it gave it
        const size_t j = r.row;
        fl w[wc29::kWires];
        uint32_t target = 0;
#pragma unroll
        for (int i = 0; i < wc29::kWires; i++) {
          const uint32_t id = t.wire_vars[(size_t)i * t.n + j];  // (below num_vars: checked when the key took the table)
          if (wire == (uint32_t)i) target = id;
          w[i] = F::from_ext(vars[id]);
        }
        const fe* sel = t.sel + j;
        const size_t n = t.n;
        bool zero_den;
        const fl val = S::row_value([&](int s) { return F::load(sel[(size_t)s * n]); }, kind, wire, w, F::load(t.konst[k]), ex,
                                    &zero_den);
        if (zero_den) atomicMin(&status[p], (unsigned long long)j);
        vars[target] = F::to_ext(val);
        continue;
      }
      const bool hint = kind > sp::INV0;
      if (solve_any_lane(hint)) {
        if (hint) solve_hint_item(hp, kind, r.row, wire, vars);
      }
      if (hint) continue;
      size_t j;
      uint32_t ids[wc29::kWires];
      const uint32_t target = solve_item_ids(t, hp, r, kind, wire, ids, &j);
      fl w[wc29::kWires];
#pragma unroll
      for (int i = 0; i < wc29::kWires; i++) w[i] = F::from_ext(vars[ids[i]]);
      const fe* sel = t.sel + j;
      const size_t n = t.n;
      bool zero_den;
      const fl val = S::template row_value<true>([&](int s) { return F::load(sel[(size_t)s * n]); }, kind, wire, w,
                                                 F::load(t.konst[k]), ex, &zero_den);
      if (zero_den) atomicMin(&status[p], (unsigned long long)j);
      vars[target] = F::to_ext(val);
    }
    __syncthreads();
  }
}

// W witnesses per workgroup (solve_pack.hpp has the item decode and the choice of W).  Slot s of workgroup b holds entry
// b W + s of the launch's witness list: witness which[entry], or the entry itself without a list; witness p reads
// given + p given_stride and writes vars_out + p vars_stride (the launches of a call with several keys: one per key, over
// that key's proofs, in rows of the call's largest lengths).  A slot at or beyond `count` loads and stores nothing; its
// lanes still reach every barrier.  Row by row the arithmetic is k_solve_vars's: the output is the same words.
template <int W, bool HINTS, int INV = sv29::kInvFermat>
__global__ __launch_bounds__(kSolveThreads) void k_solve_vars_packed(const fe* __restrict__ given, size_t given_stride,
                                                                    SolveRowTables t, sv29::Exps ex, fe* vars_out,
                                                                    size_t vars_stride,
                                                                    unsigned long long* __restrict__ status /*per witness*/,
                                                                    const uint32_t* __restrict__ which, uint32_t count,
                                                                    SolveHints hp) {
  using S = sv29::Solve<CAP_FL_SCHED, INV>;
  using F = typename S::F;
#pragma unroll 1
  for (uint32_t s = 0; s < (uint32_t)W; s++) {  // (slot by slot: a lane's stores stay next to its neighbours')
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
        fe* vars = vars_out + p * vars_stride;
        const uint32_t k = it.k;
        const sp::Row r = t.rows[k];
        const uint32_t kind = r.kw & 0xffu, wire = r.kw >> 8;
        if constexpr (!HINTS) {  // (to the letter what it was before hints, like k_solve_vars's)
          const size_t j = r.row;
          fl w[wc29::kWires];
          uint32_t target = 0;
#pragma unroll
          for (int c = 0; c < wc29::kWires; c++) {
            const uint32_t id = t.wire_vars[(size_t)c * t.n + j];  // (below num_vars: checked when the key took the table)
            if (wire == (uint32_t)c) target = id;
            w[c] = F::from_ext(vars[id]);
          }
          const fe* sel = t.sel + j;
          const size_t n = t.n;
          bool zero_den;
          const fl val = S::row_value([&](int q) { return F::load(sel[(size_t)q * n]); }, kind, wire, w, F::load(t.konst[k]), ex,
                                      &zero_den);
          if (zero_den) atomicMin(&status[p], (unsigned long long)j);
          vars[target] = F::to_ext(val);
        } else {
          const bool hint = kind > sp::INV0;
          if (solve_any_lane(hint)) {
            if (hint) solve_hint_item(hp, kind, r.row, wire, vars);
          }
          if (!hint) {
            size_t j;
            uint32_t ids[wc29::kWires];
            const uint32_t target = solve_item_ids(t, hp, r, kind, wire, ids, &j);
            fl w[wc29::kWires];
#pragma unroll
            for (int c = 0; c < wc29::kWires; c++) w[c] = F::from_ext(vars[ids[c]]);
            const fe* sel = t.sel + j;
            const size_t n = t.n;
            bool zero_den;
            const fl val = S::template row_value<true>([&](int q) { return F::load(sel[(size_t)q * n]); }, kind, wire, w,
                                                       F::load(t.konst[k]), ex, &zero_den);
            if (zero_den) atomicMin(&status[p], (unsigned long long)j);
            vars[target] = F::to_ext(val);
          }
        }
      }
    }
    __syncthreads();
  }
}

// ---- schedules with LIN rows (capgpu_plonk_key_set_solver, CAPGPU_SOLVER_LINEAR) -----------------------------------------------
// Kernels of their own, so that every instantiation above stays the code it was: k_solve_vars_lin and
// k_solve_vars_packed_lin<W> are the hint-capable walks above with the row rule's LIN case compiled in.  A schedule with a
// LIN row always runs these, with or without hints (a schedule without hints holds no hint item and hp is never read).
// One item of such a schedule: solve_item_lin (solve_items.hpp).
template <int INV>
__global__ __launch_bounds__(kSolveThreads) void k_solve_vars_lin(const fe* __restrict__ given /*[count][num_given]*/,
                                                                 SolveRowTables t, sv29::Exps ex, fe* vars_out,
                                                                 unsigned long long* __restrict__ status, SolveHints hp) {
  const size_t p = blockIdx.x;
  fe* vars = vars_out + p * t.num_vars;
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
    for (uint32_t k = t.level_off[l] + threadIdx.x; k < end; k += kSolveThreads) solve_item_lin<INV>(t, hp, ex, k, vars, &status[p]);
    __syncthreads();
  }
}

template <int W, int INV>
__global__ __launch_bounds__(kSolveThreads) void k_solve_vars_packed_lin(const fe* __restrict__ given, size_t given_stride,
                                                                        SolveRowTables t, sv29::Exps ex, fe* vars_out,
                                                                        size_t vars_stride,
                                                                        unsigned long long* __restrict__ status /*per witness*/,
                                                                        const uint32_t* __restrict__ which, uint32_t count,
                                                                        SolveHints hp) {
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
        solve_item_lin<INV>(t, hp, ex, it.k, vars_out + p * vars_stride, &status[p]);
      }
    }
    __syncthreads();
  }
}

// capgpu_plonk_pub_inputs*: the public inputs of completed assignments.  One lane per (witness, row j < num_inputs):
//   pub = q_o w4 - q_ecc w0 w1 w2 w3 w4 - rest      (the value of PI that makes wc29::Check::gate zero at the row)
// from the key's wire -> variable table and selector values, for a general row.  Entry e of the launch is witness
// which[e] (or e without a list); witness p reads vars + p vars_stride and writes row p of pub_out, `pub_stride` images long,
// of which this launch writes the first num_inputs (canonical external Montgomery form).  vars is only read.
__global__ __launch_bounds__(kSolveThreads) void k_pub_inputs(const fe* __restrict__ vars, size_t vars_stride,
                                                             const uint32_t* __restrict__ wire_vars, const fe* __restrict__ sel,
                                                             size_t n, uint32_t num_inputs, const uint32_t* __restrict__ which,
                                                             uint32_t count, fe* __restrict__ pub_out, size_t pub_stride) {
  using S = sv29::Solve<>;
  using F = typename S::F;
  const size_t i = (size_t)blockIdx.x * kSolveThreads + threadIdx.x;
  if (i >= (size_t)count * num_inputs) return;
  const uint32_t entry = (uint32_t)(i / num_inputs), j = (uint32_t)(i % num_inputs);
  const size_t p = spk::entry_witness(which, entry);
  const fe* v = vars + p * vars_stride;
  fl w[wc29::kWires];
#pragma unroll
  for (int c = 0; c < wc29::kWires; c++) w[c] = F::from_ext(v[wire_vars[(size_t)c * n + j]]);  // (ids below num_vars: checked with the table)
  const fe* q = sel + j;
  pub_out[p * pub_stride + j] = F::to_ext(S::pub_value([&](int s) { return F::load(q[(size_t)s * n]); }, w));
}

// capgpu_fr_inverse_batch*: out[i] = 1 / in[i] (0 for 0) over `count` field images (external Montgomery form; any 256-bit
// word pattern is taken mod r), canonical results.  One element per lane; in and out may be the same array - a lane reads
// its element before it writes it and touches no other - so neither is __restrict__.
template <int INV>
__global__ __launch_bounds__(kSolveThreads) void k_fr_inverse(const fe* in, fe* out, size_t count, sv29::Exps ex) {
  using S = sv29::Solve<CAP_FL_SCHED, INV>;
  using F = typename S::F;
  const size_t i = (size_t)blockIdx.x * kSolveThreads + threadIdx.x;
  if (i >= count) return;
  const fl a = F::from_ext(in[i]);
  fl y;
  if constexpr (INV == sv29::kInvGcd) {
    y = inv_gcd<FrP29, CAP_FL_SCHED>(a);
  } else {
    y = S::pow_words(a, [&](int w) { return ex.inv[w]; });
  }
  out[i] = F::to_ext(y);
}

}  // namespace pk
}  // namespace cap
