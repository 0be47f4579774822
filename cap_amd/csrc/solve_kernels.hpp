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
// Compiled in solve.hip, a translation unit of its own: the prover's kernels in plonk.hip keep the code they had.
#pragma once
#include <hip/hip_runtime.h>

#include "solve.hpp"
#include "solve29.hpp"
#include "solve_pack.hpp"

namespace cap {
namespace pk {

__global__ __launch_bounds__(kSolveThreads) void k_solve_vars(const fe* __restrict__ given /*[count][num_given]*/, SolveTables t,
                                                         sv29::Exps ex, fe* vars_out /*[count][num_vars]*/,
                                                         unsigned long long* __restrict__ status /*[count]*/) {
  using S = sv29::Solve<>;
  using F = S::F;
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
    }
    __syncthreads();
  }
}

// W witnesses per workgroup (solve_pack.hpp has the item decode and the choice of W).  Slot s of workgroup b holds entry
// b W + s of the launch's witness list: witness which[entry], or the entry itself without a list; witness p reads
// given + p given_stride and writes vars_out + p vars_stride (the launches of a call with several keys: one per key, over
// that key's proofs, in rows of the call's largest lengths).  A slot at or beyond `count` loads and stores nothing; its
// lanes still reach every barrier.  Row by row the arithmetic is k_solve_vars's: the output is the same words.
template <int W>
__global__ __launch_bounds__(kSolveThreads) void k_solve_vars_packed(const fe* __restrict__ given, size_t given_stride,
                                                                    SolveTables t, sv29::Exps ex, fe* vars_out,
                                                                    size_t vars_stride,
                                                                    unsigned long long* __restrict__ status /*per witness*/,
                                                                    const uint32_t* __restrict__ which, uint32_t count) {
  using S = sv29::Solve<>;
  using F = S::F;
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
      }
    }
    __syncthreads();
  }
}

}  // namespace pk
}  // namespace cap
