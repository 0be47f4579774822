// What the witness solver's host code (plonk.hip) and its kernel (solve_kernels.hpp, compiled in solve.hip) share: the
// schedule as the kernel reads it, and the launch.
#pragma once
#include <hip/hip_runtime.h>

#include "field.hpp"
#include "solve29.hpp"
#include "solve_pack.hpp"
#include "solve_plan.hpp"

namespace cap {
namespace pk {

constexpr unsigned long long kSolved = ~0ull;
constexpr int kSolveThreads = 256;  // one workgroup per witness, or per W witnesses (solve_pack.hpp)

// the hint tables of a schedule (device pointers, owned by the key); hints null: no hints - then no item is a hint item
struct SolveHints {
  const sp::Hint* hints;
  const uint32_t* targets;  // the hints' target ids
};

// the schedule as the kernels read it (all device pointers, owned by the key): the kernels' argument
struct SolveRowTables {
  const int32_t* slot;        // [num_vars]: index into a witness's given values, -1: not given
  const sp::Row* rows;        // the items - defining rows and hint items - by (level, kind, row or hint, chunk)
  const fe* konst;            // per item: 1 / q_o or 1 / q_hash_i, internal form, canonical (a hint item: unused)
  const uint32_t* level_off;  // [levels + 1]
  const uint32_t* wire_vars;  // [5][n] the key's table
  const fe* sel;              // [13][n] selector values, internal form, canonical
  uint32_t levels, pad;
  size_t n, num_vars, num_given;
};
// ... and as the host hands it round: with the hint tables, which the kernels take as an argument of their own, the last -
// the kernels of keys without hints keep the argument layout they had before hints
struct SolveTables : SolveRowTables {
  SolveHints hp;
  bool lin = false;  // the schedule holds LIN rows: the launches run the kernels that carry that rule (solve_kernels.hpp)
  // the DEFERRED form (capgpu_plonk_key_set_solve_form; solve_defer.hpp): the tables above are the deferred schedule's, the
  // launches run solve_defer.hip's kernels and need SolveLaunch::d_side
  bool defer = false;
  const int32_t* dslot = nullptr;        // [num_vars]: deferred slot, -1: never deferred
  const uint32_t* flush_vars = nullptr;  // the flush items' variables
  size_t side_slots = 0;                 // deferred slots per witness: a launch of `count` needs side_elems(count) images
  size_t side_elems(size_t count) const { return defer ? count * 2 * side_slots : 0; }
};

// k_solve_vars for `count` witnesses on stream s (through launch(): timed by the profiler, launch errors latched)
void solve_launch(hipStream_t s, uint32_t count, const fe* d_given, const SolveTables& t, const sv29::Exps& ex, fe* d_vars,
                  unsigned long long* d_status);

// One launch over a list of witnesses at W per workgroup (W: 1, 2, 4, 8 or 16 - spk::pack_for chooses).  d_which: `count`
// witness indices, or null for 0 .. count - 1; witness p reads d_given + p given_stride, writes d_vars + p vars_stride and
// d_status[p].  W = 1 without a list and with the tables' own row lengths is solve_launch.
struct SolveLaunch {
  uint32_t count;
  const fe* d_given;
  size_t given_stride;
  fe* d_vars;
  size_t vars_stride;
  unsigned long long* d_status;
  const uint32_t* d_which;
  fe* d_side = nullptr;  // a key in the DEFERRED form: SolveTables::side_elems(count) images of scratch, by launch entry
};
void solve_launch_packed(hipStream_t s, int W, const SolveLaunch& a, const SolveTables& t, const sv29::Exps& ex);
// The same launch for a schedule in the DEFERRED form (solve_defer.hip; solve_launch_packed hands it on and counts it):
// returns the W that ran.  form: the process's inverse form.
int solve_launch_defer(hipStream_t s, int W, const SolveLaunch& a, const SolveTables& t, const sv29::Exps& ex, int form);
// The process's inverse form (capgpu_fr_set_inverse_form; sv29::kInvFermat or sv29::kInvGcd): both launches above read it
// and run the instantiation of that form - the caller does not pass it.
int inverse_form_setting();
// k_fr_inverse over `count` field images on stream s, in the form set; d_in == d_out is allowed
void fr_inverse_launch(hipStream_t s, const fe* d_in, fe* d_out, size_t count, const sv29::Exps& ex);
// k_pub_inputs on stream s: the public inputs of `count` completed assignments (entry e: witness d_which[e], or e without
// a list; witness p reads d_vars + p vars_stride and writes the first num_inputs images of d_pub + p pub_stride)
void pub_inputs_launch(hipStream_t s, uint32_t count, const fe* d_vars, size_t vars_stride, const uint32_t* d_wire_vars,
                       const fe* d_sel, size_t n, uint32_t num_inputs, const uint32_t* d_which, fe* d_pub, size_t pub_stride);
// capgpu_plonk_solve_stats: launches, witnesses, launches at W > 1
void solve_stats(uint64_t* launches, uint64_t* witnesses, uint64_t* packed);
void solve_stats_reset();

}  // namespace pk
}  // namespace cap
