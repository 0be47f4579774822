// The kernels of the witness solver's DEFERRED form (capgpu_plonk_key_set_solve_form; solve_defer_kernels.hpp), in a
// translation unit of its own: solve.hip's and plonk.hip's code objects are not touched by them.  Host side: the launch
// solve.hip's solve_launch_packed hands a deferred schedule to.
#define CAP_FL_SCHED 1
#include "launch.hpp"
#include "solve_defer_kernels.hpp"

namespace cap {
namespace pk {

namespace {
template <int W>
void launch_packed_defer(hipStream_t s, const char* name, const SolveLaunch& a, const SolveTables& t, const sv29::Exps& ex,
                         const SolveDefer& dt, int form) {
  const auto kernel =
      form == sv29::kInvGcd ? k_solve_vars_packed_defer<W, sv29::kInvGcd> : k_solve_vars_packed_defer<W, sv29::kInvFermat>;
  launch(name, kernel, dim3(spk::blocks_for(a.count, W)), dim3(kSolveThreads), 0, s, a.d_given, a.given_stride,
         static_cast<const SolveRowTables&>(t), ex, a.d_vars, a.vars_stride, a.d_status, a.d_which, a.count, t.hp, dt);
}
}  // namespace

int solve_launch_defer(hipStream_t s, int W, const SolveLaunch& a, const SolveTables& t, const sv29::Exps& ex, int form) {
  const bool gcd = form == sv29::kInvGcd;
  const SolveDefer dt{t.dslot, t.flush_vars, a.d_side, t.side_slots};
  if (!a.d_side && t.side_slots) {  // (a caller that carved no side buffer: refused like a bad launch, nothing runs)
    LaunchError& le = launch_error();
    if (le.code == hipSuccess) {
      le.code = hipErrorInvalidValue;
      le.kernel = "k_solve_vars_defer (no side buffer)";
    }
    return 1;
  }
  if (W <= 1 && !a.d_which && a.given_stride == t.num_given && a.vars_stride == t.num_vars) {
    launch(gcd ? "k_solve_vars_defer/gcd" : "k_solve_vars_defer",
           gcd ? k_solve_vars_defer<sv29::kInvGcd> : k_solve_vars_defer<sv29::kInvFermat>, dim3(a.count), dim3(kSolveThreads), 0, s,
           a.d_given, static_cast<const SolveRowTables&>(t), ex, a.d_vars, a.d_status, t.hp, dt);
    return 1;
  }
  static const char* const names[2][5] = {
      {"k_solve_vars_packed_defer<1>", "k_solve_vars_packed_defer<2>", "k_solve_vars_packed_defer<4>",
       "k_solve_vars_packed_defer<8>", "k_solve_vars_packed_defer<16>"},
      {"k_solve_vars_packed_defer<1>/gcd", "k_solve_vars_packed_defer<2>/gcd", "k_solve_vars_packed_defer<4>/gcd",
       "k_solve_vars_packed_defer<8>/gcd", "k_solve_vars_packed_defer<16>/gcd"}};
  const char* const* name = names[gcd ? 1 : 0];
  switch (W) {
    case 16: launch_packed_defer<16>(s, name[4], a, t, ex, dt, form); return 16;
    case 8: launch_packed_defer<8>(s, name[3], a, t, ex, dt, form); return 8;
    case 4: launch_packed_defer<4>(s, name[2], a, t, ex, dt, form); return 4;
    case 2: launch_packed_defer<2>(s, name[1], a, t, ex, dt, form); return 2;
    default: launch_packed_defer<1>(s, name[0], a, t, ex, dt, form); return 1;
  }
}

}  // namespace pk
}  // namespace cap
