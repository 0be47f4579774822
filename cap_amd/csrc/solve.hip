// The witness solver's kernel (capgpu_plonk_solve_vars*; host side in plonk.hip), in a translation unit of its own.
#define CAP_FL_SCHED 1
#include "launch.hpp"
#include "solve_kernels.hpp"

namespace cap {
namespace pk {

void solve_launch(hipStream_t s, uint32_t count, const fe* d_given, const SolveTables& t, const sv29::Exps& ex, fe* d_vars,
                  unsigned long long* d_status) {
  launch("k_solve_vars", k_solve_vars, dim3(count), dim3(kSolveThreads), 0, s, d_given, t, ex, d_vars, d_status);
}

}  // namespace pk
}  // namespace cap
