// The witness solver's kernels (capgpu_plonk_solve_vars*, capgpu_plonk_prove_given*; host side in plonk.hip), in a
// translation unit of its own.
#define CAP_FL_SCHED 1
#include <atomic>

#include "launch.hpp"
#include "solve_kernels.hpp"

namespace cap {
namespace pk {

namespace {
std::atomic<uint64_t> g_launches{0}, g_witnesses{0}, g_packed{0};
void count_launch(uint32_t count, int W) {
  g_launches.fetch_add(1, std::memory_order_relaxed);
  g_witnesses.fetch_add(count, std::memory_order_relaxed);
  if (W > 1) g_packed.fetch_add(1, std::memory_order_relaxed);
}
// (a schedule with hint items runs the instantiations that hold the hint code - solve_kernels.hpp says why there are two)
template <int W>
void launch_packed(hipStream_t s, const char* name, const SolveLaunch& a, const SolveTables& t, const sv29::Exps& ex) {
  const auto kernel = t.hp.hints ? k_solve_vars_packed<W, true> : k_solve_vars_packed<W, false>;
  launch(name, kernel, dim3(spk::blocks_for(a.count, W)), dim3(kSolveThreads), 0, s, a.d_given, a.given_stride,
         static_cast<const SolveRowTables&>(t), ex, a.d_vars, a.vars_stride, a.d_status, a.d_which, a.count, t.hp);
}
}  // namespace

void solve_launch(hipStream_t s, uint32_t count, const fe* d_given, const SolveTables& t, const sv29::Exps& ex, fe* d_vars,
                  unsigned long long* d_status) {
  launch("k_solve_vars", t.hp.hints ? k_solve_vars<true> : k_solve_vars<false>, dim3(count), dim3(kSolveThreads), 0, s, d_given,
         static_cast<const SolveRowTables&>(t), ex, d_vars, d_status, t.hp);
  count_launch(count, 1);
}

void solve_launch_packed(hipStream_t s, int W, const SolveLaunch& a, const SolveTables& t, const sv29::Exps& ex) {
  if (!a.count) return;
  if (W <= 1 && !a.d_which && a.given_stride == t.num_given && a.vars_stride == t.num_vars)
    return solve_launch(s, a.count, a.d_given, t, ex, a.d_vars, a.d_status);
  switch (W) {
    case 16: launch_packed<16>(s, "k_solve_vars_packed<16>", a, t, ex); break;
    case 8: launch_packed<8>(s, "k_solve_vars_packed<8>", a, t, ex); break;
    case 4: launch_packed<4>(s, "k_solve_vars_packed<4>", a, t, ex); break;
    case 2: launch_packed<2>(s, "k_solve_vars_packed<2>", a, t, ex); break;
    default: launch_packed<1>(s, "k_solve_vars_packed<1>", a, t, ex); W = 1; break;
  }
  count_launch(a.count, W);
}

void solve_stats(uint64_t* launches, uint64_t* witnesses, uint64_t* packed) {
  if (launches) *launches = g_launches.load();
  if (witnesses) *witnesses = g_witnesses.load();
  if (packed) *packed = g_packed.load();
}
void solve_stats_reset() {
  g_launches.store(0);
  g_witnesses.store(0);
  g_packed.store(0);
}

}  // namespace pk
}  // namespace cap
