// The witness solver's kernels (capgpu_plonk_solve_vars*, capgpu_plonk_prove_given*; host side in plonk.hip), in a
// translation unit of its own.
// Here too: the process's inverse form (capgpu_fr_set_inverse_form) - which the solver's launches read - and the batch
// inverse calls (capgpu_fr_inverse_batch*), so that every kernel holding an inversion of either form is device code of this
// translation unit and plonk.hip's code object is not touched by them.
#define CAP_FL_SCHED 1
#include <atomic>

#include "context.hpp"
#include "host_util.hpp"
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
// capgpu_fr_set_inverse_form: -1 is the process default (CAPGPU_FR_INVERSE=fermat|gcd; anything else counts as fermat)
std::atomic<int> g_inverse_form{-1};
std::atomic<uint64_t> g_inv_launches[2];  // launches holding an inversion, by form: the solver's and k_fr_inverse's
void count_inverse(int form) { g_inv_launches[form].fetch_add(1, std::memory_order_relaxed); }
// (a schedule with hint items runs the instantiations that hold the hint code - solve_kernels.hpp says why there are two;
// each in the two inverse forms)
template <int W>
void launch_packed(hipStream_t s, const char* name, const SolveLaunch& a, const SolveTables& t, const sv29::Exps& ex, int form) {
  // (a schedule with LIN rows: the kernels that carry that rule, with or without hints)
  const auto kernel = t.lin ? (form == sv29::kInvGcd ? k_solve_vars_packed_lin<W, sv29::kInvGcd>
                                                     : k_solve_vars_packed_lin<W, sv29::kInvFermat>)
                      : form == sv29::kInvGcd
                          ? (t.hp.hints ? k_solve_vars_packed<W, true, sv29::kInvGcd> : k_solve_vars_packed<W, false, sv29::kInvGcd>)
                          : (t.hp.hints ? k_solve_vars_packed<W, true> : k_solve_vars_packed<W, false>);
  launch(name, kernel, dim3(spk::blocks_for(a.count, W)), dim3(kSolveThreads), 0, s, a.d_given, a.given_stride,
         static_cast<const SolveRowTables&>(t), ex, a.d_vars, a.vars_stride, a.d_status, a.d_which, a.count, t.hp);
}
}  // namespace

int inverse_form_setting() {
  static const int env_default = [] {
    const char* e = getenv("CAPGPU_FR_INVERSE");
    return e && !strcmp(e, "gcd") ? sv29::kInvGcd : sv29::kInvFermat;
  }();
  const int m = g_inverse_form.load(std::memory_order_relaxed);
  return m < 0 ? env_default : m;
}

void solve_launch(hipStream_t s, uint32_t count, const fe* d_given, const SolveTables& t, const sv29::Exps& ex, fe* d_vars,
                  unsigned long long* d_status) {
  const int form = inverse_form_setting();
  const auto kernel = t.lin ? (form == sv29::kInvGcd ? k_solve_vars_lin<sv29::kInvGcd> : k_solve_vars_lin<sv29::kInvFermat>)
                      : form == sv29::kInvGcd
                          ? (t.hp.hints ? k_solve_vars<true, sv29::kInvGcd> : k_solve_vars<false, sv29::kInvGcd>)
                          : (t.hp.hints ? k_solve_vars<true> : k_solve_vars<false>);
  launch(t.lin ? (form == sv29::kInvGcd ? "k_solve_vars_lin/gcd" : "k_solve_vars_lin")
               : form == sv29::kInvGcd ? "k_solve_vars/gcd" : "k_solve_vars",
         kernel, dim3(count), dim3(kSolveThreads), 0, s, d_given,
         static_cast<const SolveRowTables&>(t), ex, d_vars, d_status, t.hp);
  count_launch(count, 1);
  count_inverse(form);
}

void solve_launch_packed(hipStream_t s, int W, const SolveLaunch& a, const SolveTables& t, const sv29::Exps& ex) {
  if (!a.count) return;
  if (t.defer) {  // a key in the DEFERRED form: the kernels of solve_defer.hip, counted like any launch
    const int form = inverse_form_setting();
    count_launch(a.count, solve_launch_defer(s, W, a, t, ex, form));
    count_inverse(form);
    return;
  }
  if (W <= 1 && !a.d_which && a.given_stride == t.num_given && a.vars_stride == t.num_vars)
    return solve_launch(s, a.count, a.d_given, t, ex, a.d_vars, a.d_status);
  const int form = inverse_form_setting();
  const bool gcd = form == sv29::kInvGcd;
  // the name the profiler and a launch error carry: the kernel that runs - a LIN schedule's own (launch_packed)
  static const char* const names[2][2][5] = {
      {{"k_solve_vars_packed<1>", "k_solve_vars_packed<2>", "k_solve_vars_packed<4>", "k_solve_vars_packed<8>", "k_solve_vars_packed<16>"},
       {"k_solve_vars_packed<1>/gcd", "k_solve_vars_packed<2>/gcd", "k_solve_vars_packed<4>/gcd", "k_solve_vars_packed<8>/gcd",
        "k_solve_vars_packed<16>/gcd"}},
      {{"k_solve_vars_packed_lin<1>", "k_solve_vars_packed_lin<2>", "k_solve_vars_packed_lin<4>", "k_solve_vars_packed_lin<8>",
        "k_solve_vars_packed_lin<16>"},
       {"k_solve_vars_packed_lin<1>/gcd", "k_solve_vars_packed_lin<2>/gcd", "k_solve_vars_packed_lin<4>/gcd",
        "k_solve_vars_packed_lin<8>/gcd", "k_solve_vars_packed_lin<16>/gcd"}}};
  const char* const* name = names[t.lin ? 1 : 0][gcd ? 1 : 0];
  switch (W) {
    case 16: launch_packed<16>(s, name[4], a, t, ex, form); break;
    case 8: launch_packed<8>(s, name[3], a, t, ex, form); break;
    case 4: launch_packed<4>(s, name[2], a, t, ex, form); break;
    case 2: launch_packed<2>(s, name[1], a, t, ex, form); break;
    default: launch_packed<1>(s, name[0], a, t, ex, form); W = 1; break;
  }
  count_launch(a.count, W);
  count_inverse(form);
}

void pub_inputs_launch(hipStream_t s, uint32_t count, const fe* d_vars, size_t vars_stride, const uint32_t* d_wire_vars,
                       const fe* d_sel, size_t n, uint32_t num_inputs, const uint32_t* d_which, fe* d_pub, size_t pub_stride) {
  const size_t lanes = (size_t)count * num_inputs;
  if (!lanes) return;
  launch("k_pub_inputs", k_pub_inputs, dim3((uint32_t)((lanes + kSolveThreads - 1) / kSolveThreads)), dim3(kSolveThreads), 0, s,
         d_vars, vars_stride, d_wire_vars, d_sel, n, num_inputs, d_which, count, d_pub, pub_stride);
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

void fr_inverse_launch(hipStream_t s, const fe* d_in, fe* d_out, size_t count, const sv29::Exps& ex) {
  const int form = inverse_form_setting();
  const dim3 grid((uint32_t)((count + kSolveThreads - 1) / kSolveThreads)), block(kSolveThreads);
  if (form == sv29::kInvGcd)
    launch("k_fr_inverse/gcd", k_fr_inverse<sv29::kInvGcd>, grid, block, 0, s, d_in, d_out, count, ex);
  else
    launch("k_fr_inverse", k_fr_inverse<sv29::kInvFermat>, grid, block, 0, s, d_in, d_out, count, ex);
  count_inverse(form);
}

}  // namespace pk
}  // namespace cap

// ---- the C ABI of the inverse form and the batch inverse ------------------------------------------------------------
using namespace cap;
using namespace cap::pk;

namespace {
const sv29::Exps* inverse_exps() {
  static const struct Derived {
    sv29::Exps ex;
    bool ok;
    Derived() { ok = sv29::derive_exps(&ex); }
  } d;
  return d.ok ? &d.ex : nullptr;
}
// elements of one launch: the grid's x dimension holds 2^31 - 1 workgroups
constexpr size_t kMaxBatch = (size_t)0x7fffffffu * kSolveThreads;

int inverse_batch(const char* who, const void* h_in, void* h_out, const void* d_in, void* d_out, size_t count) {
  if (count && (!(h_in || d_in) || !(h_out || d_out))) {
    set_error("%s: bad argument (a NULL array with count = %zu)", who, count);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (count > kMaxBatch) {
    set_error("%s: %zu elements are more than one launch takes (%zu)", who, count, kMaxBatch);
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  if (count == 0) return CAPGPU_OK;
  const sv29::Exps* ex = inverse_exps();
  if (!ex) {
    set_error("%s: the exponent r - 2 could not be derived", who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  Context& c = ctx();
  Entry lk(c);
  hipStream_t s = c.stream;
  if (h_in) {
    if (int rc = scratch_reserve(c.stage_b, sizeof(fe) * count + 256)) return rc;
    fe* buf = (fe*)c.stage_b.p;
    CAP_HIP(hipMemcpyAsync(buf, h_in, sizeof(fe) * count, hipMemcpyHostToDevice, s));
    fr_inverse_launch(s, buf, buf, count, *ex);
    CAP_HIP(hipMemcpyAsync(h_out, buf, sizeof(fe) * count, hipMemcpyDeviceToHost, s));
    CAP_HIP(hipStreamSynchronize(s));
  } else {
    fr_inverse_launch(s, (const fe*)d_in, (fe*)d_out, count, *ex);
  }
  return take_launch_error();
}
}  // namespace

extern "C" {

int capgpu_fr_set_inverse_form(int form) {
  if (form != CAPGPU_INVERSE_FERMAT && form != CAPGPU_INVERSE_GCD) {
    set_error("capgpu_fr_set_inverse_form: %d is neither CAPGPU_INVERSE_FERMAT (0) nor CAPGPU_INVERSE_GCD (1)", form);
    return CAPGPU_ERR_INVALID_ARG;
  }
  g_inverse_form.store(form, std::memory_order_relaxed);
  return CAPGPU_OK;
}
int capgpu_fr_get_inverse_form(int* form_out) {
  if (!form_out) {
    set_error("capgpu_fr_get_inverse_form: bad argument (form_out is NULL)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  *form_out = inverse_form_setting();
  return CAPGPU_OK;
}
int capgpu_fr_inverse_batch(const void* h_in, void* h_out, size_t count) {
  return inverse_batch("capgpu_fr_inverse_batch", h_in, h_out, nullptr, nullptr, count);
}
int capgpu_fr_inverse_batch_dev(const void* d_in, void* d_out, size_t count) {
  return inverse_batch("capgpu_fr_inverse_batch_dev", nullptr, nullptr, d_in, d_out, count);
}
int capgpu_fr_inverse_stats(uint64_t* fermat_launches_out, uint64_t* gcd_launches_out) {
  if (fermat_launches_out) *fermat_launches_out = g_inv_launches[sv29::kInvFermat].load();
  if (gcd_launches_out) *gcd_launches_out = g_inv_launches[sv29::kInvGcd].load();
  return CAPGPU_OK;
}

}  // extern "C"
