// The witness solver's set-up and calls (solve_plan.hpp, solve29.hpp; the kernels: solve_kernels.hpp, compiled in
// solve.hip): capgpu_plonk_key_set_given* and _set_solver, the form of a schedule, a key's device copy of it, and
// capgpu_plonk_solve_vars* / _pub_inputs*.  No device code: the launches are solve.hip's (solve.hpp), the key's tables
// come from plonk.hip through prover.hpp, so a change here recompiles no kernel.  The given-value calls, which stand in
// plonk.hip with the rest of the proving entry points, take a key's tables from here (plonk_key.hpp: solve_tables).
// This unit does field29.hpp arithmetic on the host (solve_batch_inverse, the constants of key_set_given) and compiles
// it with the header's default multiplication schedule, not plonk.hip's CAP_FL_SCHED: the macro selects the order in
// which Fl::mul adds its partial products - same arithmetic, same results, same bounds (field29.hpp) - and no
// representation; every value that leaves this unit is packed to canonical words first.
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

#include "context.hpp"
#include "field29.hpp"
#include "host_util.hpp"
#include "plonk_key.hpp"
#include "prover.hpp"
#include "solve.hpp"
#include "solve_defer.hpp"

namespace cap {

using namespace pk;
using namespace ks;

// ---- the witness solver (solve_plan.hpp, solve29.hpp, solve_kernels.hpp) ----------------------------------------------
const sv29::Exps* solve_exps() {
  static const struct Derived {
    sv29::Exps ex;
    bool ok;
    Derived() { ok = sv29::derive_exps(&ex); }
  } d;
  return d.ok ? &d.ex : nullptr;
}

// capgpu_plonk_set_solve_pack: witnesses per workgroup of the solver's launches; 0: the automatic rule (solve_pack.hpp).
// -1: the process default (CAPGPU_SOLVE_PACK; a value that is no setting counts as 0)
static std::atomic<int> g_solve_pack{-1};
int solve_pack_setting() {
  static const int env_default = [] {
    const int e = env_int("CAPGPU_SOLVE_PACK", 0);
    return spk::valid_setting(e) ? e : 0;
  }();
  const int m = g_solve_pack.load(std::memory_order_relaxed);
  return m < 0 ? env_default : m;
}

// 1 / x for every x of v (internal form, none zero), in place: one inversion and three products per element
static void solve_batch_inverse(std::vector<fl>& v) {
  if (v.empty()) return;
  std::vector<fl> pre(v.size());
  fl acc = Fr29::one();
  for (size_t i = 0; i < v.size(); i++) {
    pre[i] = acc;
    acc = Fr29::mul(acc, v[i]);
  }
  acc = Fr29::inv(acc);
  for (size_t i = v.size(); i-- > 0;) {
    const fl x = v[i];
    v[i] = Fr29::mul(acc, pre[i]);
    acc = Fr29::mul(acc, x);
  }
}

// The device copy of K's schedule on K's device (the current one), uploaded on the first solve after a set_given.
int solve_tables(const ProvingKey& K, SolveTables* tab, std::shared_ptr<const SolveSched>* hold) {
  std::lock_guard<std::mutex> lk(K.chk_mu);
  if (!K.solve || !K.wire_vars) {
    set_error("capgpu_plonk_solve_vars: the key has no solver (capgpu_plonk_key_set_given gives it one)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  const SolveSched& S = *K.solve;
  *hold = K.solve;
  if (K.solve_dev_uid != S.uid) {
    if (K.solve_dev) {
      CAP_HIP(hipFree(K.solve_dev));  // (waits for the device: a launch may still read the tables that leave)
      K.solve_dev = nullptr;
      K.solve_dev_uid = 0;
    }
    // (the DEFERRED form: the deferred schedule's items, constants and levels take the direct ones' places)
    const bool defer = S.form == CAPGPU_SOLVE_FORM_DEFERRED;
    const std::vector<sp::Row>& h_rows = defer ? S.defer.rows : S.plan.rows;
    const std::vector<fe>& h_konst = defer ? S.defer_konst : S.konst;
    const std::vector<uint32_t>& h_off = defer ? S.defer.level_off : S.plan.level_off;
    const size_t nrows = h_rows.size();
    int32_t* dslot = nullptr;
    uint32_t* flush_vars = nullptr;
    int32_t* slot = nullptr;
    sp::Row* rows = nullptr;
    fe* konst = nullptr;
    uint32_t* off = nullptr;
    sp::Hint* hints = nullptr;
    uint32_t* targets = nullptr;
    const size_t nhints = S.plan.hints.size(), ntargets = S.plan.targets.size();
    auto carve_tables = [&](void* at) {
      Carver k(at);
      slot = k.take<int32_t>(S.plan.slot.size());
      rows = k.take<sp::Row>(nrows ? nrows : 1);
      konst = k.take<fe>(nrows ? nrows : 1);
      off = k.take<uint32_t>(h_off.size());
      if (nhints) {
        hints = k.take<sp::Hint>(nhints);
        targets = k.take<uint32_t>(ntargets);
      }
      if (defer) {
        dslot = k.take<int32_t>(S.defer.dslot.size() ? S.defer.dslot.size() : 1);
        flush_vars = k.take<uint32_t>(S.defer.flush_vars.size() ? S.defer.flush_vars.size() : 1);
      }
      return k.off + 256;
    };
    DevTmp<char> own;
    CAP_HIP(own.alloc(carve_tables(nullptr)));
    (void)carve_tables(own.p);
    CAP_HIP(hipMemcpy(slot, S.plan.slot.data(), sizeof(int32_t) * S.plan.slot.size(), hipMemcpyHostToDevice));
    if (nrows) {
      CAP_HIP(hipMemcpy(rows, h_rows.data(), sizeof(sp::Row) * nrows, hipMemcpyHostToDevice));
      CAP_HIP(hipMemcpy(konst, h_konst.data(), sizeof(fe) * nrows, hipMemcpyHostToDevice));
    }
    CAP_HIP(hipMemcpy(off, h_off.data(), sizeof(uint32_t) * h_off.size(), hipMemcpyHostToDevice));
    if (defer) {
      if (!S.defer.dslot.empty())
        CAP_HIP(hipMemcpy(dslot, S.defer.dslot.data(), sizeof(int32_t) * S.defer.dslot.size(), hipMemcpyHostToDevice));
      if (!S.defer.flush_vars.empty())
        CAP_HIP(hipMemcpy(flush_vars, S.defer.flush_vars.data(), sizeof(uint32_t) * S.defer.flush_vars.size(),
                          hipMemcpyHostToDevice));
    }
    if (nhints) {
      CAP_HIP(hipMemcpy(hints, S.plan.hints.data(), sizeof(sp::Hint) * nhints, hipMemcpyHostToDevice));
      CAP_HIP(hipMemcpy(targets, S.plan.targets.data(), sizeof(uint32_t) * ntargets, hipMemcpyHostToDevice));
    }
    SolveTables t{};
    t.slot = slot;
    t.rows = rows;
    t.konst = konst;
    t.level_off = off;
    t.hp.hints = hints;
    t.hp.targets = targets;
    t.levels = (uint32_t)(defer ? S.defer.levels : S.plan.levels);
    t.num_given = S.plan.num_given;
    t.lin = S.plan.lin_rows != 0;
    t.defer = defer;
    t.dslot = dslot;
    t.flush_vars = flush_vars;
    t.side_slots = defer ? (size_t)S.defer.slots : 0;
    K.solve_tab = t;
    K.solve_dev = own.p;
    K.solve_dev_uid = S.uid;
    own.p = nullptr;
  }
  *tab = K.solve_tab;
  tab->wire_vars = K.wire_vars;
  tab->sel = K.chk_sel;
  tab->n = K.n;
  tab->num_vars = K.num_vars;
  return CAPGPU_OK;
}

// `count` witnesses on the current context: given values and the result in host memory (h_*) or resident (d_*)
static int solve_run(uint64_t pk_handle, uint32_t count, const uint64_t* h_given, uint64_t* h_vars, const void* d_given,
                     void* d_vars, capgpu_solve_status* status_out) {
  Context& c = ctx();
  Entry lk(c);
  std::shared_ptr<ProvingKey> K;
  int rc = lookup_key(pk_handle, &K);
  if (rc) return rc;
  const sv29::Exps* ex = solve_exps();
  if (!ex) {
    set_error("capgpu_plonk_solve_vars: (r - 1) mod 5 != 1: the scalar field has no fifth-root exponent");
    return CAPGPU_ERR_INVALID_ARG;
  }
  {
    std::lock_guard<std::mutex> klk(K->chk_mu);
    if (!K->solve || !K->wire_vars) {
      set_error("capgpu_plonk_solve_vars: the key has no solver (capgpu_plonk_key_set_given gives it one)");
      return CAPGPU_ERR_INVALID_ARG;
    }
  }
  if ((rc = key_check_tables(*K))) return rc;  // the selector values on the domain (derived once per key)
  SolveTables tab;
  std::shared_ptr<const SolveSched> hold;
  if ((rc = solve_tables(*K, &tab, &hold))) return rc;
  hipStream_t s = c.stream;
  const size_t given_elems = (size_t)count * tab.num_given, var_elems = (size_t)count * tab.num_vars;
  unsigned long long* d_st = nullptr;
  fe *g = nullptr, *v = nullptr, *side = nullptr;
  auto carve_call = [&](void* at) {
    Carver k(at);
    d_st = k.take<unsigned long long>(count);
    if (h_given) g = k.take<fe>(given_elems ? given_elems : 1);
    if (h_vars) v = k.take<fe>(var_elems);
    if (tab.defer) side = k.take<fe>(tab.side_elems(count) + 1);  // (a key in the DEFERRED form: its denominators)
    return k.off + 256;
  };
  if ((rc = scratch_reserve(c.stage_b, carve_call(nullptr)))) return rc;
  (void)carve_call(c.stage_b.p);
  if (h_given) {
    if (given_elems) CAP_HIP(hipMemcpyAsync(g, h_given, sizeof(fe) * given_elems, hipMemcpyHostToDevice, s));
    d_given = g;
  }
  if (h_vars) d_vars = v;
  CAP_HIP(hipMemsetAsync(d_st, 0xff, sizeof(unsigned long long) * count, s));
  solve_launch_packed(s, spk::pack_for(solve_pack_setting(), hold->auto_pack, count),
                      SolveLaunch{count, (const fe*)d_given, tab.num_given, (fe*)d_vars, tab.num_vars, d_st, nullptr, side}, tab,
                      *ex);
  std::vector<unsigned long long> h_st(count);
  CAP_HIP(hipMemcpyAsync(h_st.data(), d_st, sizeof(unsigned long long) * count, hipMemcpyDeviceToHost, s));
  if (h_vars) CAP_HIP(hipMemcpyAsync(h_vars, d_vars, sizeof(fe) * var_elems, hipMemcpyDeviceToHost, s));
  CAP_HIP(hipStreamSynchronize(s));
  if ((rc = take_launch_error())) return rc;
  for (uint32_t p = 0; p < count; p++) {
    capgpu_solve_status& o = status_out[p];
    memset(&o, 0, sizeof o);
    if (h_st[p] != kSolved) {
      o.kind = 1;
      o.row = h_st[p];
    }
  }
  return CAPGPU_OK;
}

static_assert(sizeof(capgpu_hint) == sizeof(sp::Hint) && sizeof(capgpu_hint) == 16 && sizeof(capgpu_hint_info) == 48 &&
                  offsetof(capgpu_hint, kind) == offsetof(sp::Hint, kind) && offsetof(capgpu_hint, src) == offsetof(sp::Hint, src) &&
                  offsetof(capgpu_hint, first) == offsetof(sp::Hint, first) &&
                  offsetof(capgpu_hint, count) == offsetof(sp::Hint, count),
              "capgpu_hint is sp::Hint");
static_assert(CAPGPU_HINT_BITS == sp::HINT_BITS && CAPGPU_HINT_INV0 == sp::HINT_INV0 && CAPGPU_HINT_ISZERO == sp::HINT_ISZERO,
              "hint kinds");

static_assert(sizeof(capgpu_solver_rules_info) == 32, "capgpu_solver_rules_info");
static_assert(CAPGPU_SOLVER_LINEAR == sp::RULE_LINEAR && CAPGPU_SOLVER_DERIVE_PUBLIC == sp::RULE_DERIVE_PUBLIC, "solver flags");

// capgpu_plonk_key_set_given (who names it, no hints), capgpu_plonk_key_set_given_hints (both: flags 0) and
// capgpu_plonk_key_set_solver
static int key_set_given(const char* who, uint64_t pk_handle, const uint32_t* given_vars, size_t num_given,
                         const capgpu_hint* hints, size_t num_hints, const uint32_t* targets, size_t num_targets,
                         uint32_t flags, capgpu_solver_info* info_out, capgpu_hint_info* hint_info_out) {
  if (flags & ~sp::kRuleFlags) {
    set_error("%s: bad argument (flags 0x%x: the known bits are CAPGPU_SOLVER_LINEAR (1) and CAPGPU_SOLVER_DERIVE_PUBLIC (2))", who,
              flags);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (!given_vars && num_given) {
    set_error("%s: bad argument (given_vars is NULL)", who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if ((!hints && num_hints) || (!targets && num_targets)) {
    set_error("%s: bad argument (%s is NULL)", who, !hints && num_hints ? "hints" : "targets");
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (num_hints >= (1ull << 32) || num_targets >= (1ull << 32)) {
    set_error("%s: bad argument (num_hints and num_targets are below 2^32)", who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  std::shared_ptr<ProvingKey> K;
  int rc = home_key(pk_handle, &K);
  if (rc) return rc;
  if (!K->wire_vars) {
    set_error("%s: the key has no wire -> variable table (capgpu_plonk_preprocess_vars makes a key with one, "
              "capgpu_plonk_key_set_vars gives it one); the key is unchanged",
              who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (!solve_exps()) {
    set_error("%s: (r - 1) mod 5 != 1: the scalar field has no fifth-root exponent", who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  Runtime& R = rt();
  Context* home = nullptr;
  for (auto& cp : R.ctxs)
    if (cp->device == K->device) {
      home = cp.get();
      break;
    }
  if (!home) {
    set_error("%s: no context on the key's device %d", who, K->device);
    return CAPGPU_ERR_BAD_HANDLE;
  }
  auto S = std::make_shared<SolveSched>();
  {
    ScopedCtx sc(*home);
    Entry lk(*home);
    hipStream_t s = home->stream;
    const size_t n = K->n, cells = (size_t)NW * n, num_vars = K->num_vars;
    if ((rc = key_check_tables(*K))) return rc;
    // the table and the selector values, read back once (0.66 MB and 13.6 MB at n = 2^15)
    std::vector<uint32_t> table(cells);
    std::vector<fe> sel((size_t)NS * n);
    CAP_HIP(hipMemcpyAsync(table.data(), K->wire_vars, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, s));
    CAP_HIP(hipMemcpyAsync(sel.data(), K->chk_sel, sizeof(fe) * NS * n, hipMemcpyDeviceToHost, s));
    CAP_HIP(hipStreamSynchronize(s));
    std::vector<uint8_t> sel_zero((size_t)NS * n);
    for (size_t i = 0; i < sel.size(); i++) sel_zero[i] = Fr29::is_zero(Fr29::load(sel[i])) ? 1 : 0;
    if (!sp::solve_plan_rules(n, K->num_inputs, num_vars, table.data(), sel_zero.data(), given_vars, num_given,
                              (const sp::Hint*)hints, num_hints, targets, num_targets, flags, &S->plan)) {
      set_error("%s: %s; the key is unchanged", who, S->plan.error.c_str());
      return CAPGPU_ERR_INVALID_ARG;
    }
    const sp::Plan& P = S->plan;
    std::vector<fl> inv;
    std::vector<size_t> where;
    for (size_t k = 0; k < P.rows.size(); k++) {
      const uint32_t kind = sp::row_kind(P.rows[k]);
      if (kind == sp::OUT_INV || sp::is_hint_kind(kind)) continue;
      const int which = kind == sp::OUT_MUL ? sp::Q_O : (kind == sp::LIN ? sp::Q_LC : sp::Q_HASH) + (int)sp::row_wire(P.rows[k]);
      inv.push_back(Fr29::load(sel[(size_t)which * n + P.rows[k].row]));
      where.push_back(k);
    }
    solve_batch_inverse(inv);
    S->konst.assign(P.rows.size(), Fr29::pack(Fr29::zero()));
    for (size_t i = 0; i < inv.size(); i++) S->konst[where[i]] = Fr29::pack(Fr29::canonical(inv[i]));
    static std::atomic<uint64_t> next_uid{1};
    S->uid = next_uid.fetch_add(1);
    S->info = capgpu_solver_info{P.num_given, P.num_defined, P.levels, P.widest_level, P.inv_rows, P.root_rows};
    S->hint_info = capgpu_hint_info{P.hints.size(), P.num_hinted, P.bits_hints, P.inv_hints, P.iszero_hints, P.hint_items};
    S->rules = capgpu_solver_rules_info{P.flags, P.lin_rows, P.derived_inputs, 0};
    S->auto_pack = spk::auto_pack(spk::median_level_width(P.level_off.data(), P.levels), kSolveThreads);
    S->table = std::move(table);
    S->sel_zero = std::move(sel_zero);
  }
  // the key and the replicas other devices hold take the schedule; each uploads its tables on its next solve
  for (auto& cp : R.ctxs) {
    Context& c = *cp;
    ScopedCtx sc(c);
    Entry lk(c);
    auto it = c.keys.find(pk_handle);
    ProvingKey* k = it == c.keys.end() ? (cp.get() == home ? K.get() : nullptr) : it->second.get();
    if (!k) continue;
    std::lock_guard<std::mutex> klk(k->chk_mu);
    k->solve = S;
  }
  {
    std::lock_guard<std::mutex> klk(K->chk_mu);
    K->solve = S;
  }
  if (info_out) *info_out = S->info;
  if (hint_info_out) *hint_info_out = S->hint_info;
  return CAPGPU_OK;
}

// ---- the form of the solver's schedule (solve_defer.hpp) ---------------------------------------------------------------
static_assert(sizeof(capgpu_solve_form_info) == 64, "capgpu_solve_form_info");
// the figures of S in the form it holds; D: the deferred schedule of S's plan (S.defer, or one derived for the figures)
static capgpu_solve_form_info solve_form_figures(const SolveSched& S, const sd::Sched& D) {
  if (S.form == CAPGPU_SOLVE_FORM_DEFERRED)
    return capgpu_solve_form_info{CAPGPU_SOLVE_FORM_DEFERRED, D.deferred_vars, D.frac_rows, D.flush_levels, D.flush_items,
                                  D.levels, D.inv_levels_direct, D.inv_levels_deferred};
  return capgpu_solve_form_info{CAPGPU_SOLVE_FORM_DIRECT, 0, 0, 0, 0, S.plan.levels, D.inv_levels_direct, D.inv_levels_deferred};
}

// capgpu_plonk_pub_inputs[_dev]: host arrays (h_*) staged through the context's scratch, or resident ones (d_*)
static int pub_inputs_run(const char* who, uint64_t pk_handle, int count, const uint64_t* h_vars, uint64_t* h_pub,
                          const void* d_vars, void* d_pub) {
  if (count < 0 || (count && (!(h_vars || d_vars) || !(h_pub || d_pub)))) {
    set_error("%s: bad argument (count >= 0; a NULL array with count = %d)", who, count);
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  Context& c = ctx();
  Entry lk(c);
  std::shared_ptr<ProvingKey> K;
  int rc = lookup_key(pk_handle, &K);
  if (rc) return rc;
  if (!K->wire_vars) {
    set_error("%s: the key has no wire -> variable table (capgpu_plonk_preprocess_vars makes a key with one, "
              "capgpu_plonk_key_set_vars gives it one)",
              who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (count == 0 || K->num_inputs == 0) return CAPGPU_OK;
  if ((rc = key_check_tables(*K))) return rc;  // the selector values on the domain (derived once per key)
  hipStream_t s = c.stream;
  const size_t ni = K->num_inputs, var_elems = (size_t)count * K->num_vars, pub_elems = (size_t)count * ni;
  if (h_vars) {
    fe *v = nullptr, *p = nullptr;
    auto carve_call = [&](void* at) {
      Carver k(at);
      v = k.take<fe>(var_elems);
      p = k.take<fe>(pub_elems);
      return k.off + 256;
    };
    if ((rc = scratch_reserve(c.stage_b, carve_call(nullptr)))) return rc;
    (void)carve_call(c.stage_b.p);
    CAP_HIP(hipMemcpyAsync(v, h_vars, sizeof(fe) * var_elems, hipMemcpyHostToDevice, s));
    pub_inputs_launch(s, (uint32_t)count, v, K->num_vars, K->wire_vars, K->chk_sel, K->n, (uint32_t)ni, nullptr, p, ni);
    CAP_HIP(hipMemcpyAsync(h_pub, p, sizeof(fe) * pub_elems, hipMemcpyDeviceToHost, s));
    CAP_HIP(hipStreamSynchronize(s));
  } else {
    pub_inputs_launch(s, (uint32_t)count, (const fe*)d_vars, K->num_vars, K->wire_vars, K->chk_sel, K->n, (uint32_t)ni, nullptr,
                      (fe*)d_pub, ni);
  }
  return take_launch_error();
}

}  // namespace cap

using namespace cap;

extern "C" {

int capgpu_plonk_key_set_given(uint64_t pk_handle, const uint32_t* given_vars, size_t num_given,
                               capgpu_solver_info* info_out) {
  return key_set_given("capgpu_plonk_key_set_given", pk_handle, given_vars, num_given, nullptr, 0, nullptr, 0, 0, info_out, nullptr);
}

int capgpu_plonk_key_set_given_hints(uint64_t pk_handle, const uint32_t* given_vars, size_t num_given,
                                     const capgpu_hint* hints, size_t num_hints, const uint32_t* targets,
                                     size_t num_targets, capgpu_solver_info* info_out, capgpu_hint_info* hint_info_out) {
  return key_set_given("capgpu_plonk_key_set_given_hints", pk_handle, given_vars, num_given, hints, num_hints, targets,
                       num_targets, 0, info_out, hint_info_out);
}

int capgpu_plonk_key_set_solver(uint64_t pk_handle, const uint32_t* given_vars, size_t num_given, const capgpu_hint* hints,
                                size_t num_hints, const uint32_t* targets, size_t num_targets, uint32_t flags,
                                capgpu_solver_info* info_out, capgpu_hint_info* hint_info_out) {
  // (flags 0: the refusals open with the older call's name - the same texts)
  return key_set_given(flags ? "capgpu_plonk_key_set_solver" : "capgpu_plonk_key_set_given_hints", pk_handle, given_vars,
                       num_given, hints, num_hints, targets, num_targets, flags, info_out, hint_info_out);
}

int capgpu_plonk_key_solver_rules_info(uint64_t pk_handle, capgpu_solver_rules_info* info_out) {
  if (!info_out) {
    set_error("capgpu_plonk_key_solver_rules_info: bad argument (info_out is NULL)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  std::shared_ptr<ProvingKey> K;
  int rc = home_key(pk_handle, &K);
  if (rc) return rc;
  std::lock_guard<std::mutex> klk(K->chk_mu);
  memset(info_out, 0, sizeof *info_out);
  if (K->solve && K->wire_vars) *info_out = K->solve->rules;
  return CAPGPU_OK;
}

int capgpu_plonk_key_set_solve_form(uint64_t pk_handle, int form, capgpu_solve_form_info* info_out) {
  static const char who[] = "capgpu_plonk_key_set_solve_form";
  if (form != CAPGPU_SOLVE_FORM_DIRECT && form != CAPGPU_SOLVE_FORM_DEFERRED) {
    set_error("%s: bad argument (form %d is neither CAPGPU_SOLVE_FORM_DIRECT (0) nor CAPGPU_SOLVE_FORM_DEFERRED (1)); the key is "
              "unchanged",
              who, form);
    return CAPGPU_ERR_INVALID_ARG;
  }
  if (!pk_handle) {
    set_error("%s: bad argument (pk_handle is 0)", who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  std::shared_ptr<ProvingKey> K;
  int rc = home_key(pk_handle, &K);
  if (rc) return rc;
  std::shared_ptr<const SolveSched> old;
  {
    std::lock_guard<std::mutex> klk(K->chk_mu);
    if (K->solve && K->wire_vars) old = K->solve;
  }
  if (!old) {
    set_error("%s: the key has no solver (capgpu_plonk_key_set_given gives it one); the key is unchanged", who);
    return CAPGPU_ERR_INVALID_ARG;
  }
  // a new schedule object with a new uid: every holder uploads its tables again on its next solve
  auto S = std::make_shared<SolveSched>(*old);
  S->form = form;
  S->defer = sd::Sched();
  S->defer_konst.clear();
  const sp::Plan& P = S->plan;
  if (form == CAPGPU_SOLVE_FORM_DEFERRED) {
    sd::defer_plan(P, K->n, S->table.data(), S->sel_zero.data(), &S->defer);
    const sd::Sched& D = S->defer;
    S->defer_konst.assign(D.rows.size(), Fr29::pack(Fr29::zero()));
    for (size_t k = 0; k < D.rows.size(); k++)
      if (D.src[k] != sd::kNoSrc) S->defer_konst[k] = S->konst[D.src[k]];
    S->auto_pack = spk::auto_pack(spk::median_level_width(D.level_off.data(), D.levels), kSolveThreads);
  } else {
    S->auto_pack = spk::auto_pack(spk::median_level_width(P.level_off.data(), P.levels), kSolveThreads);
  }
  static std::atomic<uint64_t> next_uid{1ull << 40};  // (apart from the set-up calls' counter)
  S->uid = next_uid.fetch_add(1);
  Runtime& R = rt();
  for (auto& cp : R.ctxs) {
    Context& c = *cp;
    ScopedCtx sc(c);
    Entry lk(c);
    auto it = c.keys.find(pk_handle);
    if (it == c.keys.end()) continue;
    std::lock_guard<std::mutex> klk(it->second->chk_mu);
    if (it->second->solve) it->second->solve = S;
  }
  {
    std::lock_guard<std::mutex> klk(K->chk_mu);
    K->solve = S;
  }
  if (info_out) {
    if (form == CAPGPU_SOLVE_FORM_DEFERRED) {
      *info_out = solve_form_figures(*S, S->defer);
    } else {
      sd::Sched D;
      sd::defer_plan(P, K->n, S->table.data(), S->sel_zero.data(), &D);
      *info_out = solve_form_figures(*S, D);
    }
  }
  return CAPGPU_OK;
}

int capgpu_plonk_key_solve_form_info(uint64_t pk_handle, capgpu_solve_form_info* info_out) {
  if (!info_out || !pk_handle) {
    set_error("capgpu_plonk_key_solve_form_info: bad argument (%s)", info_out ? "pk_handle is 0" : "info_out is NULL");
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  std::shared_ptr<ProvingKey> K;
  int rc = home_key(pk_handle, &K);
  if (rc) return rc;
  std::shared_ptr<const SolveSched> S;
  {
    std::lock_guard<std::mutex> klk(K->chk_mu);
    if (K->solve && K->wire_vars) S = K->solve;
  }
  memset(info_out, 0, sizeof *info_out);
  if (!S) return CAPGPU_OK;
  if (S->form == CAPGPU_SOLVE_FORM_DEFERRED) {
    *info_out = solve_form_figures(*S, S->defer);
  } else {
    sd::Sched D;  // (the figures the other form would have: a host pass over the plan)
    sd::defer_plan(S->plan, K->n, S->table.data(), S->sel_zero.data(), &D);
    *info_out = solve_form_figures(*S, D);
  }
  return CAPGPU_OK;
}

int capgpu_plonk_pub_inputs(uint64_t pk_handle, int count, const uint64_t* vars, uint64_t* pub_out) {
  return pub_inputs_run("capgpu_plonk_pub_inputs", pk_handle, count, vars, pub_out, nullptr, nullptr);
}
int capgpu_plonk_pub_inputs_dev(uint64_t pk_handle, int count, const void* d_vars, void* d_pub_out) {
  return pub_inputs_run("capgpu_plonk_pub_inputs_dev", pk_handle, count, nullptr, nullptr, d_vars, d_pub_out);
}

int capgpu_plonk_key_hint_info(uint64_t pk_handle, capgpu_hint_info* info_out) {
  if (!info_out) {
    set_error("capgpu_plonk_key_hint_info: bad argument (info_out is NULL)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  std::shared_ptr<ProvingKey> K;
  int rc = home_key(pk_handle, &K);
  if (rc) return rc;
  std::lock_guard<std::mutex> klk(K->chk_mu);
  memset(info_out, 0, sizeof *info_out);
  if (K->solve && K->wire_vars) *info_out = K->solve->hint_info;
  return CAPGPU_OK;
}

int capgpu_plonk_key_solver_info(uint64_t pk_handle, capgpu_solver_info* info_out) {
  if (!info_out) {
    set_error("capgpu_plonk_key_solver_info: bad argument (info_out is NULL)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  std::shared_ptr<ProvingKey> K;
  int rc = home_key(pk_handle, &K);
  if (rc) return rc;
  std::lock_guard<std::mutex> klk(K->chk_mu);
  memset(info_out, 0, sizeof *info_out);
  if (K->solve && K->wire_vars) *info_out = K->solve->info;
  return CAPGPU_OK;
}

int capgpu_plonk_solve_vars(uint64_t pk_handle, int count, const uint64_t* given, uint64_t* vars_out,
                            capgpu_solve_status* status_out) {
  if (count < 0 || (count && (!given || !vars_out || !status_out))) {
    set_error("capgpu_plonk_solve_vars: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  if (count == 0) return CAPGPU_OK;
  return solve_run(pk_handle, (uint32_t)count, given, vars_out, nullptr, nullptr, status_out);
}

int capgpu_plonk_solve_vars_dev(uint64_t pk_handle, int count, const void* d_given, void* d_vars_out,
                                capgpu_solve_status* status_out) {
  if (count < 0 || (count && (!d_given || !d_vars_out || !status_out))) {
    set_error("capgpu_plonk_solve_vars: bad argument");
    return CAPGPU_ERR_INVALID_ARG;
  }
  CAP_CHECK_INIT();
  if (count == 0) return CAPGPU_OK;
  return solve_run(pk_handle, (uint32_t)count, nullptr, nullptr, d_given, d_vars_out, status_out);
}

int capgpu_plonk_set_solve_pack(int w) {
  if (!spk::valid_setting(w)) {
    set_error("capgpu_plonk_set_solve_pack: %d is none of 0 (automatic), 1, 2, 4, 8, 16", w);
    return CAPGPU_ERR_INVALID_ARG;
  }
  g_solve_pack.store(w, std::memory_order_relaxed);
  return CAPGPU_OK;
}
int capgpu_plonk_get_solve_pack(int* w_out) {
  if (!w_out) {
    set_error("capgpu_plonk_get_solve_pack: bad argument (w_out is NULL)");
    return CAPGPU_ERR_INVALID_ARG;
  }
  *w_out = solve_pack_setting();
  return CAPGPU_OK;
}
int capgpu_plonk_solve_stats(uint64_t* launches_out, uint64_t* witnesses_out, uint64_t* packed_launches_out) {
  CAP_CHECK_INIT();
  solve_stats(launches_out, witnesses_out, packed_launches_out);
  return CAPGPU_OK;
}

}  // extern "C"
