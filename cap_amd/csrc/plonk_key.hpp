// A proving key as the library keeps it, and the witness solver's schedule a key may carry: host data only (the device
// tables are pointers).  Every unit of the prover includes this - plonk.hip, which launches on the tables and holds keys
// for the length of a call, and the two units without device code: plonk_keys.hip, which builds, registers and serializes
// keys, and plonk_solver.hip, which gives them their solver.  Below the types: what those two units offer.
#pragma once
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "context.hpp"
#include "host_util.hpp"
#include "solve.hpp"
#include "solve_defer.hpp"

namespace cap {

// The shape of a TurboPlonk key for the units that do not see plonk_kernels.hpp: pk::NW, pk::NS, pk::kPkcCols and
// pk::QuotConst under the names the moved code uses.  plonk.hip sees both sets and asserts that they agree
// (prove_run.hpp: quot_const).
namespace ks {
constexpr int NW = kNumWires;              // wire types
constexpr int NS = kNumSelectors;          // selectors
constexpr int kPkcCols = NS + NW + NW - 1;  // columns of a key's coset table: 13 selectors, 5 sigmas, 4 x k_j x
struct QuotConst {
  fe g;          // coset generator 5 (Montgomery)
  fe k[NW];      // wire-subset separators
  fe zh_inv[8];  // 1 / ((g * w_m^i)^n - 1), i mod 6 (m = 6n: six distinct values)
};
}  // namespace ks

// The witness solver's schedule (capgpu_plonk_key_set_given): the host copy, shared by a key and its replicas; every
// ProvingKey object uploads its own device copy on first use (solve_tables).
struct SolveSched {
  uint64_t uid = 0;  // never reused: tells a key's device copy which schedule it holds
  sp::Plan plan;
  std::vector<fe> konst;  // per row of plan.rows: 1 / q_o or 1 / q_hash_i, internal form, canonical
  capgpu_solver_info info{};
  capgpu_hint_info hint_info{};  // all zero: no hints
  capgpu_solver_rules_info rules{};  // capgpu_plonk_key_set_solver's flags and what they admitted
  int auto_pack = 1;  // the schedule's term of the automatic witnesses-per-workgroup rule (spk::auto_pack)
  // The form the launches run (capgpu_plonk_key_set_solve_form).  Every set-up call makes a DIRECT schedule; the host copies
  // of the table and of the selectors' zero flags stay with it, so that a change of form is a host pass.
  int form = CAPGPU_SOLVE_FORM_DIRECT;
  std::vector<uint32_t> table;    // [5][n]
  std::vector<uint8_t> sel_zero;  // [13][n]
  sd::Sched defer;                // form == CAPGPU_SOLVE_FORM_DEFERRED: the schedule the kernels read (solve_defer.hpp)
  std::vector<fe> defer_konst;    // ... and its items' constants
};

struct ProvingKey {
  size_t n = 0, m = 0, ps = 0;  // domain, quotient domain, polynomial stride (n + 8)
  uint32_t log_n = 0, log_m = 0;
  size_t num_inputs = 0;
  uint64_t srs_handle = 0;
  fe* coef = nullptr;      // [18][ps]: 13 selector + 5 sigma polynomials (coefficients)
  fe* sig_eval = nullptr;  // [5][n]
  fe* pk_coset = nullptr;  // [22][m]: 13 selectors, 5 sigmas, k_j x for j = 1 .. 4 (pk::kPkcCols)
  fe* inv_nx1 = nullptr;   // [m]
  ks::QuotConst qc;    // arkworks form (host arithmetic, k_perm_numden)
  ks::QuotConst qc29;  // internal form of the lazy field (k_quotient)
  capgpu_verifying_key vk;
  std::vector<uint8_t> vk_bytes;
  bool recompute = false;
  int device = 0;  // HIP device the tables live on
  uint64_t uid = next_uid();  // never reused: identifies the key's tables in the signature of a captured graph
  static uint64_t next_uid() {
    static std::atomic<uint64_t> n{1};
    return n.fetch_add(1);
  }
  // Immutable once published: contexts on the same device share the object, other devices get a peer copy
  // (clone_key_to_current).  The batch workspace lives in the context (Context::prove_ws).
  // The one exception: the tables of the witness check (key_check_tables), derived on the first check of this key on this
  // device under chk_mu, read-only afterwards, freed with the key.  A replica on another device derives its own.
  mutable std::mutex chk_mu;
  mutable fe* chk_sel = nullptr;         // [13][n] selector VALUES on the domain, internal form (13.6 MB at n = 2^15)
  mutable uint32_t* chk_perm = nullptr;  // [5 n] index form of the extended permutation: cell i n + j -> i' n + j'
  mutable int chk_rc = 1;                // 1: not derived yet; CAPGPU_OK: ready; < 0: sigma was refused (chk_err), for good
  mutable std::string chk_err;
  // The wire -> variable table of CAPGPU_INPUT_VARS ([5 n] ids below num_vars; null / 0: the key has none).  Set before the
  // key is published (capgpu_plonk_preprocess_vars, replicas) or attached later by capgpu_plonk_key_set_vars, which must
  // not run beside calls that use the key; a table it replaces is freed once every context's stream has drained.  A key
  // with a table has chk_perm from the start - the permutation's index form is what the table was turned into.
  mutable uint32_t* wire_vars = nullptr;
  mutable size_t num_vars = 0;
  // The solver's schedule (null: none) and this object's device copy of it, one allocation, made under chk_mu by the first
  // solve that finds solve_dev_uid != solve->uid.  Set, replaced and dropped like the table (not beside calls that use the key).
  mutable std::shared_ptr<const SolveSched> solve;
  mutable void* solve_dev = nullptr;
  mutable uint64_t solve_dev_uid = 0;
  mutable pk::SolveTables solve_tab{};
  ProvingKey() = default;
  ProvingKey(const ProvingKey&) = delete;
  ProvingKey& operator=(const ProvingKey&) = delete;
  ~ProvingKey() {
    for (void* p : {(void*)coef, (void*)sig_eval, (void*)pk_coset, (void*)inv_nx1, (void*)chk_sel, (void*)chk_perm,
                    (void*)wire_vars, solve_dev})
      if (p) hipFree(p);
  }
};

// ---- the key registry (plonk_keys.hip; lookup_key and clone_key_to_current: context.hpp) -------------------------------
// the registry's (home) copy of a key, without replicating it
int home_key(uint64_t h, std::shared_ptr<ProvingKey>* out);
// The key of a part on the current context.  `home` (tickets only): the reference the ticket took at submission - a key
// freed since then (capgpu_plonk_free_key with the ticket outstanding) is proved from that reference instead of refused.
int part_key(uint64_t h, const std::shared_ptr<ProvingKey>* home, std::shared_ptr<ProvingKey>* out);

// ---- the witness solver's set-up (plonk_solver.hip), for the given-value calls ------------------------------------------
const sv29::Exps* solve_exps();  // null: the scalar field has no fifth-root exponent
int solve_pack_setting();        // capgpu_plonk_set_solve_pack, or the process default
// The device copy of K's schedule on K's device (the current one), uploaded on the first solve after a set_given.
int solve_tables(const ProvingKey& K, pk::SolveTables* tab, std::shared_ptr<const SolveSched>* hold);

}  // namespace cap
