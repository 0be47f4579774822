// Host-side check of the witness solver's hints: cap_amd/csrc/solve_plan.hpp (the hint table, the firing step, the
// refusals) and cap_amd/csrc/solve29.hpp (the three hint rules) with field29.hpp's bound assertions on.  Stand-alone;
// prints one summary line that tests/test_solve_hints_host.py reads, "bad=0" when every check held.
//   - every hint refusal is met and names its hint index and variable; the row refusals still come first where they did
//   - firing order, levels, chains and the (level, kind, row or hint, chunk) order on a hand-made circuit
//   - without hints the plan is what the rule gave before hints existed (restated below as plan_before), field by field,
//     on random circuits
//   - random circuits that lay unpack / is_zero / is_equal the way a circuit builder does - boolean rows, a recomposition
//     chain whose last row outputs the SOURCE, the two rows over (a, a_inv, y) - on given and on computed sources, with an
//     inverse feeding a 254-bit decomposition: after a solve in plan order every bit equals its bit of from_mont(src), every
//     inverse times its source is 1 or both are 0, every flag tells whether its source is 0, and wc29::Check::gate holds at
//     EVERY row of the circuit, constraints included
//   - a packed workgroup emulated with solve_pack.hpp's decode over the same items at W = 1, 4, 16 and ragged counts gives
//     the lone solve's words
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/solve29.hpp"
#include "../../cap_amd/csrc/solve_pack.hpp"
#include "../../cap_amd/csrc/solve_plan.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace cap;
using C = wc29::Check<CAP_FL_SCHED>;
using S = sv29::Solve<CAP_FL_SCHED>;
using F = S::F;
constexpr uint32_t kThreads = 256;  // pk::kSolveThreads (solve.hpp needs HIP)

static int bad = 0;
#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      bad++;                                                  \
      printf("FAILED line %d: %s\n", __LINE__, #x);           \
    }                                                         \
  } while (0)

static uint64_t rng_state = 0x13198a2e03707344ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static fe plain_zero() {
  fe a;
  memset(&a, 0, sizeof a);
  return a;
}
static fe ext_of_plain(const fe& a) { return F::to_ext(F::to_mont(a)); }
static fe rnd_ext() {
  fe a;
  for (int i = 0; i < 8; i++) a.v[i] = (uint32_t)rnd();
  a.v[7] &= 0x0fffffffu;  // below 2^252 < r
  return ext_of_plain(a);
}
static fe ext_of(uint32_t x) {
  fe a = plain_zero();
  a.v[0] = x;
  return ext_of_plain(a);
}
static fe ext_pow2(uint32_t k) {  // 2^k, k < 254
  fe a = plain_zero();
  a.v[k / 32] = 1u << (k % 32);
  return ext_of_plain(a);
}
static fe ext_neg(const fe& x) { return F::to_ext(F::neg(F::from_ext(x))); }
static fe sel_of(const fe& ext) { return F::pack(F::canonical(F::from_ext(ext))); }
static bool same_words(const fe& a, const fe& b) { return !memcmp(&a, &b, sizeof a); }

struct Circuit {
  size_t n, num_inputs, num_vars;
  std::vector<uint32_t> wv;  // [5][n]
  std::vector<fe> sel;       // [13][n], device form
  std::vector<uint8_t> zero;
  std::vector<sp::Hint> hints;
  std::vector<uint32_t> targets;
  Circuit(size_t n_, size_t ni, size_t nv) : n(n_), num_inputs(ni), num_vars(nv), wv(5 * n_, 0), sel(13 * n_), zero(13 * n_, 1) {
    for (auto& s : sel) memset(&s, 0, sizeof s);
  }
  void set(int s, size_t j, const fe& ext) {
    sel[s * n + j] = sel_of(ext);
    zero[s * n + j] = F::is_zero(F::load(sel[s * n + j])) ? 1 : 0;
  }
  void wires(size_t j, uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t o) {
    const uint32_t w[5] = {a, b, c, d, o};
    for (int i = 0; i < 5; i++) wv[i * n + j] = w[i];
  }
  void hint(uint32_t kind, uint32_t src, const std::vector<uint32_t>& t) {
    hints.push_back(sp::Hint{kind, src, (uint32_t)targets.size(), (uint32_t)t.size()});
    targets.insert(targets.end(), t.begin(), t.end());
  }
  bool plan(const std::vector<uint32_t>& given, sp::Plan* P) const {
    return sp::solve_plan_hints(n, num_inputs, num_vars, wv.data(), zero.data(), given.data(), given.size(), hints.data(),
                                hints.size(), targets.data(), targets.size(), P);
  }
};

// ---- the rule before hints, restated: what a plan without hints must still be ------------------------------------------
struct Before {
  std::vector<sp::Row> rows;
  std::vector<uint32_t> level_off;
  uint64_t inv_rows = 0, root_rows = 0, widest = 0;
  bool ok = true;
};
static Before plan_before(const Circuit& c, const std::vector<uint32_t>& given) {
  Before B;
  std::vector<int32_t> level(c.num_vars, -1);
  for (uint32_t g : given) level[g] = 0;
  struct It {
    uint32_t level, kind, row, wire;
  };
  std::vector<It> its;
  auto z = [&](int s, size_t j) { return c.zero[s * c.n + j] != 0; };
  for (size_t j = 0; j < c.n; j++) {
    int32_t deepest = 0;
    int unknown = -1, cells = 0, wire = -1;
    bool two = false;
    for (int i = 0; i < 5; i++) {
      const uint32_t v = c.wv[i * c.n + j];
      if (level[v] >= 0) {
        deepest = std::max(deepest, level[v]);
      } else if (unknown >= 0 && (uint32_t)unknown != v) {
        two = true;
      } else {
        unknown = (int)v;
        cells++;
        wire = i;
      }
    }
    if (unknown < 0) continue;
    if (two || j < c.num_inputs || cells != 1) {
      B.ok = false;
      return B;
    }
    It it{(uint32_t)deepest + 1, 0, (uint32_t)j, (uint32_t)wire};
    if (wire == 4 && (!z(sp::Q_O, j) || !z(sp::Q_ECC, j)))
      it.kind = z(sp::Q_ECC, j) ? 0 : 1;
    else if (wire < 4 && !z(sp::Q_HASH + wire, j) && z(sp::Q_LC + wire, j) && z(sp::Q_MUL + wire / 2, j) && z(sp::Q_ECC, j))
      it.kind = 2;
    else {
      B.ok = false;
      return B;
    }
    level[unknown] = (int32_t)it.level;
    its.push_back(it);
  }
  std::sort(its.begin(), its.end(), [](const It& a, const It& b) {
    return a.level != b.level ? a.level < b.level : a.kind != b.kind ? a.kind < b.kind : a.row < b.row;
  });
  B.level_off.push_back(0);
  for (size_t k = 0; k < its.size(); k++) {
    while (B.level_off.size() < its[k].level) B.level_off.push_back((uint32_t)k);
    B.rows.push_back(sp::Row{its[k].row, its[k].kind | its[k].wire << 8});
    B.inv_rows += its[k].kind == 1;
    B.root_rows += its[k].kind == 2;
  }
  if (!its.empty()) B.level_off.push_back((uint32_t)its.size());
  for (size_t l = 0; l + 1 < B.level_off.size(); l++) B.widest = std::max<uint64_t>(B.widest, B.level_off[l + 1] - B.level_off[l]);
  return B;
}

// ---- the solve as the kernels run it -------------------------------------------------------------------------------------
struct Solver {
  const Circuit& c;
  sp::Plan P;
  std::vector<fe> konst;
  sv29::Exps ex;
  explicit Solver(const Circuit& c_) : c(c_) { CHECK(sv29::derive_exps(&ex)); }
  bool plan(const std::vector<uint32_t>& given) {
    if (!c.plan(given, &P)) return false;
    konst.assign(P.rows.size(), plain_zero());
    for (size_t k = 0; k < P.rows.size(); k++) {
      const uint32_t kind = sp::row_kind(P.rows[k]);
      if (kind == sp::OUT_MUL) konst[k] = F::pack(F::canonical(F::inv(F::load(c.sel[sp::Q_O * c.n + P.rows[k].row]))));
      if (kind == sp::ROOT5)
        konst[k] = F::pack(F::canonical(F::inv(F::load(c.sel[(sp::Q_HASH + sp::row_wire(P.rows[k])) * c.n + P.rows[k].row]))));
    }
    return true;
  }
  // item k of the plan for the witness whose variables are `vars`, by the functions the kernels call (solve_kernels.hpp: an
  // INV0 item is row_value's kind 3 - hint_inv0 here -, ISZERO and BITS are solve_hint_item); returns whether a denominator
  // vanished
  bool item(size_t k, fe* vars) const {
    const sp::Row r = P.rows[k];
    const uint32_t kind = sp::row_kind(r), wire = sp::row_wire(r);
    if (kind >= sp::kFirstHintKind) {
      const sp::Hint h = P.hints[r.row];
      const fe src = vars[h.src];
      const uint32_t* tg = P.targets.data() + h.first;
      if (kind == sp::INV0) {
        vars[tg[0]] = S::hint_inv0(src, ex);
      } else if (kind == sp::ISZERO) {
        vars[tg[0]] = S::hint_iszero(src);
      } else {
        const uint32_t word = S::hint_bits_word(src, wire), base = wire * 32;
        const uint32_t nb = h.count - base < 32 ? h.count - base : 32;
        CHECK(base < h.count);
        for (uint32_t b = 0; b < nb; b++) vars[tg[base + b]] = S::bit_image((word >> b) & 1);
      }
      return false;
    }
    const size_t j = r.row;
    fl w[5];
    for (int i = 0; i < 5; i++) w[i] = F::from_ext(vars[c.wv[i * c.n + j]]);
    bool zd;
    const fl val = S::row_value([&](int s) { return F::load(c.sel[s * c.n + j]); }, kind, wire, w, F::load(konst[k]), ex, &zd);
    vars[c.wv[wire * c.n + j]] = F::to_ext(val);
    return zd;
  }
  void scatter(const fe* given, fe* vars) const {
    for (size_t v = 0; v < c.num_vars; v++) vars[v] = P.slot[v] >= 0 ? given[P.slot[v]] : plain_zero();
  }
  unsigned long long alone(const fe* given, fe* vars) const {
    scatter(given, vars);
    unsigned long long first = ~0ull;
    for (size_t k = 0; k < P.rows.size(); k++)
      if (item(k, vars) && P.rows[k].row < first) first = P.rows[k].row;
    return first;
  }
  // workgroup `block` of a launch at W over witnesses 0 .. count - 1, as k_solve_vars_packed<W> walks it: every lane runs its
  // stride over a level's items to the end before the next lane starts
  void packed_block(uint32_t W, uint32_t block, uint32_t count, const fe* given, fe* vars, unsigned long long* status) const {
    for (uint32_t s = 0; s < W; s++) {
      const uint32_t e = spk::slot_entry(block, s, W);
      if (e >= count) break;
      scatter(given + (size_t)e * P.num_given, vars + (size_t)e * c.num_vars);
    }
    for (size_t l = 0; l < P.levels; l++) {
      const uint32_t begin = P.level_off[l], items = spk::level_items(P.level_off[l + 1] - begin, W);
      for (uint32_t lane = 0; lane < kThreads; lane++)
        for (uint32_t i = lane; i < items; i += kThreads) {
          const spk::Item it = spk::item_decode(begin, i, W);
          CHECK(it.slot < W && it.k >= begin && it.k < P.level_off[l + 1]);
          const uint32_t e = spk::slot_entry(block, it.slot, W);
          if (e >= count) continue;
          if (item(it.k, vars + (size_t)e * c.num_vars) && P.rows[it.k].row < status[e]) status[e] = P.rows[it.k].row;
        }
    }
  }
};

// ---- hand-made: firing, levels, order ---------------------------------------------------------------------------------------
// n = 16; given = {0 (zero), 1 (one), 2, 3}; row 1 defines 4 from 2 and 3, row 2 defines 5 from 4, row 3 defines 10 from 6.
// Variables 20 .. 52 occur in no cell.
static Circuit hand_made() {
  Circuit c(16, 0, 60);
  const fe one = ext_of(1);
  c.wires(1, 2, 3, 0, 0, 4);
  c.set(sp::Q_O, 1, one);
  c.set(sp::Q_MUL, 1, one);
  c.wires(2, 4, 3, 0, 0, 5);
  c.set(sp::Q_O, 2, one);
  c.set(sp::Q_LC, 2, one);
  c.wires(3, 6, 7, 0, 0, 10);
  c.set(sp::Q_O, 3, one);
  c.set(sp::Q_LC, 3, one);
  c.set(sp::Q_LC + 1, 3, one);
  return c;
}
static const std::vector<uint32_t> kGiven = {0, 1, 2, 3};

static void check_firing() {
  Circuit c = hand_made();
  std::vector<uint32_t> wide;
  for (uint32_t v = 20; v < 53; v++) wide.push_back(v);
  c.hint(sp::HINT_BITS, 5, {6, 7});     // hint 0: its source is defined by row 2 (level 2): level 3
  c.hint(sp::HINT_INV0, 2, {8});        // hint 1: off a given value: level 1, fired before row 0
  c.hint(sp::HINT_BITS, 9, wide);       // hint 2: off hint 3's target - a chain that fires a LOWER index later: level 3
  c.hint(sp::HINT_ISZERO, 8, {9});      // hint 3: off hint 1's target: level 2
  sp::Plan P;
  CHECK(c.plan(kGiven, &P));
  if (!P.error.empty()) printf("plan refused: %s\n", P.error.c_str());
  CHECK(P.num_given == 4 && P.num_defined == 3 && P.levels == 4 && P.widest_level == 3 && P.inv_rows == 0 && P.root_rows == 0);
  CHECK(P.hints.size() == 4 && P.num_hinted == 37 && P.bits_hints == 2 && P.inv_hints == 1 && P.iszero_hints == 1);
  CHECK(P.hint_items == 5);
  const uint32_t off[5] = {0, 2, 4, 7, 8};
  CHECK(P.level_off.size() == 5 && !memcmp(P.level_off.data(), off, sizeof off));
  const sp::Row want[8] = {{1, sp::OUT_MUL | 4u << 8}, {1, sp::INV0},   {2, sp::OUT_MUL | 4u << 8}, {3, sp::ISZERO},
                           {0, sp::BITS},              {2, sp::BITS}, {2, sp::BITS | 1u << 8},    {3, sp::OUT_MUL | 4u << 8}};
  CHECK(P.rows.size() == 8);
  if (P.rows.size() == 8)
    for (int k = 0; k < 8; k++) CHECK(P.rows[k].row == want[k].row && P.rows[k].kw == want[k].kw);
  // a hinted variable on an input wire of a row that another hint completes: row 3 waits for hint 0 only
  // the same list without the chain's head: hint 2 and 3 never fire
  Circuit d = hand_made();
  d.hint(sp::HINT_BITS, 5, {6, 7});
  d.hint(sp::HINT_ISZERO, 8, {9});
  CHECK(!d.plan(kGiven, &P) && P.error.find("hint 1: its source variable 8 never gets a value") != std::string::npos);
}

static int refusals = 0;
static void refused(const Circuit& c, const std::vector<uint32_t>& given, const char* a, const char* b = nullptr) {
  sp::Plan P;
  const bool ok = c.plan(given, &P);
  CHECK(!ok && !P.error.empty());
  if (P.error.find(a) == std::string::npos || (b && P.error.find(b) == std::string::npos)) {
    bad++;
    printf("FAILED refusal: \"%s\" lacks \"%s\" / \"%s\"\n", P.error.c_str(), a, b ? b : "");
  }
  refusals++;
}

static void check_refusals() {
  auto base = [] {  // hint 0 stands; the broken one is hint 1
    Circuit c = hand_made();
    c.hint(sp::HINT_BITS, 5, {6, 7});
    return c;
  };
  {
    Circuit c = base();
    c.hints.push_back(sp::Hint{3, 2, 2, 1});
    c.targets.push_back(8);
    refused(c, kGiven, "hint 1: unknown kind 3", "variable 2");
  }
  {
    Circuit c = base();
    c.hint(sp::HINT_INV0, 60, {8});
    refused(c, kGiven, "hint 1: its source variable 60", "num_vars 60");
  }
  {
    Circuit c = base();
    c.hint(sp::HINT_INV0, 2, {61});
    refused(c, kGiven, "hint 1: its target 0, variable 61", "num_vars 60");
  }
  for (uint32_t kind : {sp::HINT_INV0, sp::HINT_ISZERO}) {
    Circuit c = base();
    c.hint(kind, 2, {8, 9});
    refused(c, kGiven, "hint 1: count 2 is out of range", "variable 2");
  }
  {
    Circuit c = base();
    c.hints.push_back(sp::Hint{sp::HINT_BITS, 2, 2, 0});
    refused(c, kGiven, "hint 1: count 0 is out of range", "variable 2");
    c.hints.back().count = 255;
    c.targets.resize(2 + 255, 8);
    refused(c, kGiven, "hint 1: count 255 is out of range", "variable 2");
  }
  {
    Circuit c = base();
    c.hints.push_back(sp::Hint{sp::HINT_BITS, 2, 2, 3});
    c.targets.push_back(8);
    c.targets.push_back(9);
    refused(c, kGiven, "hint 1: first + count = 5, num_targets is 4", "variable 2");
    c.hints.back() = sp::Hint{sp::HINT_INV0, 2, 0xffffffffu, 1};  // no wrap-around in first + count
    refused(c, kGiven, "hint 1: first + count = 4294967296", "variable 2");
  }
  {
    Circuit c = base();
    c.hint(sp::HINT_BITS, 2, {8, 9, 8});
    refused(c, kGiven, "hint 1: its target variable 8 is listed twice", "hint 1 has it too");
  }
  {
    Circuit c = base();
    c.hint(sp::HINT_INV0, 2, {7});
    refused(c, kGiven, "hint 1: its target variable 7 is listed twice", "hint 0 has it too");
  }
  {
    Circuit c = base();
    c.hint(sp::HINT_BITS, 2, {8, 2});
    refused(c, kGiven, "hint 1: its target 1 is its own source variable 2");
  }
  {
    Circuit c = base();
    c.hint(sp::HINT_ISZERO, 2, {3});
    refused(c, kGiven, "hint 1: its target variable 3 is given", "given_vars[3]");
  }
  {  // row 1 has defined variable 4 by the time its source (row 2's output) is there
    Circuit c = base();
    c.hint(sp::HINT_INV0, 5, {4});
    refused(c, kGiven, "hint 1: its target variable 4 already has a value", "row 1 defines it");
  }
  {
    Circuit c = base();
    c.hint(sp::HINT_INV0, 11, {8});
    refused(c, kGiven, "hint 1: its source variable 11 never gets a value");
  }
  {  // the row refusals are what they were, and come first: without hint 0 row 3 holds two variables without a value
    Circuit c = hand_made();
    c.hint(sp::HINT_INV0, 10, {8});
    refused(c, kGiven, "row 3 holds two variables without a value", "6 and 7");
    Circuit e = base();
    refused(e, {0, 1, 2, 3, 3}, "variable 3 is given twice");
  }
}

// ---- random circuits ----------------------------------------------------------------------------------------------------
struct Gen {
  Circuit c;
  std::vector<uint32_t> given, pool, small;  // small: given variables below 2^16
  uint32_t next;
  size_t j = 0;
  Gen(size_t n, size_t nv) : c(n, 0, nv), next(0) {
    for (uint32_t v = 0; v < 26; v++) given.push_back(v);
    next = 26;
    pool = given;
    for (uint32_t v = 2; v < 10; v++) small.push_back(v);
  }
  uint32_t pick() { return (rnd() & 3) ? pool[pool.size() - 1 - rnd() % (pool.size() < 12 ? pool.size() : 12)] : pool[rnd() % pool.size()]; }
  // a plain defining row of one of the three kinds (0 .. 2), as tests/cpp/solve_plan_check.cpp lays them
  uint32_t plain_row(uint32_t kind) {
    uint32_t w[5] = {pick(), pick(), pick(), pick(), 0};
    const uint32_t u = next++;
    for (int s = 0; s < (kind == 1 ? 13 : 12); s++) c.set(s, j, rnd_ext());
    if (kind == 2) {
      const uint32_t wire = (uint32_t)(rnd() % 4);
      c.set(sp::Q_LC + wire, j, ext_of(0));
      c.set(sp::Q_MUL + wire / 2, j, ext_of(0));
      w[4] = pick();
      w[wire] = u;
    } else {
      w[4] = u;
    }
    c.wires(j++, w[0], w[1], w[2], w[3], w[4]);
    pool.push_back(u);
    return u;
  }
  // out = a + sign b
  uint32_t lin(uint32_t a, uint32_t b, bool minus) {
    const uint32_t u = next++;
    c.set(sp::Q_LC, j, ext_of(1));
    c.set(sp::Q_LC + 1, j, minus ? ext_neg(ext_of(1)) : ext_of(1));
    c.set(sp::Q_O, j, ext_of(1));
    c.wires(j++, a, b, 0, 0, u);
    return u;
  }
  // unpack(v, nbits): the hint, a boolean row per bit (the bit on wires 0, 1 and 4), and the recomposition chain, three
  // bits a row, whose last row outputs v itself
  std::vector<uint32_t> unpack(uint32_t v, uint32_t nbits) {
    std::vector<uint32_t> bits;
    for (uint32_t i = 0; i < nbits; i++) bits.push_back(next++);
    c.hint(sp::HINT_BITS, v, bits);
    for (uint32_t b : bits) {
      c.set(sp::Q_MUL, j, ext_of(1));
      c.set(sp::Q_O, j, ext_of(1));
      c.wires(j++, b, b, 0, 0, b);
    }
    uint32_t acc = 0;
    for (uint32_t i = 0; i < nbits; i += 3) {
      uint32_t w[3] = {0, 0, 0};
      for (uint32_t t = 0; t < 3 && i + t < nbits; t++) {
        w[t] = bits[i + t];
        c.set(sp::Q_LC + t, j, ext_pow2(i + t));
      }
      c.set(sp::Q_LC + 3, j, ext_of(1));
      c.set(sp::Q_O, j, ext_of(1));
      const uint32_t out = i + 3 >= nbits ? v : next++;
      c.wires(j++, w[0], w[1], w[2], acc, out);
      acc = out;
    }
    return bits;
  }
  // is_zero(a): y = 1 - a a_inv and a y = 0 over (a, a_inv, y); both hinted
  uint32_t is_zero(uint32_t a, uint32_t* inv_out = nullptr) {
    const uint32_t inv = next++, y = next++;
    c.hint(sp::HINT_INV0, a, {inv});
    c.hint(sp::HINT_ISZERO, a, {y});
    c.set(sp::Q_MUL, j, ext_of(1));
    c.set(sp::Q_C, j, ext_neg(ext_of(1)));
    c.set(sp::Q_O, j, ext_neg(ext_of(1)));
    c.wires(j++, a, inv, 0, 0, y);
    c.set(sp::Q_MUL, j, ext_of(1));
    c.set(sp::Q_O, j, ext_of(1));
    c.wires(j++, a, y, 0, 0, 0);
    if (inv_out) *inv_out = inv;
    return y;
  }
};

static int plans_equal = 0, bits_checked = 0, invs_checked = 0, flags_checked = 0, gates_checked = 0, packed_cases = 0;
static int zero_sources = 0;

static void check_unhinted(size_t n) {
  Gen g(n, 26 + n);
  while (g.j < n - n / 8) g.plain_row((uint32_t)(rnd() % 3));
  sp::Plan P, Q;
  CHECK(g.c.plan(g.given, &P));
  CHECK(sp::solve_plan(n, 0, g.c.num_vars, g.c.wv.data(), g.c.zero.data(), g.given.data(), g.given.size(), &Q));
  const Before B = plan_before(g.c, g.given);
  CHECK(B.ok && B.rows.size() == P.rows.size() && B.level_off == P.level_off && P.level_off == Q.level_off);
  CHECK(B.rows.size() == Q.rows.size() && !memcmp(B.rows.data(), P.rows.data(), sizeof(sp::Row) * B.rows.size()) &&
        !memcmp(B.rows.data(), Q.rows.data(), sizeof(sp::Row) * B.rows.size()));
  CHECK(P.num_defined == B.rows.size() && P.inv_rows == B.inv_rows && P.root_rows == B.root_rows && P.widest_level == B.widest);
  CHECK(P.levels >= 2 && P.root_rows > 0 && P.inv_rows > 0);
  CHECK(P.hints.empty() && P.targets.empty() && P.hint_items == 0 && P.num_hinted == 0);
  plans_equal++;
}

static void check_hinted(size_t n, uint32_t witnesses) {
  Gen g(n, 4 * n);
  Circuit& c = g.c;
  std::vector<uint32_t> diffs;
  for (int t = 0; t < 6; t++) g.plain_row((uint32_t)(rnd() % 3));
  // decompositions of given and of computed small values, widths that are and are not a multiple of 3 and of 32
  g.unpack(g.small[0], 16);
  const uint32_t s1 = g.lin(g.small[1], g.small[2], false);
  g.unpack(s1, 17);
  g.unpack(g.lin(s1, g.small[3], false), 33);
  g.unpack(g.small[4], 64);
  for (int t = 0; t < 5; t++) g.plain_row((uint32_t)(rnd() % 3));
  // a full-width decomposition of a computed value, and of the inverse of one (INV0 -> BITS)
  g.unpack(g.pool.back(), 254);
  uint32_t inv;
  g.is_zero(g.pool[g.pool.size() - 2], &inv);
  g.unpack(inv, 254);
  // is_equal on both sides of the test: a difference that is zero for every witness, one that is not, one that is zero
  // for witness 1 alone (given 10 and 11 are made equal there)
  diffs.push_back(g.lin(g.small[5], g.small[5], true));
  diffs.push_back(g.lin(g.pool[30], g.small[6], true));
  diffs.push_back(g.lin(10, 11, true));
  for (uint32_t d : diffs) {
    const uint32_t y = g.is_zero(d);
    g.unpack(y, 1);  // a flag's own bit: ISZERO -> BITS
    g.pool.push_back(y);
  }
  g.is_zero(12);  // off a given value: level 1
  for (int t = 0; t < 8; t++) g.plain_row((uint32_t)(rnd() % 3));
  CHECK(g.j <= n && g.next <= c.num_vars);
  Solver sv(c);
  const bool ok = sv.plan(g.given);
  CHECK(ok);
  if (!ok) {
    printf("plan refused: %s\n", sv.P.error.c_str());
    return;
  }
  const sp::Plan& P = sv.P;
  CHECK(P.hints.size() == c.hints.size() && P.num_hinted == c.targets.size() && P.inv_hints == 5 && P.iszero_hints == 5);
  uint64_t items = 0;
  for (const sp::Hint& h : c.hints) items += (h.count + 31) / 32;
  CHECK(P.hint_items == items && P.rows.size() == P.num_defined + items);
  for (size_t l = 0; l + 1 < P.level_off.size(); l++) {
    CHECK(P.level_off[l] < P.level_off[l + 1]);
    for (uint32_t k = P.level_off[l] + 1; k < P.level_off[l + 1]; k++) {  // (kind, row or hint, chunk) ascending
      const sp::Row &a = P.rows[k - 1], &b = P.rows[k];
      const uint32_t ka = sp::row_kind(a), kb = sp::row_kind(b);
      CHECK(ka < kb || (ka == kb && (a.row < b.row || (a.row == b.row && ka == sp::BITS && sp::row_wire(a) < sp::row_wire(b)))));
    }
  }
  const size_t ng = P.num_given, nv = c.num_vars;
  std::vector<fe> given((size_t)witnesses * ng);
  for (uint32_t p = 0; p < witnesses; p++) {
    fe* gv = &given[p * ng];
    for (size_t k = 0; k < ng; k++) gv[k] = rnd_ext();
    gv[0] = ext_of(0);
    gv[1] = ext_of(1);
    for (uint32_t v = 2; v < 10; v++) gv[v] = ext_of((uint32_t)(rnd() & 0xffff));
    if (p == 1) gv[11] = gv[10];
    if (p == 2) gv[12] = ext_of(0);
  }
  std::vector<std::vector<fe>> alone(witnesses, std::vector<fe>(nv));
  for (uint32_t p = 0; p < witnesses; p++) {
    fe* vars = alone[p].data();
    CHECK(sv.alone(&given[p * ng], vars) == ~0ull);
    for (const sp::Hint& h : c.hints) {
      const fe plain = F::from_mont(F::from_ext(vars[h.src]));
      bool src_zero = true;
      for (int i = 0; i < 8; i++) src_zero &= plain.v[i] == 0;
      const uint32_t* tg = &c.targets[h.first];
      if (h.kind == sp::HINT_BITS) {
        for (uint32_t i = 0; i < h.count; i++) {
          CHECK(same_words(vars[tg[i]], ext_of((plain.v[i / 32] >> (i % 32)) & 1)));
          bits_checked++;
        }
      } else if (h.kind == sp::HINT_INV0) {
        const fl prod = F::mul(F::from_ext(vars[tg[0]]), F::from_ext(vars[h.src]));
        CHECK(src_zero ? same_words(vars[tg[0]], ext_of(0)) : F::eq(prod, F::one()));
        invs_checked++;
      } else {
        CHECK(same_words(vars[tg[0]], ext_of(src_zero ? 1 : 0)));
        flags_checked++;
        zero_sources += src_zero;
      }
    }
    for (size_t j = 0; j < n; j++) {  // every row, the constraints the solver never evaluates included
      fl w[5];
      for (int i = 0; i < 5; i++) w[i] = F::from_ext(vars[c.wv[i * n + j]]);
      CHECK(C::gate_holds([&](int s) { return F::load(c.sel[s * n + j]); }, w, F::zero()));
      gates_checked++;
    }
  }
  CHECK(same_words(alone[1][c.targets[c.hints[c.hints.size() - 4].first]], ext_of(1)));  // is_equal(10, 11) in witness 1
  for (uint32_t W : {1u, 4u, 16u})
    for (uint32_t count : {1u, W - 1, W + 1, 2 * W + 3}) {
      if (!count || count > witnesses) continue;
      std::vector<fe> vars((size_t)count * nv);
      std::vector<unsigned long long> st(count, ~0ull);
      for (uint32_t b = 0; b < spk::blocks_for(count, W); b++) sv.packed_block(W, b, count, given.data(), vars.data(), st.data());
      for (uint32_t p = 0; p < count; p++) {
        CHECK(st[p] == ~0ull);
        CHECK(!memcmp(&vars[(size_t)p * nv], alone[p].data(), sizeof(fe) * nv));
      }
      packed_cases++;
    }
}

static void check_rules(const sv29::Exps& ex) {
  // the field's edge values through the three rules: 0, 1, r - 1, 2^253, and a non-canonical image of 0 (r itself)
  fe rm1 = F::pack(F::konst(FrP29::MOD));
  rm1.v[0] -= 1;
  const fe r_image = F::pack(F::konst(FrP29::MOD));  // the words of r: an image of the value 0 * 2^256
  const fe srcs[5] = {ext_of(0), ext_of(1), ext_of_plain(rm1), ext_pow2(253), r_image};
  const bool zero[5] = {true, false, false, false, true};
  for (int t = 0; t < 5; t++) {
    CHECK(same_words(S::hint_iszero(srcs[t]), ext_of(zero[t] ? 1 : 0)));
    const fe inv = S::hint_inv0(srcs[t], ex);
    CHECK(zero[t] ? same_words(inv, ext_of(0)) : F::eq(F::mul(F::from_ext(inv), F::from_ext(srcs[t])), F::one()));
    const fe plain = F::from_mont(F::from_ext(srcs[t]));
    for (uint32_t g = 0; g < 8; g++) CHECK(S::hint_bits_word(srcs[t], g) == plain.v[g]);
  }
  CHECK(S::hint_bits_word(ext_pow2(253), 7) == 1u << 29 && S::hint_bits_word(ext_of_plain(rm1), 0) == 0xf0000000u);
  CHECK(same_words(S::bit_image(1), ext_of(1)) && same_words(S::bit_image(0), plain_zero()));
}

int main() {
  sv29::Exps ex;
  CHECK(sv29::derive_exps(&ex));
  check_rules(ex);
  check_firing();
  check_refusals();
  check_unhinted(64);
  check_unhinted(256);
  check_unhinted(512);
  check_hinted(2048, 35);
  check_hinted(2048, 3);
  printf("bad=%d refusals=%d plans=%d bits=%d invs=%d flags=%d zero_sources=%d gates=%d packed=%d\n", bad, refusals, plans_equal,
         bits_checked, invs_checked, flags_checked, zero_sources, gates_checked, packed_cases);
  return bad ? 1 : 0;
}
