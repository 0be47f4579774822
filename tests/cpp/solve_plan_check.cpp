// Host-side check of the witness solver: cap_amd/csrc/solve_plan.hpp (the plan: refusals, levels, order) and
// cap_amd/csrc/solve29.hpp (the row rule) with field29.hpp's bound assertions on.  Stand-alone; prints one summary line
// that tests/test_solve_plan_host.py reads, "bad=0" when every check held.
//   - the two exponents are derived and do what they are for: a^(r-2) a = 1, (y^5)^e = y, 0 -> 0
//   - every refusal of the rule is met and names the LOWEST offending row
//   - levels, offsets and the (level, kind, row) order on a hand-made circuit
//   - random circuits holding OUT rows with and without q_ecc and ROOT5 rows on each of wires 0 .. 3: after a solve in plan
//     order wc29::Check::gate is zero at every defining row, and y^5 equals the right-hand side at every ROOT5 row
//   - a zero denominator gives the value 0 and is flagged; the smallest flagged row is the lowest one
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/solve29.hpp"
#include "../../cap_amd/csrc/solve_plan.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace cap;
using C = wc29::Check<CAP_FL_SCHED>;
using S = sv29::Solve<CAP_FL_SCHED>;
using F = S::F;

static int bad = 0;
#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      bad++;                                                  \
      printf("FAILED line %d: %s\n", __LINE__, #x);           \
    }                                                         \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// a random field element in the memory form of a witness value (arkworks Montgomery words, canonical)
static fe rnd_ext() {
  fe a;
  for (int i = 0; i < 8; i++) a.v[i] = (uint32_t)rnd();
  a.v[7] &= 0x0fffffffu;  // below 2^252 < r
  return F::to_ext(F::to_mont(a));
}
static fe ext_of(uint32_t x) {
  fe a;
  memset(&a, 0, sizeof a);
  a.v[0] = x;
  return F::to_ext(F::to_mont(a));
}
// a selector as the device holds it: internal form, canonical, packed
static fe sel_of(const fe& ext) { return F::pack(F::canonical(F::from_ext(ext))); }
static bool same(const fl& a, const fl& b) { return F::eq(a, b); }

struct Circuit {
  size_t n, num_inputs, num_vars;
  std::vector<uint32_t> wv;  // [5][n]
  std::vector<fe> sel;       // [13][n], device form
  std::vector<uint8_t> zero;
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
  bool plan(const std::vector<uint32_t>& given, sp::Plan* P) const {
    return sp::solve_plan(n, num_inputs, num_vars, wv.data(), zero.data(), given.data(), given.size(), P);
  }
};

// the solve as the kernel runs it, one row after the other in plan order; returns the smallest row with a zero denominator
static std::vector<size_t> flagged;  // every such row of the last solve
static unsigned long long solve(const Circuit& c, const sp::Plan& P, const std::vector<fe>& given, std::vector<fe>* vars,
                                const sv29::Exps& ex) {
  std::vector<fe> konst(P.rows.size());
  for (size_t k = 0; k < P.rows.size(); k++) {
    const uint32_t kind = sp::row_kind(P.rows[k]);
    fl x = F::one();
    if (kind == sp::OUT_MUL) x = F::load(c.sel[sp::Q_O * c.n + P.rows[k].row]);
    if (kind == sp::ROOT5) x = F::load(c.sel[(sp::Q_HASH + sp::row_wire(P.rows[k])) * c.n + P.rows[k].row]);
    konst[k] = F::pack(F::canonical(F::inv(x)));
  }
  vars->assign(c.num_vars, ext_of(0));
  for (size_t v = 0; v < c.num_vars; v++)
    if (P.slot[v] >= 0) (*vars)[v] = given[P.slot[v]];
  unsigned long long first = ~0ull;
  flagged.clear();
  for (size_t k = 0; k < P.rows.size(); k++) {
    const size_t j = P.rows[k].row;
    const uint32_t kind = sp::row_kind(P.rows[k]), wire = sp::row_wire(P.rows[k]);
    fl w[5];
    for (int i = 0; i < 5; i++) w[i] = F::from_ext((*vars)[c.wv[i * c.n + j]]);
    bool zd;
    const fl val = S::row_value([&](int s) { return F::load(c.sel[s * c.n + j]); }, kind, wire, w, F::load(konst[k]), ex, &zd);
    if (zd && j < first) first = j;
    if (zd) flagged.push_back(j);
    (*vars)[c.wv[wire * c.n + j]] = F::to_ext(val);
  }
  return first;
}

static void check_exponents(const sv29::Exps& ex) {
  for (int t = 0; t < 8; t++) {
    const fl a = F::from_ext(rnd_ext());
    CHECK(same(F::mul(S::pow_fixed(a, ex.inv), a), F::one()));
    const fl a5 = F::mul(F::sqr(F::sqr(a)), a);
    CHECK(same(S::pow_fixed(a5, ex.root5), a));
    const fl y = S::pow_fixed(a, ex.root5);
    CHECK(same(F::mul(F::sqr(F::sqr(y)), y), a));
  }
  CHECK(F::is_zero(S::pow_fixed(F::zero(), ex.inv)));
  CHECK(F::is_zero(S::pow_fixed(F::zero(), ex.root5)));
  // a lazy representation of zero (r itself) is zero too
  CHECK(F::is_zero(S::pow_fixed(F::konst(FrP29::MOD), ex.inv)));
}

// n = 16, variables 0 .. 9; given = {0, 1, 2, 3}; row 0 is the public input (variable 2 on wire 4)
static Circuit hand_made() {
  Circuit c(16, 1, 10);
  const fe one = ext_of(1);
  c.wires(0, 0, 0, 0, 0, 2);
  c.set(sp::Q_O, 0, one);
  c.wires(1, 2, 3, 0, 0, 4);  // OUT, level 1
  c.set(sp::Q_O, 1, one);
  c.set(sp::Q_MUL, 1, one);
  c.wires(2, 4, 3, 0, 0, 5);  // OUT, level 2
  c.set(sp::Q_O, 2, ext_of(7));
  c.set(sp::Q_LC, 2, one);
  c.set(sp::Q_LC + 1, 2, one);
  c.wires(3, 2, 2, 1, 1, 6);  // OUT with q_ecc, level 1
  c.set(sp::Q_ECC, 3, ext_of(3));
  c.set(sp::Q_C, 3, ext_of(5));
  c.wires(4, 7, 1, 0, 0, 5);  // ROOT5 on wire 0, its wire-4 variable from level 2: level 3
  c.set(sp::Q_HASH, 4, ext_of(9));
  c.set(sp::Q_O, 4, one);
  c.set(sp::Q_LC + 1, 4, ext_of(2));
  c.wires(5, 4, 5, 6, 7, 2);  // a constraint: everything valued by now (not evaluated)
  c.set(sp::Q_O, 5, one);
  return c;
}

static void check_levels() {
  const Circuit c = hand_made();
  sp::Plan P;
  CHECK(c.plan({0, 1, 2, 3}, &P));
  CHECK(P.error.empty() && P.num_given == 4 && P.num_defined == 4 && P.levels == 3 && P.widest_level == 2);
  CHECK(P.inv_rows == 1 && P.root_rows == 1);
  const uint32_t off[4] = {0, 2, 3, 4};
  CHECK(P.level_off.size() == 4 && !memcmp(P.level_off.data(), off, sizeof off));
  CHECK(P.rows.size() == 4);
  if (P.rows.size() == 4) {
    CHECK(P.rows[0].row == 1 && P.rows[0].kw == (sp::OUT_MUL | 4u << 8));
    CHECK(P.rows[1].row == 3 && P.rows[1].kw == (sp::OUT_INV | 4u << 8));
    CHECK(P.rows[2].row == 2 && P.rows[2].kw == (sp::OUT_MUL | 4u << 8));
    CHECK(P.rows[3].row == 4 && P.rows[3].kw == (sp::ROOT5 | 0u << 8));
  }
  CHECK(P.slot[0] == 0 && P.slot[3] == 3 && P.slot[4] == -1 && P.slot[9] == -1);
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
  const std::vector<uint32_t> g = {0, 1, 2, 3};
  const fe one = ext_of(1);
  refused(hand_made(), {0, 1, 2, 3, 1}, "variable 1 is given twice", "given_vars[1] and given_vars[4]");
  refused(hand_made(), {0, 1, 2, 10}, "given_vars[3] = 10", "num_vars is 10");
  refused(hand_made(), {0, 1, 3}, "row 0 is a public-input row", "variable 2 is not given");
  {  // two unknowns at row 6, and again at row 8: the lower one is named
    Circuit c = hand_made();
    c.wires(6, 8, 0, 0, 0, 9);
    c.set(sp::Q_O, 6, one);
    c.wires(8, 8, 9, 0, 0, 1);
    refused(c, g, "row 6 holds two variables without a value", "8 and 9");
  }
  {  // an unknown on wire 4 with neither q_o nor q_ecc
    Circuit c = hand_made();
    c.wires(6, 2, 3, 0, 0, 8);
    c.set(sp::Q_LC, 6, one);
    refused(c, g, "row 6 cannot define its variable 8");
  }
  {  // the unknown on wire 4 AND on an input wire
    Circuit c = hand_made();
    c.wires(6, 2, 8, 0, 0, 8);
    c.set(sp::Q_O, 6, one);
    refused(c, g, "row 6 cannot define its variable 8");
  }
  {  // the unknown on two input wires
    Circuit c = hand_made();
    c.wires(6, 8, 8, 0, 0, 2);
    c.set(sp::Q_HASH, 6, one);
    c.set(sp::Q_O, 6, one);
    refused(c, g, "row 6 cannot define its variable 8");
  }
  for (int why = 0; why < 4; why++)
    for (uint32_t wire = 0; wire < 4; wire++) {  // the fifth-root shape with one of its conditions broken, on each wire
      Circuit c = hand_made();
      uint32_t w[5] = {2, 3, 2, 3, 4};
      w[wire] = 8;
      c.wires(7, w[0], w[1], w[2], w[3], w[4]);
      c.set(sp::Q_O, 7, one);
      if (why != 0) c.set(sp::Q_HASH + wire, 7, ext_of(4));
      if (why == 1) c.set(sp::Q_LC + wire, 7, one);
      if (why == 2) c.set(sp::Q_MUL + wire / 2, 7, one);
      if (why == 3) c.set(sp::Q_ECC, 7, one);
      // a later row that would be refused too: row 7 is the one named
      c.wires(9, 9, 9, 0, 0, 0);
      refused(c, g, "row 7 cannot define its variable 8");
      if (why == 0) {  // ... and with every condition met the row is taken, on this wire
        c.set(sp::Q_HASH + wire, 7, ext_of(4));
        c.wires(9, 0, 0, 0, 0, 0);
        sp::Plan P;
        CHECK(c.plan(g, &P) && P.root_rows == 2);
        bool found = false;
        for (const sp::Row& r : P.rows) found |= r.row == 7 && r.kw == (sp::ROOT5 | wire << 8);
        CHECK(found);
      }
    }
}

// A random circuit: every row from num_inputs on defines a fresh variable by one of the three rules, from variables
// that hold a value by then (given ones or outputs of earlier rows), so dependency chains of every depth occur.
static int gates_checked = 0, roots_checked = 0, zero_dens = 0;
static void check_random(size_t n, size_t num_inputs, const sv29::Exps& ex, bool degenerate) {
  const size_t num_given = 2 + num_inputs + 24;
  Circuit c(n, num_inputs, num_given + n);
  std::vector<uint32_t> given;
  for (uint32_t v = 0; v < num_given; v++) given.push_back(v);
  uint32_t next = (uint32_t)num_given;
  std::vector<uint32_t> pool(given);
  auto pick = [&] { return (rnd() & 3) ? pool[pool.size() - 1 - rnd() % (pool.size() < 12 ? pool.size() : 12)] : pool[rnd() % pool.size()]; };
  for (size_t j = 0; j < num_inputs; j++) {
    c.wires(j, 0, 0, 0, 0, 2 + (uint32_t)j);
    c.set(sp::Q_O, j, ext_of(1));
  }
  std::vector<size_t> ecc_rows;
  const size_t gate_rows = n - n / 8;
  for (size_t j = num_inputs; j < gate_rows; j++) {
    uint32_t w[5] = {pick(), pick(), pick(), pick(), 0};
    const uint32_t kind = (uint32_t)(rnd() % 8), u = next++;
    if (kind < 3) {  // OUT without q_ecc: every other selector set
      for (int s = 0; s < 12; s++) c.set(s, j, rnd_ext());
      w[4] = u;
    } else if (kind < 5) {  // OUT with q_ecc (and q_o = 0 half the time, unless a wire holds the zero variable:
                            // the denominator would be 0 for every witness)
      for (int s = 0; s < 13; s++) c.set(s, j, rnd_ext());
      if ((rnd() & 1) && w[0] && w[1] && w[2] && w[3]) c.set(sp::Q_O, j, ext_of(0));
      w[4] = u;
      ecc_rows.push_back(j);
    } else if (kind < 7) {  // ROOT5 on a random wire, the known value on wire 4
      const uint32_t wire = (uint32_t)(rnd() % 4);
      for (int s = 0; s < 12; s++) c.set(s, j, rnd_ext());
      c.set(sp::Q_LC + wire, j, ext_of(0));
      c.set(sp::Q_MUL + wire / 2, j, ext_of(0));
      w[4] = pick();
      w[wire] = u;
    } else {  // a row that defines nothing (it does not hold: the solver never evaluates it)
      c.set(sp::Q_O, j, ext_of(1));
      w[4] = pick();
      next--;
      c.wires(j, w[0], w[1], w[2], w[3], w[4]);
      continue;
    }
    c.wires(j, w[0], w[1], w[2], w[3], w[4]);
    pool.push_back(u);
  }
  sp::Plan P;
  CHECK(c.plan(given, &P));
  if (!P.error.empty()) {
    printf("plan refused: %s\n", P.error.c_str());
    return;
  }
  CHECK(P.num_defined == next - num_given && P.levels >= 2 && P.root_rows > 0 && P.inv_rows == ecc_rows.size());
  for (size_t l = 0; l + 1 < P.level_off.size(); l++) CHECK(P.level_off[l] < P.level_off[l + 1]);
  std::vector<fe> gv(num_given);
  for (auto& x : gv) x = rnd_ext();
  gv[0] = ext_of(0);
  gv[1] = ext_of(1);
  std::vector<fe> vars;
  std::vector<size_t> forced;
  if (degenerate && ecc_rows.size() >= 3) {
    // make the denominator of two q_ecc rows vanish for THESE values: solve once, then set q_ecc = q_o / (w0 w1 w2 w3)
    // at the rows (the values below them do not depend on their own q_ecc)
    (void)solve(c, P, gv, &vars, ex);
    for (size_t t : {ecc_rows.size() - 1, ecc_rows.size() / 2}) {
      const size_t j = ecc_rows[t];
      fl prod = F::one();
      for (int i = 0; i < 4; i++) prod = F::mul(prod, F::from_ext(vars[c.wv[i * n + j]]));
      if (F::is_zero(prod)) continue;
      if (F::is_zero(F::load(c.sel[sp::Q_O * n + j]))) c.set(sp::Q_O, j, ext_of(11));
      const fl qe = F::mul(F::load(c.sel[sp::Q_O * n + j]), F::inv(prod));
      c.sel[sp::Q_ECC * n + j] = F::pack(F::canonical(qe));
      forced.push_back(j);
    }
  }
  const unsigned long long first = solve(c, P, gv, &vars, ex);
  if (forced.empty()) {
    CHECK(first == ~0ull);
  } else {
    size_t lowest = forced[0];
    for (size_t j : forced) lowest = j < lowest ? j : lowest;
    CHECK(first == lowest);
    // (a later forced row may read values changed by the first one and not vanish any more: the lowest always does)
    CHECK(F::is_zero(F::from_ext(vars[c.wv[4 * n + lowest]])));
    zero_dens++;
  }
  for (size_t k = 0; k < P.rows.size(); k++) {
    const size_t j = P.rows[k].row;
    // (a row whose denominator vanished holds 0 and does not satisfy its gate; the 0 of a forced row can make the
    // denominator of a later q_o = 0 row vanish in turn)
    bool is_forced = false;
    for (size_t f : forced) is_forced |= f == j;
    for (size_t f : flagged) is_forced |= f == j;
    if (is_forced) continue;
    fl w[5];
    for (int i = 0; i < 5; i++) w[i] = F::from_ext(vars[c.wv[i * n + j]]);
    auto q = [&](int s) { return F::load(c.sel[s * n + j]); };
    CHECK(C::gate_holds(q, w, F::zero()));
    gates_checked++;
    if (sp::row_kind(P.rows[k]) == sp::ROOT5) {
      const uint32_t wire = sp::row_wire(P.rows[k]);
      const fl y = w[wire];
      w[wire] = F::zero();
      fl unused;
      const fl rhs = F::mul(F::sub(F::mul(q(sp::Q_O), w[4]), S::rest(q, w, &unused)),
                            F::inv(q(sp::Q_HASH + (int)wire)));
      CHECK(same(F::mul(F::sqr(F::sqr(y)), y), rhs));
      roots_checked++;
    }
  }
  // variables in no cell and not given stay 0
  for (size_t v = next; v < c.num_vars; v++) CHECK(F::is_zero(F::from_ext(vars[v])));
}

int main() {
  sv29::Exps ex;
  CHECK(sv29::derive_exps(&ex));
  CHECK(ex.inv[0] == 0xefffffffu && (ex.root5[7] >> 30) == 0);
  check_exponents(ex);
  check_levels();
  check_refusals();
  check_random(64, 3, ex, false);
  check_random(256, 5, ex, false);
  check_random(256, 0, ex, true);
  check_random(512, 7, ex, true);
  printf("bad=%d refusals=%d gates=%d roots=%d zero_dens=%d\n", bad, refusals, gates_checked, roots_checked, zero_dens);
  return bad ? 1 : 0;
}
