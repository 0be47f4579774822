// Host-side check of the solver's DEFERRED form (capgpu_plonk_key_set_solve_form): the rule of cap_amd/csrc/solve_defer.hpp and
// the field code of cap_amd/csrc/solve_defer29.hpp, with field29.hpp's bound assertions on.  Stand-alone; prints one summary
// line that tests/test_solve_defer_host.py reads, "bad=0" when every check held.
//   - 300 random circuits (OUT rows with and without q_ecc in chains, doublings, hash cells, ROOT5, LIN, public rows that are
//     derived, BITS / ISZERO / INV0 hints), the four flag values in turn
//   - each is solved item by item through the direct plan and through the deferred schedule - FRAC rows by row_value_frac,
//     flush items by flush_group over an emulated side buffer, in the Fermat and the GCD form in turn - and compared limb for
//     limb: every variable's image and the lowest row with a zero denominator
//   - every deferred variable is resolved exactly once; nothing is pending where a plain value is read
//   - each pending-variable case is met (counted; the program fails otherwise): on a hash cell, as a hint's source, as a
//     ROOT5 / LIN input, on two cells of one row, behind a zero denominator
//   - deriving the deferred schedule leaves the direct plan's bytes as they were
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/solve_defer.hpp"
#include "../../cap_amd/csrc/solve_defer29.hpp"

#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>
using namespace cap;
using S = sv29::Solve<CAP_FL_SCHED>;
using F = S::F;

static int bad = 0;
#define CHECK(x)                                    \
  do {                                              \
    if (!(x)) {                                     \
      bad++;                                        \
      printf("FAILED line %d: %s\n", __LINE__, #x); \
    }                                               \
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
static fe rnd_ext() {  // random and non-zero
  fe a;
  for (int i = 0; i < 8; i++) a.v[i] = (uint32_t)rnd();
  a.v[7] &= 0x0fffffffu;  // below 2^252 < r
  a.v[0] |= 1;
  return ext_of_plain(a);
}
static fe ext_of(uint32_t x) {
  fe a = plain_zero();
  a.v[0] = x;
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
  void wires(size_t j, const uint32_t* w) {
    for (int i = 0; i < 5; i++) wv[i * n + j] = w[i];
  }
  fl q(int s, size_t j) const { return F::load(sel[s * n + j]); }
};

static fl inverse_const(const fl& x) { return F::load(F::pack(F::canonical(F::inv(x)))); }

// one item of the direct kinds for the assignment `vars`; returns true for a zero denominator
static bool direct_item(const Circuit& c, const sp::Plan& P, const sp::Row& r, const sv29::Exps& ex, std::vector<fe>& vars) {
  const uint32_t kind = sp::row_kind(r), wire = sp::row_wire(r);
  if (sp::is_hint_kind(kind)) {
    const sp::Hint& h = P.hints[r.row];
    if (kind == sp::BITS) {
      const uint32_t word = S::hint_bits_word(vars[h.src], wire), base = wire * 32;
      for (uint32_t b = 0; b < 32 && base + b < h.count; b++) vars[P.targets[h.first + base + b]] = S::bit_image((word >> b) & 1);
    } else if (kind == sp::ISZERO) {
      vars[P.targets[h.first]] = S::hint_iszero(vars[h.src]);
    } else {
      vars[P.targets[h.first]] = S::hint_inv0(vars[h.src], ex);
    }
    return false;
  }
  const size_t j = r.row;
  fl w[5];
  for (int i = 0; i < 5; i++) w[i] = F::from_ext(vars[c.wv[i * c.n + j]]);
  fl konst = F::zero();
  if (kind == sp::OUT_MUL) konst = inverse_const(c.q(sp::Q_O, j));
  if (kind == sp::ROOT5) konst = inverse_const(c.q(sp::Q_HASH + (int)wire, j));
  if (kind == sp::LIN) konst = inverse_const(c.q(sp::Q_LC + (int)wire, j));
  bool zd = false;
  const fl v = S::row_value<true, true>([&](int s) { return c.q(s, j); }, kind, wire, w, konst, ex, &zd);
  vars[c.wv[wire * c.n + j]] = F::to_ext(v);
  return zd;
}

static const uint64_t kSolved = ~0ull;
static void start(const sp::Plan& P, const std::vector<fe>& given_vals, std::vector<fe>* vars) {
  vars->assign(P.slot.size(), plain_zero());
  for (size_t v = 0; v < P.slot.size(); v++)
    if (P.slot[v] >= 0) (*vars)[v] = given_vals[(size_t)P.slot[v]];
}
static uint64_t walk_direct(const Circuit& c, const sp::Plan& P, const sv29::Exps& ex, const std::vector<fe>& given_vals,
                            std::vector<fe>* vars) {
  start(P, given_vals, vars);
  uint64_t status = kSolved;
  for (const sp::Row& r : P.rows)
    if (direct_item(c, P, r, ex, *vars)) status = std::min<uint64_t>(status, r.row);
  return status;
}

// the cases a pending variable is met in
static int on_hash_cell = 0, as_hint_source = 0, as_root_or_lin_input = 0, on_two_cells = 0, behind_zero_den = 0;
static int frac_rows = 0, flush_items = 0, zero_dens = 0;

template <int INV>
static uint64_t walk_deferred(const Circuit& c, const sp::Plan& P, const sd::Sched& D, const sv29::Exps& ex,
                              const std::vector<fe>& given_vals, std::vector<fe>* vars_out) {
  using Dv = sv29::Defer<CAP_FL_SCHED, INV>;
  std::vector<fe>& vars = *vars_out;
  start(P, given_vals, &vars);
  std::vector<fe> side(2 * D.slots + 1, plain_zero());
  std::vector<int> resolved(P.slot.size(), 0), defined(P.slot.size(), 0);
  std::set<uint32_t> pend, zeroed;
  uint64_t status = kSolved;
  const size_t n = c.n;
  CHECK(D.level_off.size() == D.levels + 1 && D.flush_level.size() == D.levels && D.rows.size() == D.src.size());
  for (size_t l = 0; l < D.levels; l++) {
    std::vector<uint32_t> joined;
    for (uint32_t k = D.level_off[l]; k < D.level_off[l + 1]; k++) {
      const sp::Row& r = D.rows[k];
      const uint32_t kind8 = r.kw & 0xffu;
      CHECK((kind8 == sd::FLUSH) == (D.flush_level[l] != 0));
      if (kind8 == sd::FLUSH) {
        const uint32_t count = r.kw >> 8;
        CHECK(count >= 1 && count <= sd::kGroup && (size_t)r.row + count <= D.flush_vars.size());
        const uint32_t* fv = D.flush_vars.data() + r.row;
        const int32_t first = D.dslot[fv[0]];
        CHECK(first >= 0 && (size_t)first + count <= D.slots);
        for (uint32_t i = 0; i < count; i++) CHECK(D.dslot[fv[i]] == first + (int32_t)i && pend.count(fv[i]));
        fe* den = side.data() + first;
        fe* pre = den + D.slots;
        Dv::flush_group(
            count, [&](uint32_t i) { return F::load(den[i]); }, [&](uint32_t i) { return F::from_ext(vars[fv[i]]); },
            [&](uint32_t i, const fl& x) { pre[i] = F::store(x); }, [&](uint32_t i) { return F::load(pre[i]); },
            [&](uint32_t i, const fl& v) {
              vars[fv[i]] = F::to_ext(v);
              resolved[fv[i]]++;
            },
            ex);
        flush_items++;
        continue;
      }
      if (kind8 & sd::kFrac) {
        const size_t j = r.row;
        const uint32_t mask = r.kw >> 8, kind = kind8 & 0x7fu;
        CHECK(kind == sp::OUT_MUL || kind == sp::OUT_INV);
        CHECK(kind == sp::OUT_INV || mask);
        fl num[4], den[4];
        bool after_zero = false;
        for (int i = 0; i < 4; i++) {
          const uint32_t id = c.wv[i * n + j];
          CHECK(((mask >> i) & 1) == (uint32_t)pend.count(id));
          if ((mask >> i) & 1) CHECK(c.zero[(sp::Q_HASH + i) * n + j]);
          num[i] = F::from_ext(vars[id]);
          den[i] = F::one();
          if ((mask >> i) & 1) {
            den[i] = F::load(side[(size_t)D.dslot[id]]);
            after_zero |= zeroed.count(id) != 0;
            for (int i2 = 0; i2 < i; i2++)
              if (c.wv[i2 * n + j] == id) on_two_cells++;
          }
        }
        behind_zero_den += after_zero;
        const uint32_t target = c.wv[4 * n + j];
        const fl konst = kind == sp::OUT_MUL ? inverse_const(c.q(sp::Q_O, j)) : F::zero();
        fl n4, d4;
        const bool zd = Dv::row_value_frac([&](int s) { return c.q(s, j); }, kind, num, den, konst, &n4, &d4);
        CHECK(!F::is_zero(d4));  // the invariant
        if (zd) {
          status = std::min<uint64_t>(status, j);
          zeroed.insert(target);
          zero_dens++;
        }
        vars[target] = F::to_ext(n4);
        CHECK(D.dslot[target] >= 0 && (size_t)D.dslot[target] < D.slots);
        side[(size_t)D.dslot[target]] = F::store(d4);
        joined.push_back(target);
        defined[target]++;
        frac_rows++;
        continue;
      }
      // a direct item: nothing it reads is pending
      const uint32_t kind = sp::row_kind(r);
      CHECK(kind != sp::OUT_INV);
      if (sp::is_hint_kind(kind)) {
        CHECK(!pend.count(P.hints[r.row].src));
      } else {
        for (int i = 0; i < 5; i++) CHECK(!pend.count(c.wv[i * n + r.row]));
      }
      if (direct_item(c, P, r, ex, vars)) status = std::min<uint64_t>(status, r.row);
    }
    if (D.flush_level[l]) {
      // why this flush stands here: the items of the level behind it that read a pending variable's plain value
      if (l + 1 < D.levels)
        for (uint32_t k = D.level_off[l + 1]; k < D.level_off[l + 2]; k++) {
          const sp::Row& r = D.rows[k];
          const uint32_t kind = r.kw & 0x7fu;
          if (sp::is_hint_kind(kind)) {
            as_hint_source += (int)pend.count(P.hints[r.row].src);
            continue;
          }
          for (int i = 0; i < 5; i++) {
            if (!pend.count(c.wv[i * n + r.row])) continue;
            if (kind == sp::ROOT5 || kind == sp::LIN) as_root_or_lin_input++;
            else if (i < 4 && !c.zero[(sp::Q_HASH + i) * n + r.row]) on_hash_cell++;
          }
        }
      pend.clear();
    }
    for (uint32_t v : joined) pend.insert(v);
    CHECK(pend.size() <= D.slots);
  }
  CHECK(pend.empty());
  for (size_t v = 0; v < P.slot.size(); v++) CHECK(resolved[v] == defined[v] && defined[v] <= 1 && (defined[v] == 1) == (D.dslot[v] >= 0));
  return status;
}

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), sizeof(T) * a.size()));
}

static int circuits = 0, values_compared = 0, flagged[4] = {0, 0, 0, 0};

static void one_circuit(int t, const sv29::Exps& ex) {
  const uint32_t flags = (uint32_t)t % 4;
  const size_t n = 96, G = 8;
  Circuit c(n, 1, 1200);
  int bits_hints = 0;  // (three at the most: 254 targets each)
  const fe one = ext_of(1);
  // variables 0 (value 0) and 1 (value 1) and G random ones are given; variable 2 is the public input of row 0 - given,
  // or, under both flags, derived by a LIN equality row
  std::vector<uint32_t> given = {0, 1};
  std::vector<fe> val(c.num_vars, plain_zero());
  val[1] = one;
  const uint32_t pub = 2;
  uint32_t next = 3;
  std::vector<uint32_t> pool;
  for (size_t g = 0; g < G; g++) {
    const uint32_t r = (uint32_t)(rnd() % 6);
    val[next] = r == 0 ? ext_of(0) : r == 1 ? one : r == 2 ? ext_neg(one) : rnd_ext();
    given.push_back(next);
    pool.push_back(next++);
  }
  const bool derive = flags == 3;
  if (!derive) {
    val[pub] = rnd_ext();
    given.push_back(pub);
  }
  {
    const uint32_t w[5] = {0, 0, 0, 0, pub};
    c.wires(0, w);
    c.set(sp::Q_O, 0, one);
  }
  auto pick = [&]() -> uint32_t {
    // the newest variables most of the time: chains
    if (rnd() % 3) return pool[pool.size() - 1 - rnd() % std::min<size_t>(3, pool.size())];
    return pool[rnd() % pool.size()];
  };
  auto eval_row = [&](size_t j, uint32_t kind, uint32_t wire) {
    fl w[5];
    for (int i = 0; i < 5; i++) w[i] = F::from_ext(val[c.wv[i * n + j]]);
    fl konst = F::zero();
    if (kind == sp::OUT_MUL) konst = inverse_const(c.q(sp::Q_O, j));
    if (kind == sp::ROOT5) konst = inverse_const(c.q(sp::Q_HASH + (int)wire, j));
    if (kind == sp::LIN) konst = inverse_const(c.q(sp::Q_LC + (int)wire, j));
    bool zd;
    val[c.wv[wire * n + j]] = F::to_ext(S::row_value<true, true>([&](int s) { return c.q(s, j); }, kind, wire, w, konst, ex, &zd));
  };
  bool pub_done = !derive;
  for (size_t j = 1; j < n - 2; j++) {
    const uint32_t roll = (uint32_t)(rnd() % 20);
    uint32_t w[5] = {pick(), pick(), pick(), pick(), pick()};
    if (roll < 9) {  // OUT_INV: an addition's row - sometimes a doubling, sometimes with a hash cell, sometimes a zero denominator
      if (rnd() % 4 == 0) w[1] = w[0];
      if (rnd() % 5 == 0) w[3] = w[2];
      w[4] = next++;
      c.wires(j, w);
      for (int s = 0; s < 4; s++)
        if (rnd() % 2) c.set(sp::Q_LC + s, j, rnd_ext());
      for (int s = 0; s < 2; s++)
        if (rnd() % 2) c.set(sp::Q_MUL + s, j, rnd_ext());
      if (rnd() % 2) c.set(sp::Q_C, j, rnd_ext());
      if (rnd() % 8 == 0) c.set(sp::Q_HASH + (int)(rnd() % 4), j, rnd_ext());
      c.set(sp::Q_ECC, j, rnd_ext());
      c.set(sp::Q_O, j, rnd_ext());
      if (rnd() % 10 == 0) {  // q_o = q_ecc w0 w1 w2 w3: the denominator vanishes
        fl p = c.q(sp::Q_ECC, j);
        for (int i = 0; i < 4; i++) p = F::mul(p, F::from_ext(val[w[i]]));
        c.sel[sp::Q_O * n + j] = F::pack(F::canonical(p));
        c.zero[sp::Q_O * n + j] = F::is_zero(p) ? 1 : 0;
      }
      eval_row(j, sp::OUT_INV, 4);
      pool.push_back(w[4]);
    } else if (roll < 13) {  // OUT_MUL: a select or a linear combination
      w[4] = next++;
      c.wires(j, w);
      for (int s = 0; s < 4; s++)
        if (rnd() % 2) c.set(sp::Q_LC + s, j, rnd_ext());
      if (rnd() % 2) c.set(sp::Q_MUL + (int)(rnd() % 2), j, rnd_ext());
      if (rnd() % 6 == 0) c.set(sp::Q_HASH + (int)(rnd() % 4), j, rnd_ext());
      c.set(sp::Q_O, j, rnd_ext());
      eval_row(j, sp::OUT_MUL, 4);
      pool.push_back(w[4]);
    } else if (roll < 15) {  // ROOT5 on wire i
      const int i = (int)(rnd() % 4);
      w[i] = next++;
      c.wires(j, w);
      c.set(sp::Q_HASH + i, j, rnd_ext());
      c.set(sp::Q_O, j, rnd_ext());
      c.set(sp::Q_C, j, rnd_ext());
      for (int s = 0; s < 4; s++)
        if (s != i && rnd() % 2) c.set(sp::Q_LC + s, j, rnd_ext());
      eval_row(j, sp::ROOT5, (uint32_t)i);
      pool.push_back(w[i]);
    } else if (roll < 17 && (flags & sp::RULE_LINEAR)) {  // LIN on wire i; the first one under both flags defines the public input
      const int i = (int)(rnd() % 4);
      w[i] = pub_done ? next++ : pub;
      c.wires(j, w);
      for (int s = 0; s < 4; s++)
        if (s == i || rnd() % 2) c.set(sp::Q_LC + s, j, rnd_ext());
      c.set(sp::Q_O, j, rnd_ext());
      eval_row(j, sp::LIN, (uint32_t)i);
      if (pub_done) pool.push_back(w[i]);
      pub_done = true;
    } else if (roll < 20 && pool.size() > G) {  // a hint on the newest value; its targets feed later rows
      const uint32_t src = pool.back(), kind = bits_hints < 3 ? (uint32_t)(rnd() % 3) : 1 + (uint32_t)(rnd() % 2);
      bits_hints += kind == sp::HINT_BITS;
      const uint32_t cnt = kind == sp::HINT_BITS ? 254 : 1;
      c.hints.push_back(sp::Hint{kind, src, (uint32_t)c.targets.size(), cnt});
      const fe plain = S::hint_plain(val[src]);
      for (uint32_t b = 0; b < cnt; b++) {
        c.targets.push_back(next);
        val[next] = kind == sp::HINT_BITS    ? S::bit_image((S::word_of(plain, b / 32) >> (b % 32)) & 1)
                    : kind == sp::HINT_ISZERO ? S::hint_iszero(val[src])
                                              : S::hint_inv0(val[src], ex);
        if (b < 3) pool.push_back(next);
        next++;
      }
    }  // else: an empty row
  }
  if (!pub_done) {  // no LIN row came: the last row defines the public input
    const uint32_t w[5] = {pick(), pub, 0, 0, 0};
    c.wires(n - 1, w);
    c.set(sp::Q_LC, n - 1, one);
    c.set(sp::Q_LC + 1, n - 1, ext_neg(one));
    eval_row(n - 1, sp::LIN, 1);
  }
  CHECK(next <= c.num_vars);
  sp::Plan P;
  const bool ok = sp::solve_plan_rules(n, 1, c.num_vars, c.wv.data(), c.zero.data(), given.data(), given.size(), c.hints.data(),
                                       c.hints.size(), c.targets.data(), c.targets.size(), flags, &P);
  CHECK(ok);
  if (!ok) {
    printf("  (circuit %d: %s)\n", t, P.error.c_str());
    return;
  }
  const sp::Plan before = P;
  sd::Sched D;
  sd::defer_plan(P, n, c.wv.data(), c.zero.data(), &D);
  CHECK(same_bytes(P.rows, before.rows) && same_bytes(P.level_off, before.level_off) && same_bytes(P.slot, before.slot) &&
        same_bytes(P.hints, before.hints) && same_bytes(P.targets, before.targets) && P.levels == before.levels);
  // the schedule's own figures
  uint64_t fracs = 0, flushes = 0, inv_rows = 0;
  for (const sp::Row& r : D.rows) {
    fracs += (r.kw & 0xffu) != sd::FLUSH && (r.kw & sd::kFrac);
    flushes += (r.kw & 0xffu) == sd::FLUSH;
    inv_rows += (r.kw & 0xffu) == (sp::OUT_INV | sd::kFrac);
  }
  CHECK(fracs == D.frac_rows && D.deferred_vars == D.frac_rows && flushes == D.flush_items && inv_rows == P.inv_rows);
  CHECK(D.rows.size() == P.rows.size() + D.flush_items && D.levels == P.levels + D.flush_levels);
  {  // PENDING is empty behind a flush and only an OUT_INV row fills it again: no more flush levels than levels with such a row
    uint64_t inv_levels = 0;
    for (size_t l = 0; l < P.levels; l++) {
      bool any = false;
      for (uint32_t k = P.level_off[l]; k < P.level_off[l + 1]; k++) any |= sp::row_kind(P.rows[k]) == sp::OUT_INV;
      inv_levels += any;
    }
    CHECK(D.flush_levels <= inv_levels && inv_levels <= D.inv_levels_direct);
  }
  std::vector<fe> given_vals(given.size());
  for (size_t k = 0; k < given.size(); k++) given_vals[k] = val[given[k]];
  std::vector<fe> direct, deferred;
  const uint64_t st_direct = walk_direct(c, P, ex, given_vals, &direct);
  const uint64_t st_deferred = t % 2 ? walk_deferred<sv29::kInvGcd>(c, P, D, ex, given_vals, &deferred)
                                     : walk_deferred<sv29::kInvFermat>(c, P, D, ex, given_vals, &deferred);
  CHECK(st_direct == st_deferred);
  for (size_t v = 0; v < c.num_vars; v++) {
    CHECK(same_words(direct[v], deferred[v]));
    if (v < next) CHECK(same_words(direct[v], val[v]));  // ... and both are the values the circuit was made with
    values_compared++;
  }
  circuits++;
  flagged[flags]++;
}

int main() {
  sv29::Exps ex;
  CHECK(sv29::derive_exps(&ex));
  for (int t = 0; t < 300; t++) one_circuit(t, ex);
  CHECK(on_hash_cell > 0 && as_hint_source > 0 && as_root_or_lin_input > 0 && on_two_cells > 0 && behind_zero_den > 0);
  CHECK(zero_dens > 0 && frac_rows > 0 && flush_items > 0);
  printf("circuits=%d flags=%d/%d/%d/%d values=%d frac_rows=%d flush_items=%d zero_dens=%d cases: hash=%d hint=%d root_lin=%d "
         "two_cells=%d behind_zero=%d bad=%d\n",
         circuits, flagged[0], flagged[1], flagged[2], flagged[3], values_compared, frac_rows, flush_items, zero_dens, on_hash_cell,
         as_hint_source, as_root_or_lin_input, on_two_cells, behind_zero_den, bad);
  return bad ? 1 : 0;
}
