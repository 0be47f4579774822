// Host-side check of the packed witness solver: cap_amd/csrc/solve_pack.hpp (the item decode and the choice of W) with
// solve_plan.hpp and solve29.hpp, field29.hpp's bound assertions on.  Stand-alone; prints one summary line that
// tests/test_solve_pack_host.py reads, "bad=0" when every check held.
//   - one packed workgroup is emulated with the kernel's own decode: scatter slot by slot, then the levels in order, every
//     lane running its stride over a level's items to the end before the next lane starts (a dependency inside a level
//     would show), an empty slot doing nothing
//   - the result is compared word for word with the row-by-row solve of each witness alone, statuses included, for
//     W in {1, 2, 4, 8, 16}, count in {1, W-1, W, W+1, 2W+3}, with and without a witness list, with row strides larger
//     than num_vars and num_given; rows of witnesses outside the list and the tails of the rows keep their guard words
//   - the circuit has a level wider than a workgroup's lanes at every W (300 rows) and levels of one row
//   - a zero denominator in slot 1 of a workgroup leaves slots 0 and 2 what their lone solves give
//   - the automatic rule on hand-made width profiles
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/solve29.hpp"
#include "../../cap_amd/csrc/solve_pack.hpp"
#include "../../cap_amd/csrc/solve_plan.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace cap;
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

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
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
static fe sel_of(const fe& ext) { return F::pack(F::canonical(F::from_ext(ext))); }
static fe guard() {
  fe a;
  for (int i = 0; i < 8; i++) a.v[i] = 0xdeadbeefu;
  return a;
}
static bool same_words(const fe& a, const fe& b) { return !memcmp(&a, &b, sizeof a); }

struct Circuit {
  size_t n, num_vars;
  std::vector<uint32_t> wv;  // [5][n]
  std::vector<fe> sel;       // [13][n], device form
  std::vector<uint8_t> zero;
  std::vector<fe> konst;  // per plan row, once the plan stands
  sp::Plan P;
  Circuit(size_t n_, size_t nv) : n(n_), num_vars(nv), wv(5 * n_, 0), sel(13 * n_), zero(13 * n_, 1) {
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
  bool plan(const std::vector<uint32_t>& given) {
    if (!sp::solve_plan(n, 0, num_vars, wv.data(), zero.data(), given.data(), given.size(), &P)) return false;
    konst.resize(P.rows.size());
    for (size_t k = 0; k < P.rows.size(); k++) {
      const uint32_t kind = sp::row_kind(P.rows[k]);
      fl x = F::one();
      if (kind == sp::OUT_MUL) x = F::load(sel[sp::Q_O * n + P.rows[k].row]);
      if (kind == sp::ROOT5) x = F::load(sel[(sp::Q_HASH + sp::row_wire(P.rows[k])) * n + P.rows[k].row]);
      konst[k] = F::pack(F::canonical(F::inv(x)));
    }
    return true;
  }
};

// plan row k for the witness whose variables are `vars`; returns whether the denominator vanished
static bool run_row(const Circuit& c, size_t k, fe* vars, const sv29::Exps& ex) {
  const size_t j = c.P.rows[k].row;
  const uint32_t kind = sp::row_kind(c.P.rows[k]), wire = sp::row_wire(c.P.rows[k]);
  fl w[5];
  for (int i = 0; i < 5; i++) w[i] = F::from_ext(vars[c.wv[i * c.n + j]]);
  bool zd;
  const fl val = S::row_value([&](int s) { return F::load(c.sel[s * c.n + j]); }, kind, wire, w, F::load(c.konst[k]), ex, &zd);
  vars[c.wv[wire * c.n + j]] = F::to_ext(val);
  return zd;
}

// one witness alone, row by row in plan order (what tests/cpp/solve_plan_check.cpp does)
static unsigned long long solve_alone(const Circuit& c, const fe* given, fe* vars, const sv29::Exps& ex) {
  for (size_t v = 0; v < c.num_vars; v++) vars[v] = c.P.slot[v] >= 0 ? given[c.P.slot[v]] : ext_of(0);
  unsigned long long first = ~0ull;
  for (size_t k = 0; k < c.P.rows.size(); k++)
    if (run_row(c, k, vars, ex) && c.P.rows[k].row < first) first = c.P.rows[k].row;
  return first;
}

static size_t items_run = 0;
// workgroup `block` of a launch at W over `count` list entries, as k_solve_vars_packed<W> walks it
static void packed_block(const Circuit& c, uint32_t W, uint32_t block, uint32_t count, const uint32_t* which, const fe* given,
                         size_t given_stride, fe* vars_out, size_t vars_stride, unsigned long long* status,
                         const sv29::Exps& ex) {
  for (uint32_t s = 0; s < W; s++) {
    const uint32_t entry = spk::slot_entry(block, s, W);
    if (entry >= count) break;
    const size_t p = spk::entry_witness(which, entry);
    for (uint32_t lane = 0; lane < kThreads; lane++)
      for (size_t v = lane; v < c.num_vars; v += kThreads)
        vars_out[p * vars_stride + v] = c.P.slot[v] >= 0 ? given[p * given_stride + c.P.slot[v]] : ext_of(0);
  }
  for (size_t l = 0; l < c.P.levels; l++) {
    const uint32_t begin = c.P.level_off[l], items = spk::level_items(c.P.level_off[l + 1] - begin, W);
    for (uint32_t lane = 0; lane < kThreads; lane++)
      for (uint32_t i = lane; i < items; i += kThreads) {
        const spk::Item it = spk::item_decode(begin, i, W);
        CHECK(it.slot < W && it.k >= begin && it.k < c.P.level_off[l + 1]);
        const uint32_t entry = spk::slot_entry(block, it.slot, W);
        if (entry >= count) continue;
        const size_t p = spk::entry_witness(which, entry);
        if (run_row(c, it.k, vars_out + p * vars_stride, ex)) {
          const unsigned long long j = c.P.rows[it.k].row;
          if (j < status[p]) status[p] = j;
        }
        items_run++;
      }
  }
}

// The circuit: 8 given variables (0 .. 7); level 1: 300 OUT_MUL rows and one OUT_INV row (`inv_row`, whose denominator is
// q_o - q_ecc v0 v1 v2 v3 - the given values themselves); level 2: one ROOT5 row; level 3: 20 OUT_MUL rows and a second
// OUT_INV row reading the first one's value; level 4: one ROOT5 row on wire 2; level 5: one OUT_MUL row.
struct Built {
  Circuit c;
  size_t inv_row, inv_row2;
};
static Built build() {
  Built b{Circuit(512, 8 + 330), 0, 0};
  Circuit& c = b.c;
  uint32_t next = 8;
  size_t j = 0;
  auto g = [] { return (uint32_t)(rnd() % 8); };
  std::vector<uint32_t> l1;
  for (int t = 0; t < 300; t++, j++) {
    for (int s = 0; s < 12; s++) c.set(s, j, rnd_ext());
    c.wires(j, g(), g(), g(), g(), next);
    l1.push_back(next++);
  }
  b.inv_row = j;
  for (int s = 0; s < 13; s++) c.set(s, j, rnd_ext());
  c.wires(j, 0, 1, 2, 3, next);
  const uint32_t inv1 = next++;
  j++;
  // level 2: ROOT5 on wire 0, the known value on wire 4 from level 1
  for (int s = 0; s < 12; s++) c.set(s, j, rnd_ext());
  c.set(sp::Q_LC, j, ext_of(0));
  c.set(sp::Q_MUL, j, ext_of(0));
  c.wires(j, next, l1[3], l1[7], g(), l1[11]);
  const uint32_t root1 = next++;
  j++;
  std::vector<uint32_t> l3;
  for (int t = 0; t < 20; t++, j++) {
    for (int s = 0; s < 12; s++) c.set(s, j, rnd_ext());
    c.wires(j, root1, l1[t], g(), l1[299 - t], next);
    l3.push_back(next++);
  }
  b.inv_row2 = j;
  for (int s = 0; s < 13; s++) c.set(s, j, rnd_ext());
  c.wires(j, root1, inv1, 4, 5, next);
  const uint32_t inv2 = next++;
  j++;
  for (int s = 0; s < 12; s++) c.set(s, j, rnd_ext());
  c.set(sp::Q_LC + 2, j, ext_of(0));
  c.set(sp::Q_MUL + 1, j, ext_of(0));
  c.wires(j, l3[0], l3[19], next, inv2, l3[5]);
  const uint32_t root2 = next++;
  j++;
  for (int s = 0; s < 12; s++) c.set(s, j, rnd_ext());
  c.wires(j, root2, inv2, l3[2], g(), next);
  next++;
  j++;
  CHECK(c.plan({0, 1, 2, 3, 4, 5, 6, 7}));
  if (!c.P.error.empty()) printf("plan refused: %s\n", c.P.error.c_str());
  CHECK(c.P.levels == 5 && c.P.widest_level == 301 && c.P.inv_rows == 2 && c.P.root_rows == 2 && next <= c.num_vars);
  CHECK(c.P.level_off[2] - c.P.level_off[1] == 1);  // narrower than every W > 1
  return b;
}

static int cases = 0, zero_dens = 0;
// `total` witnesses with strides beyond the rows' lengths; the launch covers `count` of them (a list, or 0 .. count - 1)
static void check_case(const Circuit& c, uint32_t W, uint32_t count, bool listed, const std::vector<fe>& all_given,
                       uint32_t total, const std::vector<std::vector<fe>>& alone, const std::vector<unsigned long long>& alone_st,
                       const sv29::Exps& ex) {
  const size_t num_given = c.P.num_given, gs = num_given + 3, vs = c.num_vars + 5;
  std::vector<uint32_t> which;
  if (listed) {  // a non-monotone slice of a permutation: 5, 0, 3, 8, 1, ...
    const uint32_t perm[] = {5, 0, 3, 8, 1, 12, 7, 2, 10, 4, 14, 9, 6, 13, 11};
    for (uint32_t i = 0, t = 0; which.size() < count; i++) {
      const uint32_t p = i < 15 ? perm[i] : 15 + t++;
      if (p < total) which.push_back(p);
    }
  }
  std::vector<fe> given((size_t)total * gs, guard()), vars((size_t)total * vs, guard());
  for (uint32_t p = 0; p < total; p++)
    for (size_t k = 0; k < num_given; k++) given[p * gs + k] = all_given[p * num_given + k];
  std::vector<unsigned long long> st(total, ~0ull);
  for (uint32_t b = 0; b < spk::blocks_for(count, W); b++)
    packed_block(c, W, b, count, listed ? which.data() : nullptr, given.data(), gs, vars.data(), vs, st.data(), ex);
  std::vector<uint8_t> in_launch(total, 0);
  for (uint32_t e = 0; e < count; e++) in_launch[listed ? which[e] : e] = 1;
  for (uint32_t p = 0; p < total; p++) {
    for (size_t v = 0; v < vs; v++) {
      const fe& got = vars[p * vs + v];
      if (in_launch[p] && v < c.num_vars) {
        if (!same_words(got, alone[p][v])) {
          bad++;
          printf("FAILED W=%u count=%u listed=%d: witness %u variable %zu differs from its lone solve\n", W, count, listed, p, v);
          return;
        }
      } else if (!same_words(got, guard())) {
        bad++;
        printf("FAILED W=%u count=%u listed=%d: witness %u word %zu was written\n", W, count, listed, p, v);
        return;
      }
    }
    CHECK(st[p] == (in_launch[p] ? alone_st[p] : ~0ull));
  }
  cases++;
}

static void check_auto_rule() {
  auto profile = [](std::vector<uint32_t> widths) {
    std::vector<uint32_t> off{0};
    for (uint32_t w : widths) off.push_back(off.back() + w);
    return spk::median_level_width(off.data(), widths.size());
  };
  CHECK(profile({18}) == 18 && profile({600, 1, 18, 18, 2}) == 18 && profile({1, 1, 1, 900}) == 1);
  CHECK(profile({200, 200, 3}) == 200 && profile({}) == 0 && profile({4, 9}) == 4);
  const int T = (int)kThreads;
  CHECK(spk::auto_pack(18, T) == 8 && spk::auto_pack(1, T) == 16 && spk::auto_pack(200, T) == 1);
  CHECK(spk::auto_pack(16, T) == 16 && spk::auto_pack(17, T) == 8 && spk::auto_pack(128, T) == 2 && spk::auto_pack(129, T) == 1);
  CHECK(spk::auto_pack(0, T) == 16);
  // the count term: a lone witness runs unpacked, 3 witnesses at most 2 per workgroup
  CHECK(spk::pack_for(0, 8, 1) == 1 && spk::pack_for(0, 16, 1) == 1 && spk::pack_for(16, 16, 1) == 1);
  CHECK(spk::pack_for(0, 8, 3) == 2 && spk::pack_for(0, 8, 2) == 2 && spk::pack_for(0, 8, 7) == 4 && spk::pack_for(0, 8, 8) == 8);
  CHECK(spk::pack_for(0, 8, 256) == 8 && spk::pack_for(0, 16, 4096) == 16 && spk::pack_for(0, 16, 15) == 8);
  CHECK(spk::pack_for(0, 1, 4096) == 1);
  // a forced W holds whatever the count (beyond one)
  CHECK(spk::pack_for(4, 8, 3) == 4 && spk::pack_for(16, 1, 2) == 16 && spk::pack_for(1, 16, 4096) == 1);
  for (int w = -2; w <= 40; w++) CHECK(spk::valid_setting(w) == (w == 0 || w == 1 || w == 2 || w == 4 || w == 8 || w == 16));
  CHECK(spk::blocks_for(1, 16) == 1 && spk::blocks_for(16, 16) == 1 && spk::blocks_for(17, 16) == 2 && spk::blocks_for(5, 1) == 5);
}

int main() {
  sv29::Exps ex;
  CHECK(sv29::derive_exps(&ex));
  check_auto_rule();
  Built b = build();
  Circuit& c = b.c;
  const uint32_t total = 2 * 16 + 3;  // the largest count
  const size_t ng = c.P.num_given;
  std::vector<fe> given((size_t)total * ng);
  for (auto& x : given) x = rnd_ext();
  // witness 1's first OUT_INV denominator vanishes: q_ecc = q_o / (v0 v1 v2 v3) for ITS values.  In a launch without a
  // list witness 1 sits in slot 1 of workgroup 0 at every W > 1, between witnesses 0 and 2.
  {
    fl prod = F::one();
    for (int i = 0; i < 4; i++) prod = F::mul(prod, F::from_ext(given[1 * ng + i]));
    const fl qe = F::mul(F::load(c.sel[sp::Q_O * c.n + b.inv_row]), F::inv(prod));
    c.sel[sp::Q_ECC * c.n + b.inv_row] = F::pack(F::canonical(qe));
  }
  std::vector<std::vector<fe>> alone(total, std::vector<fe>(c.num_vars));
  std::vector<unsigned long long> alone_st(total);
  for (uint32_t p = 0; p < total; p++) {
    alone_st[p] = solve_alone(c, &given[p * ng], alone[p].data(), ex);
    CHECK(alone_st[p] == (p == 1 ? b.inv_row : ~0ull));
  }
  CHECK(F::is_zero(F::from_ext(alone[1][c.wv[4 * c.n + b.inv_row]])));
  zero_dens += alone_st[1] == b.inv_row;
  const uint32_t Ws[] = {1, 2, 4, 8, 16};
  for (uint32_t W : Ws) {
    const uint32_t counts[] = {1, W - 1, W, W + 1, 2 * W + 3};
    for (uint32_t count : counts) {
      if (!count) continue;  // (W = 1: W - 1 is an empty launch)
      check_case(c, W, count, false, given, total, alone, alone_st, ex);
      check_case(c, W, count, true, given, total, alone, alone_st, ex);
    }
  }
  // the level of 301 rows is wider than the workgroup's lanes at every W, the one-row levels narrower than every W > 1
  CHECK(spk::level_items(301, 1) > kThreads && spk::level_items(1, 2) < 2 * kThreads);
  printf("bad=%d cases=%d items=%zu zero_dens=%d\n", bad, cases, items_run, zero_dens);
  return bad ? 1 : 0;
}
