// Host-side check of cap_amd/csrc/invgcd29.hpp (Fr inversion by a constant-time GCD in jumps of divsteps) and of the GCD
// form of the witness solver's row rule (solve29.hpp), with field29.hpp's bound assertions on.  Stand-alone; prints one
// summary line that tests/test_inv_gcd_host.py reads, "bad=0" when every check held.
//   For every vector a (internal Montgomery form, normalized, possibly lazy):
//     - canonical(inv_gcd(a)) == canonical(pow_fixed(a, r - 2)), limb for limb
//     - mul(a, inv_gcd(a)) == 1 unless a = 0 (mod r)
//     - the loop ended in g = 0 and f = +-1 (f = r for a = 0 mod r)
//   Vectors, each taken twice - as the field element x (a = x 2^261 mod r) and as the integer the GCD itself starts from
//   (the limbs of a ARE the vector) - and the latter also as the lazy representatives a + r and a + 7r (all below 2^261):
//     0, 1, 2, r - 1, r - 2, (r - 1) / 2, (r + 1) / 2;  2^k, 2^k - 1 and r - 2^k for k = 0 .. 253;  100 000 SplitMix64 values
//   Then random circuits (OUT rows with and without q_ecc, fifth roots, forced zero denominators) are solved row by row
//   through row_value in both forms: every value, every zero_den flag and every INV0 hint equal, word for word.
#define CAP_FL_CHECK 1
#include "../../cap_amd/csrc/solve29.hpp"
#include "../../cap_amd/csrc/solve_plan.hpp"

#include <cstdio>
#include <cstring>
#include <vector>
using namespace cap;
using SF = sv29::Solve<CAP_FL_SCHED, sv29::kInvFermat>;
using SG = sv29::Solve<CAP_FL_SCHED, sv29::kInvGcd>;
using F = SF::F;

static int bad = 0;
#define CHECK(x)                                    \
  do {                                              \
    if (!(x)) {                                     \
      bad++;                                        \
      if (bad < 20) printf("FAILED line %d: %s\n", __LINE__, #x); \
    }                                               \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
CAP_WRAPS static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// ---- 256-bit integers, 8 words ---------------------------------------------------------------------------------
struct U {
  uint32_t w[8];
};
static U u_small(uint32_t x) {
  U a{};
  a.w[0] = x;
  return a;
}
static U u_sub(const U& a, const U& b) {
  U r;
  int64_t c = 0;
  for (int i = 0; i < 8; i++) {
    c += (int64_t)a.w[i] - b.w[i];
    r.w[i] = (uint32_t)c;
    c >>= 32;
  }
  return r;
}
static U u_add(const U& a, const U& b) { return u_sub(a, u_sub(u_small(0), b)); }
static U u_pow2(int k) {
  U a{};
  a.w[k / 32] = 1u << (k % 32);
  return a;
}
static U u_half(const U& a) {
  U r;
  for (int i = 0; i < 8; i++) r.w[i] = (a.w[i] >> 1) | (i < 7 ? a.w[i + 1] << 31 : 0);
  return r;
}
static U modulus() {
  const fe p = F::pack(F::konst(FrP29::MOD));
  U r;
  memcpy(r.w, p.v, sizeof r.w);
  return r;
}
static fe fe_of(const U& a) {
  fe x;
  memcpy(x.v, a.w, sizeof a.w);
  return x;
}

// ---- one vector ----------------------------------------------------------------------------------------------------
static sv29::Exps ex;
static long vectors = 0, zeros = 0, neg_f = 0;

static bool limbs_equal(const fl& a, const fl& b) { return !memcmp(a.v, b.v, sizeof a.v); }

static void check_one(const fl& a) {
  ig29::End end;
  const fl inv = inv_gcd<FrP29, CAP_FL_SCHED>(a, &end);
  for (int i = 0; i < 9; i++) CHECK(inv.v[i] < (1u << 29));
  const fl want = F::canonical(SF::pow_fixed(a, ex.inv));
  CHECK(limbs_equal(F::canonical(inv), want));
  CHECK(limbs_equal(inv, inv_gcd<FrP29, CAP_FL_SCHED>(a)));
  const bool zero = F::is_zero(a);
  bool g0 = true, f_one = end.f.v[0] == 1, f_minus = true, f_mod = true;
  for (int i = 0; i < 9; i++) {
    g0 &= end.g.v[i] == 0;
    if (i) f_one &= end.f.v[i] == 0;
    f_minus &= end.f.v[i] == (i < 8 ? (int32_t)F::M29 : -1);
    f_mod &= end.f.v[i] == (int32_t)FrP29::MOD[i];
  }
  CHECK(g0);
  if (zero) {
    CHECK(f_mod);
    CHECK(F::is_zero(inv));
    zeros++;
  } else {
    CHECK(f_one || f_minus);
    CHECK(F::eq(F::mul(a, inv), F::one()));
    neg_f += f_minus;
  }
  vectors++;
}

// a + k r, carried (k r < 2^257: normalized whenever a is)
static fl plus_mod(const fl& a, uint32_t k) {
  fl r;
  for (int i = 0; i < 9; i++) r.v[i] = a.v[i] + k * FrP29::MOD[i];  // limbs below 2^29 + 7 * 2^29
  return F::normalize(r);
}

static void check_vector(const U& x) {
  check_one(F::to_mont(fe_of(x)));  // as the field element x
  const fl raw = F::unpack(fe_of(x));  // as the integer the GCD starts from
  check_one(raw);
  check_one(plus_mod(raw, 1));
  check_one(plus_mod(raw, 7));
}

// ---- the row rule in both forms on random circuits -------------------------------------------------------------------
static fe rnd_ext() {
  fe a;
  for (int i = 0; i < 8; i++) a.v[i] = (uint32_t)rnd();
  a.v[7] &= 0x0fffffffu;  // below 2^252 < r
  return F::to_ext(F::to_mont(a));
}
static fe ext_of(uint32_t x) { return F::to_ext(F::to_mont(fe_of(u_small(x)))); }
static fe sel_of(const fe& ext) { return F::pack(F::canonical(F::from_ext(ext))); }

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
};

static long rows_compared = 0, inv_rows = 0, root_rows = 0, flagged_rows = 0;

// the solve as the kernel runs it, row after row in plan order, in form S; flags: zero_den per plan row
template <class S>
static void solve(const Circuit& c, const sp::Plan& P, const std::vector<fe>& given, std::vector<fe>* vars,
                  std::vector<uint8_t>* flags) {
  vars->assign(c.num_vars, ext_of(0));
  flags->assign(P.rows.size(), 0);
  for (size_t v = 0; v < c.num_vars; v++)
    if (P.slot[v] >= 0) (*vars)[v] = given[P.slot[v]];
  for (size_t k = 0; k < P.rows.size(); k++) {
    const size_t j = P.rows[k].row;
    const uint32_t kind = sp::row_kind(P.rows[k]), wire = sp::row_wire(P.rows[k]);
    fl x = F::one();
    if (kind == sp::OUT_MUL) x = F::load(c.sel[sp::Q_O * c.n + j]);
    if (kind == sp::ROOT5) x = F::load(c.sel[(sp::Q_HASH + wire) * c.n + j]);
    const fl konst = F::canonical(F::inv(x));
    fl w[5];
    for (int i = 0; i < 5; i++) w[i] = F::from_ext((*vars)[c.wv[i * c.n + j]]);
    bool zd;
    const fl val = S::row_value([&](int s) { return F::load(c.sel[s * c.n + j]); }, kind, wire, w, konst, ex, &zd);
    (*flags)[k] = zd;
    (*vars)[c.wv[wire * c.n + j]] = F::to_ext(val);
  }
}

static void check_random(size_t n, size_t num_inputs, bool degenerate) {
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
  for (size_t j = num_inputs; j < n - n / 8; j++) {
    uint32_t w[5] = {pick(), pick(), pick(), pick(), 0};
    const uint32_t kind = (uint32_t)(rnd() % 8), u = next++;
    if (kind < 2) {  // OUT without q_ecc
      for (int s = 0; s < 12; s++) c.set(s, j, rnd_ext());
      w[4] = u;
    } else if (kind < 5) {  // OUT with q_ecc, q_o = 0 half the time (unless a wire holds the zero variable)
      for (int s = 0; s < 13; s++) c.set(s, j, rnd_ext());
      if ((rnd() & 1) && w[0] && w[1] && w[2] && w[3]) c.set(sp::Q_O, j, ext_of(0));
      w[4] = u;
      ecc_rows.push_back(j);
    } else {  // ROOT5 on a random wire, the known value on wire 4
      const uint32_t wire = (uint32_t)(rnd() % 4);
      for (int s = 0; s < 12; s++) c.set(s, j, rnd_ext());
      c.set(sp::Q_LC + wire, j, ext_of(0));
      c.set(sp::Q_MUL + wire / 2, j, ext_of(0));
      w[4] = pick();
      w[wire] = u;
    }
    c.wires(j, w[0], w[1], w[2], w[3], w[4]);
    pool.push_back(u);
  }
  sp::Plan P;
  CHECK(sp::solve_plan(c.n, c.num_inputs, c.num_vars, c.wv.data(), c.zero.data(), given.data(), given.size(), &P));
  if (!P.error.empty()) {
    printf("plan refused: %s\n", P.error.c_str());
    return;
  }
  std::vector<fe> gv(num_given);
  for (auto& x : gv) x = rnd_ext();
  gv[0] = ext_of(0);
  gv[1] = ext_of(1);
  std::vector<fe> vf, vg;
  std::vector<uint8_t> ff, fg;
  if (degenerate && ecc_rows.size() >= 3) {  // q_ecc = q_o / (w0 w1 w2 w3) at two rows: their denominators vanish
    solve<SF>(c, P, gv, &vf, &ff);
    for (size_t t : {ecc_rows.size() - 1, ecc_rows.size() / 2}) {
      const size_t j = ecc_rows[t];
      fl prod = F::one();
      for (int i = 0; i < 4; i++) prod = F::mul(prod, F::from_ext(vf[c.wv[i * n + j]]));
      if (F::is_zero(prod)) continue;
      if (F::is_zero(F::load(c.sel[sp::Q_O * n + j]))) c.set(sp::Q_O, j, ext_of(11));
      c.sel[sp::Q_ECC * n + j] = F::pack(F::canonical(F::mul(F::load(c.sel[sp::Q_O * n + j]), F::inv(prod))));
    }
  }
  solve<SF>(c, P, gv, &vf, &ff);
  solve<SG>(c, P, gv, &vg, &fg);
  CHECK(vf.size() == vg.size() && !memcmp(vf.data(), vg.data(), sizeof(fe) * vf.size()));
  CHECK(ff == fg);
  long fl_rows = 0;
  for (size_t k = 0; k < P.rows.size(); k++) {
    fl_rows += ff[k];
    if (ff[k]) CHECK(F::is_zero(F::from_ext(vg[c.wv[sp::row_wire(P.rows[k]) * n + P.rows[k].row]])));
  }
  CHECK(degenerate ? fl_rows >= 1 : fl_rows == 0);
  flagged_rows += fl_rows;
  rows_compared += (long)P.rows.size();
  inv_rows += (long)P.inv_rows;
  root_rows += (long)P.root_rows;
}

static void check_hints() {
  for (int t = 0; t < 16; t++) {
    const fe src = t == 0 ? ext_of(0) : t == 1 ? ext_of(1) : rnd_ext();
    const fe a = SF::hint_inv0(src, ex), b = SG::hint_inv0(src, ex);
    CHECK(!memcmp(&a, &b, sizeof a));
    if (t == 0) CHECK(!memcmp(&b, &src, sizeof b));  // 0 -> 0
    if (t == 1) CHECK(!memcmp(&b, &src, sizeof b));  // 1 -> 1
  }
}

int main(int argc, char** argv) {
  const long randoms = argc > 1 ? atol(argv[1]) : 100000;
  CHECK(sv29::derive_exps(&ex));
  static_assert(ig29::kJumps * ig29::kJump >= 735, "the proven divstep count");
  const U r = modulus();
  check_vector(u_small(0));
  check_vector(u_small(1));
  check_vector(u_small(2));
  check_vector(u_sub(r, u_small(1)));
  check_vector(u_sub(r, u_small(2)));
  check_vector(u_half(u_sub(r, u_small(1))));
  check_vector(u_half(u_add(r, u_small(1))));
  for (int k = 0; k < 254; k++) {
    check_vector(u_pow2(k));
    check_vector(u_sub(u_pow2(k), u_small(1)));
    check_vector(u_sub(r, u_pow2(k)));
  }
  const long edge = vectors;
  for (long i = 0; i < randoms; i++) {
    U x;
    for (int w = 0; w < 8; w += 2) {
      const uint64_t z = rnd();
      x.w[w] = (uint32_t)z;
      x.w[w + 1] = (uint32_t)(z >> 32);
    }
    // any 256-bit value as the field element (to_mont reduces it); below 2^261 as limbs it is normalized as it stands
    check_one(F::to_mont(fe_of(x)));
    if ((i & 7) == 0) check_one(plus_mod(F::unpack(fe_of(x)), (uint32_t)(i >> 3) % 8));
  }
  check_random(64, 3, false);
  check_random(256, 5, false);
  check_random(256, 0, true);
  check_random(512, 7, true);
  check_hints();
  printf("bad=%d edge=%ld vectors=%ld zeros=%ld neg_f=%ld rows=%ld inv_rows=%ld root_rows=%ld flagged=%ld jumps=%d\n", bad, edge,
         vectors, zeros, neg_f, rows_compared, inv_rows, root_rows, flagged_rows, ig29::kJumps);
  return bad ? 1 : 0;
}
