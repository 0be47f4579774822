// Host-side check of cap_amd/csrc/transcript_dev.hpp: everything the device transcript shares with the host (CAP_HD) runs
// here against keccak.hpp and host_util.hpp - the permutation in its lane form on 64 simulated lanes (LaneSim below, the
// stand-in for the wavefront's cross-lane moves), sponge framing and padding at every length 0..272, the fork into two
// digests, chained transcript challenges, the 48-byte reduction, the variable-time inversion, Jacobian -> affine,
// compression at its boundaries (y = 0, (p - 1)/2, (p + 1)/2, infinity) and the linearisation scalars.  Prints bad=0.
#include "../../cap_amd/csrc/transcript_dev.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cap_amd/csrc/host_util.hpp"
using namespace cap;

struct LaneSim {
  struct U64 {
    uint64_t l[64];
  };
  struct I32 {
    int l[64];
  };
  template <class F>
  static I32 idx(F f) {
    I32 r;
    for (int i = 0; i < 64; i++) r.l[i] = f(i & 31);
    return r;
  }
  template <class F>
  static U64 make(F f) {
    U64 r;
    for (int i = 0; i < 64; i++) r.l[i] = f(i & 31, i >> 5);
    return r;
  }
  static U64 shfl(const U64& v, const I32& src) {
    U64 r;
    for (int i = 0; i < 64; i++) r.l[i] = v.l[(i & 32) | (src.l[i] & 31)];
    return r;
  }
  static U64 rol(const U64& v, const I32& s) {
    U64 r;
    for (int i = 0; i < 64; i++) r.l[i] = s.l[i] ? (v.l[i] << s.l[i]) | (v.l[i] >> (64 - s.l[i])) : v.l[i];
    return r;
  }
  static U64 bxor(const U64& a, const U64& b) {
    U64 r;
    for (int i = 0; i < 64; i++) r.l[i] = a.l[i] ^ b.l[i];
    return r;
  }
  static U64 andn(const U64& a, const U64& b) {
    U64 r;
    for (int i = 0; i < 64; i++) r.l[i] = ~a.l[i] & b.l[i];
    return r;
  }
  template <class F>
  static void for_each(const U64& a, F f) {
    for (int i = 0; i < 64; i++) f(i & 31, i >> 5, a.l[i]);
  }
  static void sync() {}
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static fe rnd_raw() {
  fe r;
  for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)rnd64();
  return r;
}
template <class F>
static fe rnd_field() {  // Montgomery form of a random element
  fe r = rnd_raw();
  r.v[7] &= 0x0fffffffu;
  return F::to_mont(r);
}
static int bad = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      bad++;                              \
      if (bad < 20) printf(__VA_ARGS__);  \
    }                                     \
  } while (0)

int main() {
  td::KeccakTabs<LaneSim> tabs;
  tabs.init();
  // the permutation on lanes against keccak_f1600, both halves
  for (int it = 0; it < 50; it++) {
    uint64_t st[2][25];
    LaneSim::U64 a = LaneSim::make([](int, int) { return 0ull; });
    for (int h = 0; h < 2; h++)
      for (int i = 0; i < 25; i++) a.l[32 * h + i] = st[h][i] = it ? rnd64() : 0;
    td::keccak_f_lanes<LaneSim>(a, tabs);
    for (int h = 0; h < 2; h++) {
      keccak_f1600(st[h]);
      for (int i = 0; i < 25; i++) CHECK(a.l[32 * h + i] == st[h][i], "keccak-f lane %d half %d differs\n", i, h);
    }
  }
  // plain digests at every length 0..272 and a few long ones; the fork byte; three segments
  std::vector<uint8_t> msg(5000);
  for (auto& b : msg) b = (uint8_t)rnd64();
  std::vector<uint32_t> lens;
  for (uint32_t l = 0; l <= 273; l++) lens.push_back(l);
  for (uint32_t l : {407u, 408u, 2000u, 4096u, 4097u}) lens.push_back(l);
  for (uint32_t len : lens) {
    uint8_t want[64], got[64];
    keccak256(msg.data(), len, want);
    td::SpongeMsg m{nullptr, msg.data(), nullptr, 0, len, 0, 0};
    td::store_digest<LaneSim>(td::sponge_digest<LaneSim>(m, tabs), got, 1);
    CHECK(!memcmp(want, got, 32), "digest of %u bytes differs\n", len);
    // forked: H(msg || 0), H(msg || 1), with the message cut into three segments at random places
    std::vector<uint8_t> m0(msg.begin(), msg.begin() + len);
    m0.push_back(0);
    keccak256(m0.data(), m0.size(), want);
    m0.back() = 1;
    keccak256(m0.data(), m0.size(), want + 32);
    const uint32_t c1 = len ? (uint32_t)(rnd64() % (len + 1)) : 0, c2 = c1 + (uint32_t)(rnd64() % (len - c1 + 1));
    td::SpongeMsg mf{msg.data(), msg.data() + c1, msg.data() + c2, c1, c2 - c1, len - c2, 1};
    td::store_digest<LaneSim>(td::sponge_digest<LaneSim>(mf, tabs), got, 2);
    CHECK(!memcmp(want, got, 64), "forked digest of %u bytes differs\n", len);
  }
  // empty-message known answer
  {
    static const uint8_t kat[32] = {0xc5, 0xd2, 0x46, 0x01, 0x86, 0xf7, 0x23, 0x3c, 0x92, 0x7e, 0x7d, 0xb2, 0xdc, 0xc7, 0x03, 0xc0,
                                    0xe5, 0x00, 0xb6, 0x53, 0xca, 0x82, 0x27, 0x3b, 0x7b, 0xfa, 0xd8, 0x04, 0x5d, 0x85, 0xa4, 0x70};
    uint8_t got[32];
    td::SpongeMsg m{nullptr, nullptr, nullptr, 0, 0, 0, 0};
    td::store_digest<LaneSim>(td::sponge_digest<LaneSim>(m, tabs), got, 1);
    CHECK(!memcmp(kat, got, 32), "empty-message digest differs\n");
  }
  // chained transcript challenges against SolidityTranscript, prefixes of every residue mod 136, and the reduction
  for (uint32_t lpre = 0; lpre < 300; lpre += (lpre < 140 ? 1 : 23)) {
    SolidityTranscript t;
    t.append(msg.data(), lpre);
    uint8_t state[64] = {0};
    uint8_t app[td::kAppBytes];
    for (auto& b : app) b = (uint8_t)rnd64();
    const uint32_t steps[5] = {td::kAppZ, td::kAppZ, td::kAppQuot, td::kAppEvals, td::kAppBytes};
    uint32_t have = 0;
    for (int s = 0; s < 5; s++) {
      t.append(app + have, steps[s] - have);
      have = steps[s];
      uint8_t h[64];
      t.challenge_bytes(h);
      td::transcript_challenge<LaneSim>(state, msg.data(), lpre, app, have, tabs);
      CHECK(!memcmp(h, state, 64), "challenge %d with a prefix of %u bytes differs\n", s, lpre);
      CHECK(Fr::eq(challenge_to_fr(h), td::reduce48(state)), "reduction differs\n");
    }
  }
  for (int it = 0; it < 200; it++) {
    uint8_t h[64];
    for (auto& b : h) b = it < 2 ? (it ? 0xff : 0) : (uint8_t)rnd64();
    CHECK(Fr::eq(challenge_to_fr(h), td::reduce48(h)), "reduction of random bytes differs\n");
  }
  // the variable-time inversion against Fp::inv, both fields, edge values and non-canonical inputs
  for (int it = 0; it < 300; it++) {
    fe a = it < 6 ? Fq::zero() : rnd_raw();
    if (it == 1) a.v[0] = 1;
    if (it == 2) a = Fq::one();
    if (it == 3) (void)Fq::sub_raw(a, Fq::modulus(), Fq::one());
    if (it == 4) a = Fq::modulus();
    if (it == 5) a = Fr::modulus();
    if (it >= 6 && it % 3) a.v[7] &= 0x1fffffffu;
    // (a value above the modulus is brought below it first, as Fp::inv_host does; the Fermat chain wants a field element)
    fe aq = a, ar = a;
    for (int k = 0; k < 6 && Fq::geq_mod(aq); k++) (void)Fq::sub_mod_raw(aq, aq);
    for (int k = 0; k < 6 && Fr::geq_mod(ar); k++) (void)Fr::sub_mod_raw(ar, ar);
    CHECK(Fq::eq(td::inv_vartime32<FqP>(a), Fq::inv(aq)), "Fq inversion %d differs\n", it);
    CHECK(Fr::eq(td::inv_vartime32<FrP>(a), Fr::inv(ar)), "Fr inversion %d differs\n", it);
    CHECK(Fr::eq(td::inv_vartime32<FrP>(a), Fr::inv_fermat(ar)), "Fr inversion %d differs from the Fermat chain\n", it);
  }
  // Jacobian -> affine (any coordinates: the formulas never ask for a curve point) with points at infinity in between
  for (int it = 0; it < 100; it++) {
    const int count = 1 + it % 5;
    std::vector<g1_jac> in(count);
    std::vector<g1_affine> want;
    for (int i = 0; i < count; i++) {
      in[i].x = rnd_field<Fq>();
      in[i].y = rnd_field<Fq>();
      in[i].z = (rnd64() % 5 == 0) ? Fq::zero() : rnd_field<Fq>();
    }
    batch_to_affine(in, want);
    g1_affine got[5];
    td::to_affine(in.data(), count, got);
    for (int i = 0; i < count; i++) {
      CHECK(Fq::eq(want[i].x, got[i].x) && Fq::eq(want[i].y, got[i].y), "affine point %d of %d differs\n", i, count);
      uint8_t b0[32], b1[32];
      serialize_g1(want[i], b0);
      td::compress_g1(got[i], b1);
      CHECK(!memcmp(b0, b1, 32), "compressed point differs\n");
    }
  }
  // compression boundaries: y = 0 (x != 0), (p - 1)/2, (p + 1)/2, p - 1, 1, and infinity
  {
    fe half = Fq::modulus();  // (p - 1) / 2: p is odd
    for (int i = 0; i < 7; i++) half.v[i] = (half.v[i] >> 1) | (half.v[i + 1] << 31);
    half.v[7] >>= 1;
    fe half1 = half, one = Fq::zero(), pm1;
    one.v[0] = 1;
    (void)Fq::add_raw(half1, half, one);
    (void)Fq::sub_raw(pm1, Fq::modulus(), one);
    const fe ys[6] = {Fq::zero(), half, half1, pm1, one, rnd_raw()};
    int flagged = 0;
    for (int k = 0; k < 6; k++) {
      g1_affine p;
      p.x = rnd_field<Fq>();
      p.y = k < 5 ? Fq::to_mont(ys[k]) : rnd_field<Fq>();
      uint8_t b0[32], b1[32];
      serialize_g1(p, b0);
      td::compress_g1(p, b1);
      CHECK(!memcmp(b0, b1, 32), "compression boundary %d differs\n", k);
      flagged += (b1[31] & 0x80) != 0;
      if (k == 1) CHECK(!(b1[31] & 0x80), "y = (p - 1)/2 must not be flagged\n");
      if (k == 2) CHECK((b1[31] & 0x80) != 0, "y = (p + 1)/2 must be flagged\n");
      if (k == 0) CHECK(!(b1[31] & 0xc0), "y = 0 must carry no flag\n");
    }
    CHECK(flagged >= 2, "flags\n");
    g1_affine inf;
    inf.x = inf.y = Fq::zero();
    uint8_t b0[32], b1[32];
    serialize_g1(inf, b0);
    td::compress_g1(inf, b1);
    CHECK(!memcmp(b0, b1, 32) && b1[31] == 0x40, "infinity differs\n");
    fe e = rnd_field<Fr>();
    serialize_fr(e, b0);
    td::serialize_fr(e, b1);
    CHECK(!memcmp(b0, b1, 32), "serialised scalar differs\n");
  }
  // the linearisation scalars against the derivation as prove_batch wrote it out before the two modes shared it
  for (int it = 0; it < 40; it++) {
    td::LinIn in;
    for (auto& e : in.ev) e = rnd_field<Fr>();
    in.beta = rnd_field<Fr>();
    in.gamma = rnd_field<Fr>();
    in.alpha = rnd_field<Fr>();
    in.alpha2 = Fr::sqr(in.alpha);
    in.zeta = it == 0 ? Fr::one() : rnd_field<Fr>();  // zeta = 1: the inverse of zero is zero on both sides
    in.v = rnd_field<Fr>();
    for (int i = 0; i < 5; i++) in.k[i] = Fr::to_mont(fe_from_words(K_CANON[i]));
    in.n = (uint64_t)1 << (5 + it % 12);
    fe got[td::kLinScalars];
    td::lin_scalars(in, got);
    std::vector<fe> want;
    const fe *we = in.ev, *se = in.ev + 5;
    const size_t n = in.n;
    uint32_t e_n[8] = {(uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0, 0, 0, 0, 0, 0};
    fe zeta_n = Fr::pow(in.zeta, e_n);
    fe zh = Fr::sub(zeta_n, Fr::one());
    fe l1 = Fr::mul(zh, Fr::inv(Fr::mul(fr_from_u64((uint64_t)n), Fr::sub(in.zeta, Fr::one()))));
    for (int j = 0; j < 4; j++) want.push_back(we[j]);
    fe w01 = Fr::mul(we[0], we[1]), w23 = Fr::mul(we[2], we[3]);
    want.push_back(w01);
    want.push_back(w23);
    for (int j = 0; j < 4; j++) {
      fe w2 = Fr::sqr(we[j]);
      want.push_back(Fr::mul(Fr::sqr(w2), we[j]));
    }
    want.push_back(Fr::neg(we[4]));
    want.push_back(Fr::one());
    want.push_back(Fr::mul(Fr::mul(w01, w23), we[4]));
    fe bz = Fr::mul(in.beta, in.zeta);
    fe cz = in.alpha;
    for (int j = 0; j < 5; j++) cz = Fr::mul(cz, Fr::add(Fr::add(we[j], in.gamma), j == 0 ? bz : Fr::mul(in.k[j], bz)));
    want.push_back(Fr::add(cz, Fr::mul(in.alpha2, l1)));
    fe cs = Fr::mul(Fr::mul(in.alpha, in.beta), in.ev[9]);
    for (int j = 0; j < 4; j++) cs = Fr::mul(cs, Fr::add(Fr::add(we[j], in.gamma), Fr::mul(in.beta, se[j])));
    want.push_back(Fr::neg(cs));
    uint32_t e_n2[8] = {(uint32_t)(n + 2), (uint32_t)((uint64_t)(n + 2) >> 32), 0, 0, 0, 0, 0, 0};
    fe zp = Fr::pow(in.zeta, e_n2);
    fe cq = Fr::neg(zh);
    for (int j = 0; j < 5; j++) {
      want.push_back(cq);
      cq = Fr::mul(cq, zp);
    }
    fe cf = in.v;
    for (int j = 0; j < 9; j++) {
      want.push_back(cf);
      cf = Fr::mul(cf, in.v);
    }
    CHECK(want.size() == (size_t)td::kLinScalars, "term count\n");
    for (int i = 0; i < td::kLinScalars; i++) CHECK(Fr::eq(want[i], got[i]), "linearisation scalar %d differs\n", i);
    // zeta's bases
    fe b4[4];
    const fe omega = rnd_field<Fr>();
    td::zeta_bases(in.zeta, omega, b4);
    const fe zw = Fr::mul(in.zeta, omega);
    CHECK(Fr::eq(b4[0], in.zeta) && Fr::eq(b4[1], zw) && Fr::eq(b4[2], Fr::inv(in.zeta)) && Fr::eq(b4[3], Fr::inv(zw)),
          "zeta's bases differ\n");
  }
  printf("bad=%d\n", bad);
  return bad ? 1 : 0;
}
