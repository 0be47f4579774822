// Host-side check of cap_amd/csrc/verify_front.hpp: the CAP_HD parts of the device verifier's front end run here against
// the host verifier itself.  verify.hip is included as source, so that its verifier_terms - the function k_verify_front
// mirrors - is called directly: for proofs under two keys (0 and 4 public inputs) and ext_msg lengths around the sponge's
// 136-byte rate, the seven challenges (against SolidityTranscript in verifier_terms' order) and every scalar (against
// verifier_terms' terms) must be equal; then the weight rule.  The lanes are the 64 simulated ones of
// transcript_dev_check.cpp.  Prints bad=0.
#include "../../cap_amd/csrc/verify.hip"

#include <cstdio>
#include <set>
#include <string>

#include "../../cap_amd/csrc/verify_front.hpp"

// what verify.hip expects from the rest of the library: never reached here
namespace cap {
void set_error(const char*, ...) {}
int pairing_form() { return 0; }
int pairing_check2_wave_dev(const g1_affine&, const pairing::g2_affine&, const g1_affine&, const pairing::g2_affine&, int*) {
  return CAPGPU_ERR_NOT_INITIALISED;
}
}  // namespace cap
extern "C" {
int capgpu_device_info(char*, int*, uint64_t*) { return CAPGPU_ERR_NOT_INITIALISED; }
int capgpu_srs_upload(const void*, size_t, size_t, int, uint64_t*) { return CAPGPU_ERR_NOT_INITIALISED; }
int capgpu_msm_g1(uint64_t, size_t, const uint64_t*, size_t, uint64_t*) { return CAPGPU_ERR_NOT_INITIALISED; }
int capgpu_srs_free(uint64_t) { return CAPGPU_ERR_NOT_INITIALISED; }
}

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

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd64() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static fe rnd_fr() {  // Montgomery form of a random element
  fe r;
  for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)rnd64();
  r.v[7] &= 0x0fffffffu;
  return Fr::to_mont(r);
}
static g1_affine rnd_g1() {
  g1_affine gen;
  gen.x = Fq::one();
  gen.y = Fq::dbl(Fq::one());
  return G1::to_affine(g1_smul(gen, rnd_fr()));
}
static void put_g1(uint64_t w[8], const g1_affine& p) { affine_to_words(p, w); }
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
  const size_t msg_lens[6] = {0, 1, 135, 136, 137, 300};
  for (int key = 0; key < 2; key++) {
    capgpu_verifying_key vk;
    memset(&vk, 0, sizeof vk);
    vk.domain_size = key ? 256 : 128;
    vk.num_inputs = key ? 4 : 0;
    for (int i = 0; i < kNumWires; i++) fe_to_words(Fr::to_mont(fe_from_words(K_CANON[i])), vk.k[i]);
    for (int i = 0; i < kNumSelectors; i++) put_g1(vk.selector_comms[i], rnd_g1());
    for (int i = 0; i < kNumWires; i++) put_g1(vk.sigma_comms[i], rnd_g1());
    // the key as capgpu_plonk_vk_upload keeps it
    vf::DevVk dk;
    memset(&dk, 0, sizeof dk);
    for (int i = 0; i < 5; i++) dk.k[i] = fe_from_words(vk.k[i]);
    for (int i = 0; i < 18; i++) dk.pts[i] = g1_from_words(i < 13 ? vk.selector_comms[i] : vk.sigma_comms[i - 13]);
    dk.pts[18].x = Fq::one();
    dk.pts[18].y = Fq::dbl(Fq::one());
    dk.n = vk.domain_size;
    dk.num_inputs = (uint32_t)vk.num_inputs;
    dk.n_mont = fr_from_u64(dk.n);
    dk.omega = vf::domain_generator(dk.n);
    vf::prefix_bytes(dk, dk.prefix);
    for (int i = 0; i < 19; i++) CHECK(vf::g1_valid(dk.pts[i]) && g1_on_curve(dk.pts[i]), "key point %d\n", i);
    for (size_t mlen : msg_lens) {
      capgpu_proof pr;
      for (int i = 0; i < kNumWires; i++) {
        put_g1(pr.wires_poly_comms[i], rnd_g1());
        put_g1(pr.split_quot_poly_comms[i], rnd_g1());
        fe_to_words(rnd_fr(), pr.wires_evals[i]);
      }
      for (int i = 0; i < kNumWires - 1; i++) fe_to_words(rnd_fr(), pr.wire_sigma_evals[i]);
      fe_to_words(rnd_fr(), pr.perm_next_eval);
      put_g1(pr.prod_perm_poly_comm, rnd_g1());
      put_g1(pr.opening_proof, rnd_g1());
      put_g1(pr.shifted_opening_proof, rnd_g1());
      std::vector<uint64_t> pubs(4 * vk.num_inputs + 4);
      for (size_t i = 0; i < vk.num_inputs; i++) fe_to_words(rnd_fr(), &pubs[4 * i]);
      std::vector<uint8_t> msg(mlen + 1);
      for (auto& b : msg) b = (uint8_t)rnd64();

      ProofTerms pt;
      int valid = 0;
      int rc = verifier_terms(&vk, pubs.data(), vk.num_inputs, &pr, msg.data(), mlen, &pt, &valid);
      CHECK(rc == 0 && valid == 1 && pt.a.size() == 2 && pt.b.size() == 33, "host terms: rc %d valid %d\n", rc, valid);
      if (rc || !valid) continue;

      // ---- what k_verify_front does, on simulated lanes ----
      const uint8_t* prb = (const uint8_t*)&pr;
      std::vector<uint8_t> pre(mlen + vf::kPrefixBytes + 32 * vk.num_inputs), app(vf::kAppBytes);
      bool ok = true;
      for (uint32_t t = 0; t < 13; t++) {
        const g1_affine p = *(const g1_affine*)(prb + 64 * t);
        ok = ok && vf::g1_valid(p);
        td::compress_g1(p, &app[t < 11 ? 32 * t : 32 * (t + 10)]);
      }
      for (uint32_t t = 13; t < 23; t++) {
        const fe e = *(const fe*)(prb + td::kPrWireEvals + 32 * (t - 13));
        ok = ok && !Fr::geq_mod(e);
        td::serialize_fr(e, &app[td::kAppEvals + 32 * (t - 13)]);
      }
      std::vector<fe> pub_fe(vk.num_inputs + 1);
      for (size_t j = 0; j < vk.num_inputs; j++) {
        pub_fe[j] = fe_from_words(&pubs[4 * j]);
        ok = ok && !Fr::geq_mod(pub_fe[j]);
        td::serialize_fr(pub_fe[j], &pre[mlen + vf::kPrefixBytes + 32 * j]);
      }
      memcpy(pre.data(), msg.data(), mlen);
      memcpy(pre.data() + mlen, dk.prefix, vf::kPrefixBytes);
      CHECK(ok, "input checks\n");
      uint8_t st[64] = {0};
      auto draw = [&](uint32_t lapp) {
        td::transcript_challenge<LaneSim>(st, pre.data(), (uint32_t)pre.size(), app.data(), lapp, tabs);
        return td::reduce48(st);
      };
      fe ch[7];
      const uint32_t lapps[7] = {td::kAppZ, td::kAppZ, td::kAppZ, td::kAppQuot, td::kAppEvals, vf::kAppOpen, vf::kAppBytes};
      for (int k = 0; k < 7; k++) ch[k] = draw(lapps[k]);
      // the host transcript, in verifier_terms' order
      {
        SolidityTranscript t;
        if (mlen) t.append(msg.data(), mlen);
        t.append_u64_le(254);
        t.append_u64_le(vk.domain_size);
        t.append_u64_le(vk.num_inputs);
        for (int i = 0; i < kNumWires; i++) append_fr(t, fe_from_words(vk.k[i]));
        for (int i = 0; i < kNumSelectors; i++) append_g1(t, g1_from_words(vk.selector_comms[i]));
        for (int i = 0; i < kNumWires; i++) append_g1(t, g1_from_words(vk.sigma_comms[i]));
        for (size_t i = 0; i < vk.num_inputs; i++) append_fr(t, pub_fe[i]);
        for (int i = 0; i < kNumWires; i++) append_g1(t, g1_from_words(pr.wires_poly_comms[i]));
        fe want[7];
        want[0] = get_challenge(t);
        want[1] = get_challenge(t);
        want[2] = get_challenge(t);
        append_g1(t, g1_from_words(pr.prod_perm_poly_comm));
        want[3] = get_challenge(t);
        for (int i = 0; i < kNumWires; i++) append_g1(t, g1_from_words(pr.split_quot_poly_comms[i]));
        want[4] = get_challenge(t);
        for (int i = 0; i < kNumWires; i++) append_fr(t, fe_from_words(pr.wires_evals[i]));
        for (int i = 0; i < kNumWires - 1; i++) append_fr(t, fe_from_words(pr.wire_sigma_evals[i]));
        append_fr(t, fe_from_words(pr.perm_next_eval));
        want[5] = get_challenge(t);
        append_g1(t, g1_from_words(pr.opening_proof));
        append_g1(t, g1_from_words(pr.shifted_opening_proof));
        want[6] = get_challenge(t);
        for (int k = 0; k < 7; k++) CHECK(Fr::eq(want[k], ch[k]), "key %d msg %zu: challenge %d differs\n", key, mlen, k);
      }
      CHECK(Fr::eq(ch[6], pt.u), "u differs from verifier_terms'\n");
      fe zh;
      CHECK(vf::vanishing(ch[4], dk.n, &zh), "zeta in the domain\n");
      fe pi = Fr::zero();
      for (uint32_t lane = 0; lane < 64; lane++)
        pi = Fr::add(pi, vf::pi_partial(pub_fe.data(), dk.num_inputs, lane, 64, ch[4], zh, dk.omega, dk.n_mont));
      const vf::FrontIn in{(const fe*)(prb + td::kPrWireEvals), dk.k, ch[1], ch[2], ch[3], ch[4], ch[5], ch[6], dk.omega,
                           dk.n_mont, zh, pi, dk.n};
      fe got[vf::kTerms];
      vf::front_scalars(in, got);
      // verifier_terms' b-terms: 13 selectors, z, sigma 4, 5 quotient parts, 5 wires, sigma 0..3, z (u), W_zeta, W_zeta_w, G
      fe want[vf::kTerms];
      want[0] = pt.a[0].s;
      want[1] = pt.a[1].s;
      for (int j = 0; j < 5; j++) want[vf::kTermWires + j] = pt.b[20 + j].s;
      want[vf::kTermZ] = Fr::add(pt.b[13].s, pt.b[29].s);
      for (int j = 0; j < 5; j++) want[vf::kTermQuot + j] = pt.b[15 + j].s;
      want[vf::kTermBWzeta] = pt.b[30].s;
      want[vf::kTermBWzetaW] = pt.b[31].s;
      for (int j = 0; j < 13; j++) want[vf::kTermSel + j] = pt.b[j].s;
      for (int j = 0; j < 4; j++) want[vf::kTermSig + j] = pt.b[25 + j].s;
      want[vf::kTermSig + 4] = pt.b[14].s;
      want[vf::kTermGen] = pt.b[32].s;
      for (int k = 0; k < vf::kTerms; k++) CHECK(Fr::eq(want[k], got[k]), "key %d msg %zu: scalar %d differs\n", key, mlen, k);
      // ... and the points those scalars go with
      CHECK(!memcmp(&pt.b[13].p, &pt.b[29].p, sizeof(g1_affine)), "the two z terms share their point\n");
      for (int j = 0; j < 18; j++)
        CHECK(!memcmp(&dk.pts[j], &pt.b[j < 13 ? j : (j < 17 ? 25 + (j - 13) : 14)].p, sizeof(g1_affine)), "key point %d\n", j);
      CHECK(!memcmp(&dk.pts[18], &pt.b[32].p, sizeof(g1_affine)), "generator\n");
    }
  }
  // a malformed point or scalar is seen
  {
    g1_affine p = rnd_g1();
    CHECK(vf::g1_valid(p), "valid point\n");
    p.y.v[0] ^= 1;
    CHECK(!vf::g1_valid(p) && !g1_on_curve(p), "off-curve point\n");
    g1_affine q = rnd_g1();
    (void)Fq::add_raw(q.x, q.x, Fq::modulus());  // x + p: the same residue, not canonical (fits in 256 bits)
    CHECK(!vf::g1_valid(q) && !g1_on_curve(q), "non-canonical point\n");
    g1_affine inf;
    inf.x = inf.y = Fq::zero();
    CHECK(vf::g1_valid(inf), "infinity\n");
    fe zh;
    CHECK(!vf::vanishing(Fr::one(), 128, &zh) && !vf::vanishing(vf::domain_generator(128), 128, &zh), "zeta in the domain\n");
  }
  // ---- the weight rule ----
  for (uint32_t count : {1u, 2u, 5u, 64u, 65u}) {
    std::vector<uint8_t> ub(32 * count);
    for (uint32_t i = 0; i < count; i++) td::serialize_fr(rnd_fr(), &ub[32 * i]);
    auto weights = [&](const std::vector<uint8_t>& u) {
      uint8_t S[32], idx8[8], dig[32];
      vf::weight_seed<LaneSim>(u.data(), count, tabs, S);
      uint8_t ref[32];
      keccak256(u.data(), u.size(), ref);
      CHECK(!memcmp(S, ref, 32), "seed differs from Keccak-256 of the u bytes\n");
      std::vector<fe> r(count);
      for (uint32_t i = 0; i < count; i++) r[i] = vf::weight<LaneSim>(S, i, tabs, idx8, dig);
      return r;
    };
    const std::vector<fe> r = weights(ub);
    CHECK(Fr::eq(r[0], Fr::one()), "r_0 != 1\n");
    std::set<std::string> seen;
    for (uint32_t i = 0; i < count; i++) {
      const fe c = Fr::from_mont(r[i]);
      if (i) CHECK(!(c.v[4] | c.v[5] | c.v[6] | c.v[7]), "r_%u >= 2^128\n", i);
      seen.insert(std::string((const char*)c.v, 32));
      if (i) {  // the rule as the header states it, through keccak.hpp
        uint8_t S[32], m[40], d[32];
        keccak256(ub.data(), ub.size(), S);
        memcpy(m, S, 32);
        for (int b = 0; b < 8; b++) m[32 + b] = (uint8_t)((uint64_t)i >> (8 * b));
        keccak256(m, 40, d);
        CHECK(!memcmp(d, c.v, 16), "r_%u is not the first 16 bytes of Keccak-256(S || le64(i))\n", i);
      }
    }
    CHECK(seen.size() == count, "weights not pairwise distinct (count %u)\n", count);
    for (uint32_t j = 0; j < count; j++) {  // one u_j changed: every r_i, i >= 1, changes
      std::vector<uint8_t> ub2 = ub;
      ub2[32 * j + (j % 31)] ^= (uint8_t)(1u << (j % 8));
      const std::vector<fe> r2 = weights(ub2);
      CHECK(Fr::eq(r2[0], Fr::one()), "r_0 != 1\n");
      for (uint32_t i = 1; i < count; i++) CHECK(!Fr::eq(r[i], r2[i]), "r_%u unchanged by u_%u (count %u)\n", i, j, count);
    }
  }
  printf("bad=%d\n", bad);
  return bad ? 1 : 0;
}
