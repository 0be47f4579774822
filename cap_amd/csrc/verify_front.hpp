// The verifier's front end on the device (K13 of DESIGN.md §4): what verify.hip's verifier_terms does on a host thread -
// input checks, the Fiat-Shamir transcript, the ~35 scalars of a proof's pairing inputs - done by one wavefront per proof
// (verify_dev.hip: k_verify_front), and the weights that fold a block of proofs into one pairing check.
//
// Replaces, for capgpu_plonk_verify_block_dev / _resident, the per-proof host work of `PlonkKzgSnark::batch_verify` as
// txn_batch_verify calls it (src/lib.rs:455-529).  Everything CAP_HD here also runs on the host:
// tests/cpp/verify_front_check.cpp compares it with verifier_terms, challenge by challenge and scalar by scalar.
//
// Term order of one proof (kTerms scalars, arkworks Montgomery form).  A = sum of the a-terms, B = sum of the others; the
// proof holds iff e(A, [tau]H) e(-B, H) == 1:
//    0      W_zeta            1                      a-terms
//    1      W_zeta_omega      u
//    2..6   wire commitments  v^(j+1)                b-terms on the proof's own points
//    7      z commitment      (alpha prod(..) + alpha^2 L1) + u     - verifier_terms has these as two terms
//    8..12  quotient parts    -Z_H zeta^(j (n+2))
//   13      W_zeta            zeta
//   14      W_zeta_omega      u zeta omega
//   15..27  selectors 0..12                          b-terms on the key's points
//   28..32  sigma 0..4        v^(6+j), j < 4;  -alpha beta z(zeta w) prod(..) for sigma 4
//   33      generator         -E
// The key terms of the proofs of one key share their points: a block's B side is 13 x count + 19 x keys points.
//
// Weights of a block of `count` proofs (the verifier's private choice; soundness 2^-128):
//   S   = Keccak-256(u_0 || ... || u_{count-1}), u_i as the transcript appends a field element (32 bytes, canonical,
//         little-endian), thirty-two zero bytes for a proof that failed its input checks;
//   r_0 = 1;  r_i = the first 16 bytes, little-endian, of Keccak-256(S || le64(i)) for i >= 1.
// Every r_i (i >= 1) depends on every u_j through S, and each u_j binds its statement and proof.  (verify.hip's host
// weights re-absorb the whole seed transcript per proof - quadratic in the block.)
#pragma once
#include "transcript_dev.hpp"

namespace cap {
namespace vf {

constexpr int kTerms = 34, kATerms = 2, kOwnTerms = 15, kKeyTerms = 19;  // kOwnTerms: a-terms and own b-terms
constexpr int kTermWzeta = 0, kTermWzetaW = 1, kTermWires = 2, kTermZ = 7, kTermQuot = 8, kTermBWzeta = 13,
              kTermBWzetaW = 14, kTermSel = 15, kTermSig = 28, kTermGen = 33;
// what the rounds append after the public inputs: td::kApp* for the commitments and evaluations, then the two openings
constexpr uint32_t kAppOpen = td::kAppBytes, kAppShifted = td::kAppBytes + 32, kAppBytes = td::kAppBytes + 64;
// the key's transcript prefix: 254, n, num_inputs (u64 LE each), k_i (5 x 32), 13 + 5 compressed commitments
constexpr uint32_t kPrefixBytes = 24 + 32 * 5 + 32 * 18;

// A verifying key as the device holds it (capgpu_plonk_vk_upload makes it once, on the host)
struct DevVk {
  fe k[5];       // coset representatives, Montgomery
  fe omega;      // generator of the domain, Montgomery
  fe n_mont;     // n as a field element
  uint64_t n;
  uint32_t num_inputs, pad;
  g1_affine pts[kKeyTerms];  // 13 selectors, 5 sigmas, the generator (arkworks form)
  uint8_t prefix[kPrefixBytes];
};

// omega_n = omega_28^(2^(28 - log n)): the generator verify.hip derives for a domain of n = 2^k <= 2^28 points (Montgomery)
CAP_HD fe domain_generator(uint64_t n) {
  const uint32_t root28[8] = {0x725b19f0u, 0x9bd61b6eu, 0x41112ed4u, 0x402d111eu,
                              0x8ef62abcu, 0x00e0a7ebu, 0xa58a7e85u, 0x2a3c09f0u};
  fe w;
  for (int i = 0; i < 8; i++) w.v[i] = root28[i];
  w = Fr::to_mont(w);
  for (uint64_t m = n; m < ((uint64_t)1 << 28); m <<= 1) w = Fr::sqr(w);
  return w;
}

CAP_HD bool g1_canonical(const g1_affine& p) { return !Fq::geq_mod(p.x) && !Fq::geq_mod(p.y); }
// canonical coordinates and on y^2 = x^3 + 3, or (0, 0)
CAP_HD bool g1_valid(const g1_affine& p) {
  if (!g1_canonical(p)) return false;
  if (G1::is_inf(p)) return true;
  const fe b3 = Fq::add(Fq::dbl(Fq::one()), Fq::one());
  return Fq::eq(Fq::sqr(p.y), Fq::add(Fq::mul(Fq::sqr(p.x), p.x), b3));
}

CAP_HD void prefix_bytes(const DevVk& vk, uint8_t out[kPrefixBytes]) {
  const uint64_t head[3] = {254, vk.n, vk.num_inputs};
  for (int w = 0; w < 3; w++)
    for (int b = 0; b < 8; b++) out[8 * w + b] = (uint8_t)(head[w] >> (8 * b));
  for (int i = 0; i < 5; i++) td::serialize_fr(vk.k[i], out + 24 + 32 * i);
  for (int i = 0; i < 18; i++) td::compress_g1(vk.pts[i], out + 184 + 32 * i);
}

// Z_H(zeta) = zeta^n - 1; false when zeta lies in the domain (the proof is rejected)
CAP_HD bool vanishing(const fe& zeta, uint64_t n, fe* zh) {
  *zh = Fr::sub(Fr::pow_u64(zeta, n), Fr::one());
  return !(Fr::is_zero(*zh) || Fr::eq(zeta, Fr::one()));
}
// lane `lane` of `lanes`: sum over j = lane, lane + lanes, ... < num_inputs of pub_j L_j(zeta),
// L_j(zeta) = Z_H w^j / (n (zeta - w^j)).  Public values: the inversion is the variable-time one.
CAP_HD fe pi_partial(const fe* pubs, uint32_t num_inputs, uint32_t lane, uint32_t lanes, const fe& zeta, const fe& zh,
                     const fe& omega, const fe& n_mont) {
  fe acc = Fr::zero();
  if (lane >= num_inputs) return acc;
  fe x = Fr::pow_u64(omega, lane);
  const fe step = Fr::pow_u64(omega, lanes);
  for (uint32_t j = lane; j < num_inputs; j += lanes) {
    const fe li = Fr::mul(Fr::mul(zh, x), td::fr_inv_public(Fr::mul(n_mont, Fr::sub(zeta, x))));
    acc = Fr::add(acc, Fr::mul(pubs[j], li));
    x = Fr::mul(x, step);
  }
  return acc;
}

struct FrontIn {
  const fe* ev;  // the proof's 10 evaluations: wires (5), sigmas (4), z(zeta omega)
  const fe* k;   // the key's 5 coset representatives
  fe beta, gamma, alpha, zeta, v, u, omega, n_mont, zh, pi;
  uint64_t n;
};
// the kTerms scalars of one proof, in the order above; `out` may be device memory (every index is a constant after
// unrolling: nothing is kept in an indexed local array)
CAP_HD void front_scalars(const FrontIn& in, fe* out) {
  const fe *we = in.ev, *se = in.ev + 5;
  const fe znext = in.ev[9], one = Fr::one();
  const fe alpha2 = Fr::sqr(in.alpha);
  const fe l1 = Fr::mul(in.zh, td::fr_inv_public(Fr::mul(in.n_mont, Fr::sub(in.zeta, one))));
  // r0 = PI(zeta) - alpha^2 L1(zeta) - alpha z(zeta w) (w4 + gamma) prod_{j<4} (w_j + beta sigma_j + gamma)
  fe prod = one;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 4; j++) prod = Fr::mul(prod, Fr::add(Fr::add(we[j], in.gamma), Fr::mul(in.beta, se[j])));
  const fe az = Fr::mul(in.alpha, znext);
  const fe r0 = Fr::sub(Fr::sub(in.pi, Fr::mul(alpha2, l1)), Fr::mul(Fr::mul(az, Fr::add(we[4], in.gamma)), prod));
  // selectors
  const fe w01 = Fr::mul(we[0], we[1]), w23 = Fr::mul(we[2], we[3]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 4; j++) {
    out[kTermSel + j] = we[j];
    const fe w2 = Fr::sqr(we[j]);
    out[kTermSel + 6 + j] = Fr::mul(Fr::sqr(w2), we[j]);
  }
  out[kTermSel + 4] = w01;
  out[kTermSel + 5] = w23;
  out[kTermSel + 10] = Fr::neg(we[4]);
  out[kTermSel + 11] = one;
  out[kTermSel + 12] = Fr::mul(Fr::mul(w01, w23), we[4]);
  // z's commitment: alpha prod(w_j + beta k_j zeta + gamma) + alpha^2 L1(zeta), and u from the batched opening
  const fe bz = Fr::mul(in.beta, in.zeta);
  fe cz = in.alpha;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 5; j++) cz = Fr::mul(cz, Fr::add(Fr::add(we[j], in.gamma), Fr::mul(in.k[j], bz)));
  out[kTermZ] = Fr::add(Fr::add(cz, Fr::mul(alpha2, l1)), in.u);
  out[kTermSig + 4] = Fr::neg(Fr::mul(Fr::mul(az, in.beta), prod));
  // quotient parts
  const fe zp = Fr::pow_u64(in.zeta, in.n + 2);
  fe cq = Fr::neg(in.zh);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 5; j++) {
    out[kTermQuot + j] = cq;
    cq = Fr::mul(cq, zp);
  }
  // batched openings: v^(j+1) on wires and sigmas, E = -r0 + sum v^(j+1) eval_j + u z(zeta w)
  fe e_acc = Fr::neg(r0), cf = in.v;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 9; j++) {
    out[j < 5 ? kTermWires + j : kTermSig + (j - 5)] = cf;
    e_acc = Fr::add(e_acc, Fr::mul(cf, in.ev[j]));
    cf = Fr::mul(cf, in.v);
  }
  e_acc = Fr::add(e_acc, Fr::mul(in.u, znext));
  out[kTermGen] = Fr::neg(e_acc);
  out[kTermWzeta] = one;
  out[kTermWzetaW] = in.u;
  out[kTermBWzeta] = in.zeta;
  out[kTermBWzetaW] = Fr::mul(Fr::mul(in.u, in.zeta), in.omega);
}

// ---- weights ----------------------------------------------------------------------------------------------------------
// S = Keccak-256(ub[0 .. 32 count)) to S (32 bytes); all lanes of X take part
template <class X>
CAP_HD void weight_seed(const uint8_t* ub, uint32_t count, const td::KeccakTabs<X>& tabs, uint8_t* S) {
  const td::SpongeMsg m{nullptr, ub, nullptr, 0, 32 * count, 0, 0};
  const typename X::U64 a = td::sponge_digest<X>(m, tabs);
  td::store_digest<X>(a, S, 1);
  X::sync();
}
// The first 16 bytes, little-endian, of Keccak-256(S || le64(i)) as a canonical integer below 2^128 - for every i, 0
// included (srs_check.hpp folds with these).  idx8: 8 bytes the caller owns, dig: 32; all lanes of X take part and return
// the same value
template <class X>
CAP_HD fe weight_bits(const uint8_t* S, uint64_t i, const td::KeccakTabs<X>& tabs, uint8_t* idx8, uint8_t* dig) {
  X::for_each(X::make([](int, int) { return 0ull; }), [idx8, i](int l, int half, uint64_t) {
    if (l < 8 && half == 0) idx8[l] = (uint8_t)(i >> (8 * l));
  });
  X::sync();
  const td::SpongeMsg m{S, idx8, nullptr, 32, 8, 0, 0};
  const typename X::U64 a = td::sponge_digest<X>(m, tabs);
  td::store_digest<X>(a, dig, 1);
  X::sync();
  fe r = Fr::zero();
  for (int w = 0; w < 4; w++)
    r.v[w] = (uint32_t)dig[4 * w] | ((uint32_t)dig[4 * w + 1] << 8) | ((uint32_t)dig[4 * w + 2] << 16) |
             ((uint32_t)dig[4 * w + 3] << 24);
  return r;
}
// r_i of the block verifier (Montgomery): 1 for i = 0, the hashed weight otherwise
template <class X>
CAP_HD fe weight(const uint8_t* S, uint64_t i, const td::KeccakTabs<X>& tabs, uint8_t* idx8, uint8_t* dig) {
  if (i == 0) return Fr::one();
  return Fr::to_mont(weight_bits<X>(S, i, tabs, idx8, dig));
}

}  // namespace vf
}  // namespace cap
