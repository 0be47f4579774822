// The prover's Fiat-Shamir transcript on the device (K10 of DESIGN.md §4): Keccak-256 with its state spread over the lanes
// of a wavefront, jf-plonk's SolidityTranscript on top of it, and the per-proof steps between the rounds of
// plonk.hip's prove_batch - Jacobian -> affine of a round's commitments, their compressed bytes, the challenges, zeta's
// tables and the linearisation scalars - so that a prove call is enqueued without a host wait between its rounds.
//
// Replaces `jf_plonk::transcript::SolidityTranscript` (imported at src/proof/transfer.rs:39-45; sha3 0.10.1 Keccak256
// underneath) where keccak.hpp / host_util.hpp replace it on the host.  The byte contract IS the host path's: a
// challenge hashes state(64) || everything appended so far || 0 and ... || 1, keeps the two digests as the new state and
// reduces the first 48 bytes little-endian mod r.  tests/cpp/transcript_dev_check.cpp runs everything CAP_HD in this file
// on the host - the lane form of the permutation on 64 simulated lanes - against keccak.hpp and host_util.hpp.
//
// Why the state is spread over lanes: one lane running Keccak-f alone executes ~4000 dependent instructions per block and
// a challenge re-absorbs the whole transcript (15-20 blocks).  With lane i = x + 5 y holding A[x][y], a round is 9
// cross-lane moves of 64 bits and a dozen ALU instructions.  Lanes 0..24 of each half of the wavefront carry one state:
// the halves run the same instructions, and differ only in the last message byte (jf-plonk's fork into two digests).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "curve.hpp"
#include "field29.hpp"
// CAP_TD_NO_KERNELS: a second translation unit (verify_dev.hip) takes the sponge and the lanes without the prover's kernels
#if defined(__HIPCC__) && !defined(CAP_TD_NO_KERNELS)
#include "plonk_kernels.hpp"
#endif

namespace cap {
namespace td {

// ---- sponge framing ----------------------------------------------------------------------------------------------------
// The message a sponge absorbs: up to three segments (the transcript's state, its prefix, what the rounds appended), then -
// for a transcript challenge - one byte that is 0 in the first half of the wavefront and 1 in the second.
struct SpongeMsg {
  const uint8_t *a, *b, *c;
  uint32_t la, lb, lc;
  uint32_t fork;  // 1: the fork byte follows the segments
};
constexpr uint32_t kRate = 136;
CAP_HD uint32_t sponge_len(const SpongeMsg& m) { return m.la + m.lb + m.lc + m.fork; }
CAP_HD uint32_t sponge_blocks(const SpongeMsg& m) { return sponge_len(m) / kRate + 1; }
// byte k of the padded message of `len` bytes that ends at `end` (original Keccak padding: 0x01 after the message, 0x80
// into the last block's last byte)
CAP_HD uint8_t sponge_byte(const SpongeMsg& m, uint32_t len, uint32_t end, uint32_t k, uint32_t half) {
  uint8_t v = 0;
  if (k < m.la) v = m.a[k];
  else if (k < m.la + m.lb) v = m.b[k - m.la];
  else if (k < m.la + m.lb + m.lc) v = m.c[k - m.la - m.lb];
  else if (k < len) v = (uint8_t)half;
  if (k == len) v ^= 0x01;
  if (k == end - 1) v ^= 0x80;
  return v;
}
// word w (little-endian) of the padded message.  A word that lies inside one segment at an 8-byte aligned address - all of
// the state and, with the prover's aligned prefix array, all of the prefix - is one load; the others go byte by byte.
CAP_HD uint64_t sponge_load8(const uint8_t* p) {
  if (((uintptr_t)p & 7) == 0) return *(const uint64_t*)p;
  uint64_t r = 0;
  for (int i = 7; i >= 0; i--) r = (r << 8) | p[i];
  return r;
}
CAP_HD uint64_t sponge_word(const SpongeMsg& m, uint32_t len, uint32_t end, uint32_t w, uint32_t half) {
  const uint32_t k = 8 * w, ab = m.la + m.lb, abc = ab + m.lc;
  if (k + 8 <= m.la) return sponge_load8(m.a + k);
  if (k >= m.la && k + 8 <= ab) return sponge_load8(m.b + (k - m.la));
  if (k >= ab && k + 8 <= abc) return sponge_load8(m.c + (k - ab));
  uint64_t r = 0;
  for (int i = 7; i >= 0; i--) r = (r << 8) | sponge_byte(m, len, end, k + (uint32_t)i, half);
  return r;
}

// ---- Keccak-f[1600] on lanes ----------------------------------------------------------------------------------------------
CAP_HD uint64_t keccak_rc(int rnd) {
  switch (rnd) {
    case 0: return 0x0000000000000001ULL;
    case 1: return 0x0000000000008082ULL;
    case 2: return 0x800000000000808AULL;
    case 3: return 0x8000000080008000ULL;
    case 4: return 0x000000000000808BULL;
    case 5: return 0x0000000080000001ULL;
    case 6: return 0x8000000080008081ULL;
    case 7: return 0x8000000000008009ULL;
    case 8: return 0x000000000000008AULL;
    case 9: return 0x0000000000000088ULL;
    case 10: return 0x0000000080008009ULL;
    case 11: return 0x000000008000000AULL;
    case 12: return 0x000000008000808BULL;
    case 13: return 0x800000000000008BULL;
    case 14: return 0x8000000000008089ULL;
    case 15: return 0x8000000000008003ULL;
    case 16: return 0x8000000000008002ULL;
    case 17: return 0x8000000000000080ULL;
    case 18: return 0x000000000000800AULL;
    case 19: return 0x800000008000000AULL;
    case 20: return 0x8000000080008081ULL;
    case 21: return 0x8000000000008080ULL;
    case 22: return 0x0000000080000001ULL;
    default: return 0x8000000080008008ULL;
  }
}
// rho offset of lane i = x + 5 y: the triangular numbers along the orbit of (1, 0) under (x, y) -> (y, 2x + 3y)
CAP_HD int keccak_rot(int i) {
  int x = 1, y = 0, r = 0;
  if (i == 0 || i >= 25) return 0;
  for (int t = 0; t < 24; t++) {
    r = (r + t + 1) & 63;
    if (x + 5 * y == i) return r;
    const int ny = (2 * x + 3 * y) % 5;
    x = y;
    y = ny;
  }
  return 0;
}
// pi sends lane x + 5 y to lane y + 5 ((2x + 3y) mod 5): the lane whose value lane j receives
CAP_HD int keccak_pi_src(int j) {
  for (int i = 0; i < 25; i++) {
    const int x = i % 5, y = i / 5;
    if (y + 5 * ((2 * x + 3 * y) % 5) == j) return i;
  }
  return j;  // lanes 25..31 hold nothing
}

// X: the lanes.  U64 / I32: one value per lane; make(f): lane (l, half) gets f(l, half), l = lane mod 32; idx(f): f(l);
// shfl(v, src): lane (l, half) gets lane (src, half)'s value; rol(v, r): rotate left by the lane's own r.
// LaneDev (below) is a wavefront, LaneSim (tests) 64 simulated lanes.
template <class X>
struct KeccakTabs {
  typename X::I32 up1, up2, up3, up4, xm1, xp1, xp2, pis, rot;
  CAP_HD void init() {
    up1 = X::idx([](int l) { return l < 25 ? (l + 5) % 25 : l; });
    up2 = X::idx([](int l) { return l < 25 ? (l + 10) % 25 : l; });
    up3 = X::idx([](int l) { return l < 25 ? (l + 15) % 25 : l; });
    up4 = X::idx([](int l) { return l < 25 ? (l + 20) % 25 : l; });
    xm1 = X::idx([](int l) { return l < 25 ? l / 5 * 5 + (l % 5 + 4) % 5 : l; });
    xp1 = X::idx([](int l) { return l < 25 ? l / 5 * 5 + (l % 5 + 1) % 5 : l; });
    xp2 = X::idx([](int l) { return l < 25 ? l / 5 * 5 + (l % 5 + 2) % 5 : l; });
    pis = X::idx([](int l) { return keccak_pi_src(l); });
    rot = X::idx([](int l) { return keccak_rot(l); });
  }
};
template <class X>
CAP_HD void keccak_f_lanes(typename X::U64& a, const KeccakTabs<X>& t) {
  using U = typename X::U64;
  const typename X::I32 one = X::idx([](int) { return 1; });
  for (int rnd = 0; rnd < 24; rnd++) {
    // theta: every lane of column x gets C[x], then D[x] = C[x - 1] ^ rol(C[x + 1], 1)
    U c = X::bxor(X::bxor(X::bxor(a, X::shfl(a, t.up1)), X::bxor(X::shfl(a, t.up2), X::shfl(a, t.up3))), X::shfl(a, t.up4));
    a = X::bxor(a, X::bxor(X::shfl(c, t.xm1), X::rol(X::shfl(c, t.xp1), one)));
    // rho at the source, pi as one move
    U b = X::shfl(X::rol(a, t.rot), t.pis);
    // chi, iota
    a = X::bxor(b, X::andn(X::shfl(b, t.xp1), X::shfl(b, t.xp2)));
    const uint64_t rc = keccak_rc(rnd);
    a = X::bxor(a, X::make([rc](int l, int) { return l == 0 ? rc : 0ull; }));
  }
}
// the sponge's state after the padded message: lanes 0..3 of half h hold digest h
template <class X>
CAP_HD typename X::U64 sponge_digest(const SpongeMsg& m, const KeccakTabs<X>& t) {
  typename X::U64 a = X::make([](int, int) { return 0ull; });
  const uint32_t nb = sponge_blocks(m), len = sponge_len(m), end = nb * kRate;
  for (uint32_t blk = 0; blk < nb; blk++) {
    a = X::bxor(a, X::make([&m, len, end, blk](int l, int half) {
                  return l < 17 ? sponge_word(m, len, end, blk * 17 + (uint32_t)l, (uint32_t)half) : 0ull;
                }));
    keccak_f_lanes<X>(a, t);
  }
  return a;
}
// `halves` digests of 32 bytes to out
template <class X>
CAP_HD void store_digest(const typename X::U64& a, uint8_t* out, int halves) {
  X::for_each(a, [out, halves](int l, int half, uint64_t v) {
    if (l < 4 && half < halves)
      for (int i = 0; i < 8; i++) out[32 * half + 8 * l + i] = (uint8_t)(v >> (8 * i));
  });
}
// SolidityTranscript::challenge_bytes: state <- H(state || pre || app || 0) || H(state || pre || app || 1)
template <class X>
CAP_HD void transcript_challenge(uint8_t* state, const uint8_t* pre, uint32_t lpre, const uint8_t* app, uint32_t lapp,
                                 const KeccakTabs<X>& t) {
  const SpongeMsg m{state, pre, app, 64, lpre, lapp, 1};
  const typename X::U64 a = sponge_digest<X>(m, t);
  X::sync();  // every lane has read the old state
  store_digest<X>(a, state, 2);
  X::sync();
}

// ---- field steps -----------------------------------------------------------------------------------------------------------
// from_le_bytes_mod_order over the first 48 bytes of a challenge (host_util.hpp: challenge_to_fr)
CAP_HD fe reduce48(const uint8_t* h) {
  fe lo, hi = Fr::zero();
  for (int i = 0; i < 8; i++)
    lo.v[i] = (uint32_t)h[4 * i] | ((uint32_t)h[4 * i + 1] << 8) | ((uint32_t)h[4 * i + 2] << 16) | ((uint32_t)h[4 * i + 3] << 24);
  for (int i = 0; i < 4; i++)
    hi.v[i] = (uint32_t)h[32 + 4 * i] | ((uint32_t)h[33 + 4 * i] << 8) | ((uint32_t)h[34 + 4 * i] << 16) |
              ((uint32_t)h[35 + 4 * i] << 24);
  return Fr::add(Fr::to_mont(lo), Fr::mul(Fr::to_mont(hi), Fr::r2()));
}
CAP_HD fe to_internal(const fe& a) { return Fr29::pack(Fr29::canonical(Fr29::from_ext(a))); }

// Inverse of a PUBLIC value (commitments, zeta): the binary extended Euclidean algorithm of Fp::inv_host on 32-bit limbs.
// Variable time - never for a value that depends on the witness (round 2's total keeps its fixed-length chain).  A lone
// lane needs ~0.17 ms for the 254 squarings of the Fermat chain; a proof has six such inversions between its rounds.
// Same value as Fp::inv (the inverse is unique, the result canonical); inv(0) = 0.
template <class PR>
CAP_HD fe inv_vartime32(const fe& a) {
  using F = Fp<PR>;
  fe u = a;
  for (int k = 0; k < 6 && F::geq_mod(u); k++) (void)F::sub_mod_raw(u, u);
  if (F::is_zero(u)) return F::zero();
  fe w = F::modulus(), x1 = F::zero(), x2 = F::zero();
  const fe p = F::modulus();
  x1.v[0] = 1;
  auto is_one = [](const fe& z) {
    uint32_t o = z.v[0] ^ 1u;
    for (int i = 1; i < 8; i++) o |= z.v[i];
    return o == 0;
  };
  auto shr1 = [](fe& z) {
    for (int i = 0; i < 7; i++) z.v[i] = (z.v[i] >> 1) | (z.v[i + 1] << 31);
    z.v[7] >>= 1;
  };
  auto halve_pair = [&](fe& z, fe& x) {  // z even: z /= 2, x /= 2 mod p (x < p < 2^254: x + p fits)
    while (!(z.v[0] & 1)) {
      shr1(z);
      if (x.v[0] & 1) (void)F::add_raw(x, x, p);
      shr1(x);
    }
  };
  while (!is_one(u) && !is_one(w)) {
    halve_pair(u, x1);
    halve_pair(w, x2);
    fe d;
    if (F::sub_raw(d, u, w) == 0) {  // u >= w
      u = d;
      if (F::sub_raw(x1, x1, x2)) (void)F::add_raw(x1, x1, p);
    } else {
      (void)F::sub_raw(w, w, u);
      if (F::sub_raw(x2, x2, x1)) (void)F::add_raw(x2, x2, p);
    }
  }
  const fe x = is_one(u) ? x1 : x2;  // (a R)^-1 as a plain integer; the Montgomery form of a^-1 is x R^2
  return F::to_mont(F::to_mont(x));
}
CAP_HD fe fr_inv_public(const fe& a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return inv_vartime32<FrP>(a);
#else
  return Fr::inv(a);
#endif
}

// `count` (<= 5) Jacobian points -> affine with ONE inversion (host_util.hpp: batch_to_affine); z = 0 -> (0, 0)
CAP_HD void to_affine(const g1_jac* in, int count, g1_affine* out) {
  fe pre[5];
  fe acc = Fq::one();
  for (int i = 0; i < count; i++) {
    pre[i] = acc;
    if (!Fq::is_zero(in[i].z)) acc = Fq::mul(acc, in[i].z);
  }
#if defined(__HIP_DEVICE_COMPILE__)
  fe inv = inv_vartime32<FqP>(acc);
#else
  fe inv = Fq::inv(acc);
#endif
  for (int i = count; i-- > 0;) {
    if (Fq::is_zero(in[i].z)) {
      out[i].x = Fq::zero();
      out[i].y = Fq::zero();
      continue;
    }
    const fe zi = Fq::mul(inv, pre[i]);
    inv = Fq::mul(inv, in[i].z);
    const fe zi2 = Fq::sqr(zi);
    out[i].x = Fq::mul(in[i].x, zi2);
    out[i].y = Fq::mul(in[i].y, Fq::mul(zi2, zi));
  }
}
CAP_HD void put_words(uint8_t* out, const fe& c) {
  for (int i = 0; i < 8; i++)
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(c.v[i] >> (8 * b));
}
// ark-serialize 0.3 compressed G1 (host_util.hpp: serialize_g1): canonical y against canonical -y
CAP_HD void compress_g1(const g1_affine& p, uint8_t out[32]) {
  if (G1::is_inf(p)) {
    for (int i = 0; i < 32; i++) out[i] = 0;
    out[31] |= 0x40;
    return;
  }
  const fe x = Fq::from_mont(p.x), y = Fq::from_mont(p.y), ny = Fq::from_mont(Fq::neg(p.y));
  put_words(out, x);
  bool larger = false;
  for (int i = 7; i >= 0; i--)
    if (y.v[i] != ny.v[i]) {
      larger = y.v[i] > ny.v[i];
      break;
    }
  if (larger) out[31] |= 0x80;
}
CAP_HD void serialize_fr(const fe& a_mont, uint8_t out[32]) { put_words(out, Fr::from_mont(a_mont)); }

// ---- round 5's linearisation scalars ------------------------------------------------------------------------------------
// The 29 scalars of k_lincomb's terms, in term order, arkworks form: the ONE derivation both transcript modes run
// (prove_batch on the host, k_tr_evals on the device).
constexpr int kLinScalars = 29;
struct LinIn {
  fe ev[10];  // wire evaluations (5), sigma evaluations (4), z(zeta omega)
  fe beta, gamma, alpha, alpha2, zeta, v;
  fe k[5];  // the coset representatives (Montgomery)
  uint64_t n;
};
CAP_HD void lin_scalars(const LinIn& in, fe out[kLinScalars]) {
  const fe *we = in.ev, *se = in.ev + 5;
  const fe znext = in.ev[9];
  fe nw = Fr::zero();
  nw.v[0] = (uint32_t)in.n;
  nw.v[1] = (uint32_t)(in.n >> 32);
  const fe n_mont = Fr::to_mont(nw);
  const fe zeta_n = Fr::pow_u64(in.zeta, in.n);
  const fe zh = Fr::sub(zeta_n, Fr::one());
  const fe l1 = Fr::mul(zh, fr_inv_public(Fr::mul(n_mont, Fr::sub(in.zeta, Fr::one()))));
  int t = 0;
  for (int j = 0; j < 4; j++) out[t++] = we[j];
  const fe w01 = Fr::mul(we[0], we[1]), w23 = Fr::mul(we[2], we[3]);
  out[t++] = w01;
  out[t++] = w23;
  for (int j = 0; j < 4; j++) {
    const fe w2 = Fr::sqr(we[j]);
    out[t++] = Fr::mul(Fr::sqr(w2), we[j]);
  }
  out[t++] = Fr::neg(we[4]);
  out[t++] = Fr::one();
  out[t++] = Fr::mul(Fr::mul(w01, w23), we[4]);
  // z(X): alpha * prod(w_i + beta k_i zeta + gamma) + alpha^2 L1(zeta)
  const fe bz = Fr::mul(in.beta, in.zeta);
  fe cz = in.alpha;
  for (int j = 0; j < 5; j++) cz = Fr::mul(cz, Fr::add(Fr::add(we[j], in.gamma), j == 0 ? bz : Fr::mul(in.k[j], bz)));
  out[t++] = Fr::add(cz, Fr::mul(in.alpha2, l1));
  // last sigma polynomial: - alpha beta z(zeta w) prod_{i<4}(w_i + beta sigma_i + gamma)
  fe cs = Fr::mul(Fr::mul(in.alpha, in.beta), znext);
  for (int j = 0; j < 4; j++) cs = Fr::mul(cs, Fr::add(Fr::add(we[j], in.gamma), Fr::mul(in.beta, se[j])));
  out[t++] = Fr::neg(cs);
  // quotient part: - Z_H(zeta) * zeta^(i (n + 2))
  const fe zp = Fr::pow_u64(in.zeta, in.n + 2);
  fe cq = Fr::neg(zh);
  for (int j = 0; j < 5; j++) {
    out[t++] = cq;
    cq = Fr::mul(cq, zp);
  }
  // batched opening at zeta: v^(j + 1)
  fe cf = in.v;
  for (int j = 0; j < 9; j++) {
    out[t++] = cf;
    cf = Fr::mul(cf, in.v);
  }
}
// zeta's four bases - zeta, zeta omega and their inverses from one inversion - as round 4's squarings table wants them
CAP_HD void zeta_bases(const fe& zeta, const fe& omega, fe bases[4]) {
  const fe zw = Fr::mul(zeta, omega);
  const fe zi = fr_inv_public(Fr::mul(zeta, zw));  // 1/z = zw * zi, 1/zw = z * zi
  bases[0] = zeta;
  bases[1] = zw;
  bases[2] = Fr::mul(zw, zi);
  bases[3] = Fr::mul(zeta, zi);
}

// what the rounds append after the prefix, per proof: 5 + 1 + 5 commitments, then 10 evaluations
constexpr uint32_t kAppWires = 0, kAppZ = 160, kAppQuot = 192, kAppEvals = 352, kAppBytes = 672;
// byte offsets of capgpu_proof's members (include/capgpu.h; static_asserts in plonk.hip)
constexpr uint32_t kPrWires = 0, kPrZ = 320, kPrQuot = 384, kPrOpen = 704, kPrShifted = 768, kPrWireEvals = 832,
                   kPrSigmaEvals = 992, kPrNext = 1120, kPrBytes = 1152;

#if defined(__HIPCC__)
// ---- the lanes of a wavefront ----------------------------------------------------------------------------------------------
struct LaneDev {
  using U64 = uint64_t;
  using I32 = int;
  template <class F>
  static __device__ __forceinline__ I32 idx(F f) { return f((int)(threadIdx.x & 31)); }
  template <class F>
  static __device__ __forceinline__ U64 make(F f) { return f((int)(threadIdx.x & 31), (int)((threadIdx.x >> 5) & 1)); }
  static __device__ __forceinline__ U64 shfl(U64 v, I32 src) {  // the state's lanes travel as two 32-bit halves
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 32), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 32);
    return ((uint64_t)hi << 32) | lo;
  }
  static __device__ __forceinline__ U64 rol(U64 v, I32 r) { return r ? (v << r) | (v >> (64 - r)) : v; }
  static __device__ __forceinline__ U64 bxor(U64 a, U64 b) { return a ^ b; }
  static __device__ __forceinline__ U64 andn(U64 a, U64 b) { return ~a & b; }
  template <class F>
  static __device__ __forceinline__ void for_each(U64 a, F f) { f((int)(threadIdx.x & 31), (int)((threadIdx.x >> 5) & 1), a); }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
};

#if !defined(CAP_TD_NO_KERNELS)
// the transcript of `count` proofs on the device
struct TrBufs {
  uint8_t* state;           // [count][64]
  const uint8_t* pre;       // [count][pre_stride]: init message || vk_bytes || public inputs
  const uint32_t* pre_len;  // [count]
  uint8_t* app;             // [count][kAppBytes]
  uint32_t pre_stride;
};
__device__ __forceinline__ void store_fe(uint8_t* dst, const fe& a) {  // dst is 16-byte aligned
  *(fe*)dst = a;
}
// draws one challenge with the whole wavefront; every lane returns it
__device__ __forceinline__ fe draw(const TrBufs& t, uint32_t p, uint32_t lapp, const KeccakTabs<LaneDev>& tabs) {
  uint8_t* st = t.state + (size_t)p * 64;
  transcript_challenge<LaneDev>(st, t.pre + (size_t)p * t.pre_stride, t.pre_len[p], t.app + (size_t)p * kAppBytes, lapp, tabs);
  return reduce48(st);
}

// digests[i] = Keccak-256(data[offsets[i] .. offsets[i + 1])): one wavefront per message
__global__ __launch_bounds__(64) void k_keccak_batch(const uint8_t* __restrict__ data, const uint64_t* __restrict__ offsets,
                                                     uint32_t count, uint8_t* __restrict__ digests) {
  const uint32_t i = blockIdx.x;
  if (i >= count) return;
  KeccakTabs<LaneDev> tabs;
  tabs.init();
  const SpongeMsg m{nullptr, data + offsets[i], nullptr, 0, (uint32_t)(offsets[i + 1] - offsets[i]), 0, 0};
  const uint64_t a = sponge_digest<LaneDev>(m, tabs);
  store_digest<LaneDev>(a, digests + (size_t)i * 32, 1);
}

// Rounds 1-3, one wavefront per proof: the round's NPTS commitments (comms[p NPTS ..]) to affine - into the proof struct and,
// compressed, into the transcript - then the round's challenges.
//   ROUND 1: tau (drawn and discarded), beta, gamma;  2: alpha;  3: zeta and the 4 x 24 squarings table pw.
// chal / chal29: the challenges in arkworks' and in the internal form.
template <int ROUND>
__global__ __launch_bounds__(64) void k_tr_comms(TrBufs t, const g1_jac* __restrict__ comms, uint8_t* __restrict__ proofs,
                                                 pk::Chal* __restrict__ chal, pk::Chal* __restrict__ chal29,
                                                 fe* __restrict__ zeta_out, fe* __restrict__ pw, fe omega, uint32_t count) {
  constexpr int NPTS = ROUND == 2 ? 1 : 5;
  constexpr uint32_t app_off = ROUND == 1 ? kAppWires : (ROUND == 2 ? kAppZ : kAppQuot);
  constexpr uint32_t pr_off = ROUND == 1 ? kPrWires : (ROUND == 2 ? kPrZ : kPrQuot);
  __shared__ fe sh[4];
  const uint32_t p = blockIdx.x;
  if (p >= count) return;
  if (threadIdx.x == 0) {
    g1_jac in[NPTS];
    g1_affine out[NPTS];
    for (int i = 0; i < NPTS; i++) in[i] = comms[(size_t)p * NPTS + i];
    to_affine(in, NPTS, out);
    for (int i = 0; i < NPTS; i++) {
      uint8_t* pr = proofs + (size_t)p * kPrBytes + pr_off + 64 * i;
      store_fe(pr, out[i].x);
      store_fe(pr + 32, out[i].y);
      compress_g1(out[i], t.app + (size_t)p * kAppBytes + app_off + 32 * i);
    }
  }
  __syncthreads();
  KeccakTabs<LaneDev> tabs;
  tabs.init();
  constexpr uint32_t lapp = app_off + 32 * NPTS;
  if (ROUND == 1) {
    (void)draw(t, p, lapp, tabs);  // plookup's tau: drawn by jf-plonk even when the circuit has no lookups
    const fe beta = draw(t, p, lapp, tabs), gamma = draw(t, p, lapp, tabs);
    if (threadIdx.x == 0) {
      chal[p].beta = beta;
      chal[p].gamma = gamma;
      chal[p].alpha = Fr::zero();
      chal[p].alpha2 = Fr::zero();
      const fe beta_inv = fr_inv_public(beta);  // beta is public; inv(0) = 0: k_quotient then takes the direct form
      chal[p].beta_inv = beta_inv;
      chal[p].alpha_beta5 = Fr::zero();
      chal29[p].beta = to_internal(beta);
      chal29[p].gamma = to_internal(gamma);
      chal29[p].alpha = Fr::zero();
      chal29[p].alpha2 = Fr::zero();
      chal29[p].beta_inv = to_internal(beta_inv);
      chal29[p].alpha_beta5 = Fr::zero();
    }
  } else if (ROUND == 2) {
    const fe alpha = draw(t, p, lapp, tabs);
    if (threadIdx.x == 0) {
      const fe a2 = Fr::sqr(alpha);
      chal[p].alpha = alpha;
      chal[p].alpha2 = a2;
      chal29[p].alpha = to_internal(alpha);
      chal29[p].alpha2 = to_internal(a2);
      const fe beta = chal[p].beta, b2 = Fr::sqr(beta);
      const fe ab5 = Fr::mul(alpha, Fr::mul(Fr::sqr(b2), beta));
      chal[p].alpha_beta5 = ab5;
      chal29[p].alpha_beta5 = to_internal(ab5);
    }
  } else {
    const fe zeta = draw(t, p, lapp, tabs);
    if (threadIdx.x == 0) {
      zeta_out[p] = zeta;
      fe b4[4];
      zeta_bases(zeta, omega, b4);
      for (int q = 0; q < 4; q++) sh[q] = b4[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      fe x = sh[threadIdx.x];
      for (int b = 0; b < 24; b++) {
        pw[((size_t)p * 4 + threadIdx.x) * 24 + b] = x;
        x = Fr::sqr(x);
      }
    }
  }
}

// Round 4's end, one wavefront per proof: the ten evaluations into the proof struct and the transcript, v drawn, the 29
// scalars of k_lincomb's terms (internal form) written beside the `poly` and `len` the host uploaded with the call.
__global__ __launch_bounds__(64) void k_tr_evals(TrBufs t, const fe* __restrict__ evals, uint8_t* __restrict__ proofs,
                                                 const pk::Chal* __restrict__ chal, const fe* __restrict__ zeta,
                                                 pk::LinTerm* __restrict__ terms, LinIn base, uint32_t count) {
  const uint32_t p = blockIdx.x;
  if (p >= count) return;
  if (threadIdx.x < 10) {
    const fe e = evals[(size_t)p * 10 + threadIdx.x];
    store_fe(proofs + (size_t)p * kPrBytes + kPrWireEvals + 32 * threadIdx.x, e);  // the three members are contiguous
    serialize_fr(e, t.app + (size_t)p * kAppBytes + kAppEvals + 32 * threadIdx.x);
  }
  __syncthreads();
  KeccakTabs<LaneDev> tabs;
  tabs.init();
  const fe v = draw(t, p, kAppBytes, tabs);
  if (threadIdx.x == 0) {
    LinIn in = base;  // k and n
    for (int i = 0; i < 10; i++) in.ev[i] = evals[(size_t)p * 10 + i];
    in.beta = chal[p].beta;
    in.gamma = chal[p].gamma;
    in.alpha = chal[p].alpha;
    in.alpha2 = chal[p].alpha2;
    in.zeta = zeta[p];
    in.v = v;
    fe sc[kLinScalars];
    lin_scalars(in, sc);
    for (int i = 0; i < kLinScalars; i++) terms[(size_t)p * kLinScalars + i].scalar = to_internal(sc[i]);
  }
}

// Round 5's end: the two opening proofs to affine, into the proof struct
__global__ __launch_bounds__(64) void k_tr_open(const g1_jac* __restrict__ comms, uint8_t* __restrict__ proofs, uint32_t count) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  g1_jac in[2] = {comms[(size_t)p * 2], comms[(size_t)p * 2 + 1]};
  g1_affine out[2];
  to_affine(in, 2, out);
  uint8_t* pr = proofs + (size_t)p * kPrBytes + kPrOpen;
  store_fe(pr, out[0].x);
  store_fe(pr + 32, out[0].y);
  store_fe(pr + 64, out[1].x);
  store_fe(pr + 96, out[1].y);
}
#endif  // CAP_TD_NO_KERNELS
#endif  // __HIPCC__

}  // namespace td
}  // namespace cap
