// The wire format of a proof, host and device (K14 of DESIGN.md §4): the 769 ark-serialize bytes a TransferNote / MintNote /
// FreezeNote carries (src/transfer.rs:54-66) <-> capgpu_proof.  The decode rule IS capgpu_proof_deserialize's
// (params.hip), the encode rule capgpu_proof_serialize's (verify.hip); here they are written once per field kind as
// CAP_HD code, so that proof_codec.hip runs them one lane per field and tests/cpp/proof_codec_check.cpp runs the same
// functions on the host against params.hpp's g1_decompress_host and the bound on Fr.
//
// Record layout (byte offsets; every Vec carries a u64 little-endian length):
//     0  u64 = 5      8 + 32 k  wire commitments (k < 5)      168  permutation product
//   200  u64 = 5    208 + 32 k  quotient parts (k < 5)        368  opening      400  shifted opening
//   432  u64 = 5    440 + 32 k  wire evaluations (k < 5)
//   600  u64 = 4    608 + 32 k  sigma evaluations (k < 4)     736  next evaluation
//   768  Option tag of the plookup proof, must be 0
// A point: x little-endian, bit 7 of byte 31 = "y is the larger root", bit 6 = infinity.  Both bits: invalid.  Infinity is
// valid only with x = 0 and decodes to (0, 0).  Otherwise x < p, x^3 + 3 a square, and the flag picks the root.
// A scalar: valid when < r; stored as Montgomery words.
// Status of a record: 0 when valid, else 1 + the offset of the first offending field in the order above - the field the
// host reader stops at.  The fields lie in the record in that order, so the first one is the one at the lowest offset.
// A record whose status is not 0 decodes to a struct of all-ones words: every coordinate and evaluation is then
// non-canonical and k_verify_front / vf::g1_valid reject it by their own checks.
// Records sit at any byte address: every word is assembled from bytes.
#pragma once
#include <string.h>

#include "../../include/capgpu.h"
#include "transcript_dev.hpp"

namespace cap {
namespace pc {

constexpr uint32_t kBytes = CAPGPU_PROOF_BYTES, kPoints = 13, kScalars = 10, kHeads = 4, kTagOffset = 768;
constexpr uint32_t kStatusUnset = 0xFFFFFFFFu;  // the status word before any lane has reported
static_assert(sizeof(capgpu_proof) == td::kPrBytes, "capgpu_proof layout");

// point k of the struct (its 13 points are contiguous, 64 bytes each) in the record
CAP_HD uint32_t point_offset(uint32_t k) {
  if (k < 5) return 8 + 32 * k;
  if (k == 5) return 168;
  if (k < 11) return 208 + 32 * (k - 6);
  return k == 11 ? 368 : 400;
}
// evaluation k of the struct (its 10 evaluations are contiguous behind the points, 32 bytes each) in the record
CAP_HD uint32_t scalar_offset(uint32_t k) {
  if (k < 5) return 440 + 32 * k;
  if (k < 9) return 608 + 32 * (k - 5);
  return 736;
}
CAP_HD uint32_t head_offset(uint32_t k) { return k == 0 ? 0 : (k == 1 ? 200 : (k == 2 ? 432 : 600)); }
CAP_HD uint64_t head_value(uint32_t k) { return k == 3 ? 4 : 5; }

CAP_HD fe load_le(const uint8_t* b) {
  fe r;
  for (int i = 0; i < 8; i++)
    r.v[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
  return r;
}
CAP_HD uint64_t load_u64(const uint8_t* b) {
  uint64_t r = 0;
  for (int i = 7; i >= 0; i--) r = (r << 8) | b[i];
  return r;
}
CAP_HD void store_u64(uint8_t* b, uint64_t v) {
  for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * i));
}

// (p + 1) / 4, the square-root exponent for p = 3 mod 4 (params.hpp: fq_sqrt_exponent); a kernel takes it as an argument
struct SqrtExp {
  uint32_t w[8];
};
CAP_HD SqrtExp sqrt_exponent() {
  uint32_t m[8];
  uint64_t c = 1;
  for (int i = 0; i < 8; i++) {
    c += FqP::MOD[i];
    m[i] = (uint32_t)c;
    c >>= 32;
  }
  SqrtExp e;
  for (int i = 0; i < 8; i++) e.w[i] = (m[i] >> 2) | (i < 7 ? m[i + 1] << 30 : 0);
  return e;
}

// a > b as 256-bit integers
CAP_HD bool greater(const fe& a, const fe& b) {
  bool r = false;
  for (int i = 0; i < 8; i++)
    if (a.v[i] != b.v[i]) r = a.v[i] > b.v[i];  // the most significant difference is seen last
  return r;
}

// 32 bytes -> an affine point in arkworks' form; false (and (0, 0)) on every encoding ark-serialize rejects.  The power
// (p + 1) / 4 runs on the 9 x 29-bit field with an exponent every lane shares, as g1_decompress_kernel's does.
CAP_HD bool decode_point(const uint8_t* b, const SqrtExp& e, g1_affine* out) {
  using F = Fq29;
  fe x = load_le(b);
  const uint32_t flags = x.v[7] >> 30;  // bit 31 = 0x80 of the last byte (larger root), bit 30 = 0x40 (infinity)
  x.v[7] &= 0x3fffffffu;
  out->x = Fq::zero();
  out->y = Fq::zero();
  if (flags == 3) return false;
  if (flags == 1) return Fq::is_zero(x);
  if (Fq::geq_mod(x)) return false;
  const fl xi = F::to_mont(x);
  fe three = Fq::zero();
  three.v[0] = 3;
  const fl rhs = F::add_norm(F::mul(F::sqr(xi), xi), F::to_mont(three));
  fl y = F::one();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int bit = 253; bit >= 0; bit--) {
    y = F::sqr(y);
    if ((e.w[bit >> 5] >> (bit & 31)) & 1) y = F::mul(y, rhs);
  }
  if (!F::eq(F::sqr(y), rhs)) return false;
  const fe yc = F::from_mont(y);
  fe nyc;
  (void)Fq::sub_raw(nyc, Fq::modulus(), yc);  // y = 0 does not occur on y^2 = x^3 + 3 over this field
  if (greater(yc, nyc) != (flags == 2)) y = F::neg(y);
  out->x = F::to_ext(xi);
  out->y = F::to_ext(y);
  return true;
}
// 32 bytes -> an evaluation in Montgomery form; false for a value >= r
CAP_HD bool decode_scalar(const uint8_t* b, fe* out) {
  const fe v = load_le(b);
  *out = Fr::to_mont(v);
  return !Fr::geq_mod(v);
}
// the four length prefixes and the tag: kStatusUnset when they are what a TurboPlonk proof has, else 1 + the offset of the
// first that is not
CAP_HD uint32_t frame_status(const uint8_t* rec) {
  for (uint32_t k = 0; k < kHeads; k++)
    if (load_u64(rec + head_offset(k)) != head_value(k)) return 1 + head_offset(k);
  return rec[kTagOffset] != 0 ? 1 + kTagOffset : kStatusUnset;
}

CAP_HD void poison(capgpu_proof* out) {
  uint64_t* w = (uint64_t*)out;
  for (uint32_t i = 0; i < td::kPrBytes / 8; i++) w[i] = ~0ull;
}
// One record, field after field: the whole rule on one thread (the host's form; proof_codec.hip spreads the same
// functions over lanes and takes the minimum).  Returns the status.
CAP_HD uint32_t decode_record(const uint8_t* rec, const SqrtExp& e, capgpu_proof* out) {
  uint32_t st = frame_status(rec);
  uint8_t* o = (uint8_t*)out;
  for (uint32_t k = 0; k < kPoints; k++) {
    g1_affine p;
    const bool ok = decode_point(rec + point_offset(k), e, &p);
    memcpy(o + 64 * k, &p, 64);
    if (!ok && 1 + point_offset(k) < st) st = 1 + point_offset(k);
  }
  for (uint32_t k = 0; k < kScalars; k++) {
    fe v;
    const bool ok = decode_scalar(rec + scalar_offset(k), &v);
    memcpy(o + td::kPrWireEvals + 32 * k, &v, 32);
    if (!ok && 1 + scalar_offset(k) < st) st = 1 + scalar_offset(k);
  }
  if (st == kStatusUnset) return 0;
  poison(out);
  return st;
}

// ---- struct -> record: the inverse on canonical structs (capgpu_proof_serialize's bytes) ---------------------------------
CAP_HD void encode_frame(uint8_t* rec) {
  for (uint32_t k = 0; k < kHeads; k++) store_u64(rec + head_offset(k), head_value(k));
  rec[kTagOffset] = 0;  // Option::None for the plookup proof
}
CAP_HD void encode_record(const capgpu_proof& in, uint8_t* rec) {
  const uint8_t* s = (const uint8_t*)&in;
  encode_frame(rec);
  for (uint32_t k = 0; k < kPoints; k++) {
    g1_affine p;
    memcpy(&p, s + 64 * k, 64);
    td::compress_g1(p, rec + point_offset(k));
  }
  for (uint32_t k = 0; k < kScalars; k++) {
    fe v;
    memcpy(&v, s + td::kPrWireEvals + 32 * k, 32);
    td::serialize_fr(v, rec + scalar_offset(k));
  }
}

#if defined(__HIPCC__)
// proof_codec.hip.  `count` records at d_bytes + i * stride (any byte address, stride >= kBytes) -> d_proofs[i] and
// d_status[i], enqueued on s; count >= 1.  CAPGPU_OK or the launch error.
int decode_launch(const uint8_t* d_bytes, size_t stride, size_t count, void* d_proofs, int* d_status, hipStream_t s);
int encode_launch(const void* d_proofs, size_t count, uint8_t* d_bytes, size_t stride, hipStream_t s);
#endif

}  // namespace pc
}  // namespace cap
