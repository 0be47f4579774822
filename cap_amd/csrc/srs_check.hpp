// Audit of a resident SRS (K15 of DESIGN.md §4): are the points [tau^i] g for the tau whose [tau] h the caller holds?
//
// The reference trusts its ceremony file by a SHA-256 over the bytes (load_srs, src/proof/mod.rs:95-102) and its key files
// not at all (load_data, src/parameters.rs:560-577); capgpu_srs_check asks the question itself.  With P[0 .. n) the
// resident points and (h, beta_h) the open key:
//   point pass  every P[i] is a point of y^2 = x^3 + 3 other than infinity (k_srs_points, below);
//   weights     r_i, i < n - 1: the first 16 bytes, little-endian, of Keccak-256(seed || le64(i)) - the block verifier's
//               byte convention (verify_front.hpp: vf::weight_bits; original 0x01 padding, the index as 8 little-endian
//               bytes behind the 32 seed bytes), here for EVERY i (the block verifier fixes r_0 = 1);
//   fold        A = sum_{i < n-1} r_i P[i],  B = sum_{i < n-1} r_i P[i + 1]: two MSMs over one weight array on the
//               resident table, at point offsets 0 and 1;
//   pairing     e(A, beta_h) e(-B, h) == 1, one wave-form check.
// Soundness.  P[i + 1] = tau P[i] for all i gives B = tau A: a consistent SRS is ALWAYS accepted (the identity is exact).
// With D_i = P[i + 1] - tau P[i] not all zero, the check passes iff sum r_i D_i = 0, which for weights drawn after the
// points were fixed has probability about 2^-128.  Hence seed == NULL draws the seed from the operating system; a seed
// the caller passes is for reproducibility and must not be known to whoever made the file.
// Not covered: the hiding powers (powers_of_gamma_g - host-side compressed bytes the prover never reads),
// neg_powers_of_h, whether P[0] is any particular generator, a sharded SRS, and the window tables beyond window 0
// (rows the library derives itself from window 0).
//
// The predicate is CAP_HD: tests/cpp/srs_check_host.cpp runs it on the host against field.hpp / curve.hpp.
#pragma once
#include "curve.hpp"
#include "field29.hpp"

namespace cap {
namespace sc {

constexpr uint32_t kFaultNone = 0, kFaultInfinity = 1, kFaultOffCurve = 2;
constexpr unsigned long long kNoIndex = ~0ull;  // the two result words before any lane has reported

// 3 in the internal form of the lazy field (3 * 2^261 mod p), limbs normalized
CAP_HD fl curve_b() {
  const fl one = Fq29::one();
  return Fq29::normalize(Fq29::add(Fq29::add(one, one), one));
}

// One resident base in the table's internal form (window 0 of MsmBases: x * 2^261 mod p as 8 words, any image below
// 2^256; (0, 0) = infinity): kFaultNone for a point of the curve other than infinity.  The comparison is field29.hpp's
// exact zero test on y^2 - (x^3 + 3).
CAP_HD uint32_t point_fault(const g1_affine& p) {
  using F = Fq29;
  if (G1::is_inf(p)) return kFaultInfinity;
  const fl x = F::load(p.x), y = F::load(p.y);
  const fl rhs = F::add_norm(F::mul(F::sqr(x), x), curve_b());
  return F::eq(F::sqr(y), rhs) ? kFaultNone : kFaultOffCurve;
}

#if defined(__HIPCC__)
constexpr int kPointThreads = 256;
// One lane per base.  out[0]: the lowest faulty index; out[1]: (that index << 2) | its kind - both by atomicMin from
// all-ones, so no order between lanes or workgroups is needed.
__global__ __launch_bounds__(kPointThreads) void k_srs_points(const g1_affine* __restrict__ ext, unsigned long long n,
                                                              unsigned long long* __restrict__ out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kPointThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t kind = point_fault(ext[i]);
  if (kind == kFaultNone) return;
  atomicMin(&out[0], i);
  atomicMin(&out[1], (i << 2) | kind);
}
#endif

}  // namespace sc
}  // namespace cap
