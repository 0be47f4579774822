// Signed window digits of a 256-bit scalar WITHOUT a carry chain over the windows (the variable-base MSM, msm.hip
// "one-shot MSM": window w of a scalar is its own sub-MSM, so a thread wants digit w alone).
//
// The usual recoding walks the windows from the bottom: a chunk above 2^(c-1) becomes chunk - 2^c and carries one into
// the next window, so digit w depends on every window below it.  Here the constant
//     B = sum_{w < W} 2^(c w + c - 1)
// is added to the scalar ONCE (a 9-limb addition), and
//     d_w = ((k + B) >> c w) mod 2^c  -  2^(c-1)          in [-2^(c-1), 2^(c-1) - 1]
// because  sum_w d_w 2^(c w) = (k + B) - B = k  as long as k + B < 2^(c W).  With W = msm_recode_windows(c) that holds
// for every k < 2^256: c W >= 258 for c = 2 .. 16 (c W = 256 is excluded by the extra window, c W = 257 has no divisor in
// range), and B < 2^(c W - 1) (1 + 2^-c + ...) < 0.51 * 2^(c W).
//
// Host and device: tests/cpp/msm_recode_check.cpp compiles this header with the host compiler under the
// unsigned-overflow sanitizer (no operation here wraps).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CAP_RECODE_HD __host__ __device__ __forceinline__
#else
#define CAP_RECODE_HD inline
#endif

namespace cap {

// windows of c bits that hold any 256-bit scalar in signed digits (one more when c divides 256: the top carry)
CAP_RECODE_HD uint32_t msm_recode_windows(uint32_t c) {
  uint32_t w = (256 + c - 1) / c;
  if (256 % c == 0) w += 1;
  return w;
}

// k + B: 288 bits (c W <= 272 for c >= 9; c W < 288 for every c in 2 .. 16), and one zero limb for the two-limb reads
struct msm_biased {
  uint32_t v[10];
};

// the constant B for window size c (2 .. 16), as 9 limbs (+ the zero guard limb)
CAP_RECODE_HD msm_biased msm_recode_bias(uint32_t c) {
  msm_biased b;
  for (int i = 0; i < 10; i++) b.v[i] = 0;
  const uint32_t windows = msm_recode_windows(c);
  for (uint32_t w = 0; w < windows; w++) {
    const uint32_t bit = c * w + c - 1;
    b.v[bit >> 5] |= 1u << (bit & 31);
  }
  return b;
}

// k (eight 32-bit limbs, any value) + bias
CAP_RECODE_HD msm_biased msm_recode_add(const uint32_t k[8], const msm_biased& bias) {
  msm_biased r;
  uint64_t carry = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 9; i++) {
    const uint64_t s = (uint64_t)(i < 8 ? k[i] : 0u) + bias.v[i] + carry;
    r.v[i] = (uint32_t)(s & 0xFFFFFFFFu);
    carry = s >> 32;
  }
  r.v[9] = 0;  // (carry is 0: k + B < 2^(c W) <= 2^288)
  return r;
}

// digit w of the biased scalar
CAP_RECODE_HD int32_t msm_recode_digit(const msm_biased& kb, uint32_t w, uint32_t c) {
  const uint32_t bit = w * c, limb = bit >> 5, off = bit & 31;
  const uint64_t two = (uint64_t)kb.v[limb] | ((uint64_t)kb.v[limb + 1] << 32);
  const uint32_t chunk = (uint32_t)(two >> off) & ((1u << c) - 1u);
  return (int32_t)chunk - (int32_t)(1u << (c - 1));
}

}  // namespace cap
