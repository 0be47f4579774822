// Witness check on the lazy 29-bit field: the TurboPlonk gate constraint at one row, and the index form of one value of
// the extended permutation.  Host + device, like curve29.hpp and pairing29.hpp: tests/cpp/gate_check.cpp builds this
// header for the host with field29.hpp's bound assertions on and compares with oracle/plonk.py.
//
// The reference runs `check_circuit_satisfiability` inside every prove() before it calls the SNARK
// (src/proof/transfer.rs:167-177; mint.rs and freeze.rs likewise); the kernels of check_kernels.hpp are that step.
//
// Gate (spec eq. (1); selector order q_lc x4, q_mul x2, q_hash x4, q_o, q_c, q_ecc):
//   q_c + PI + sum_i q_lc_i w_i + q_mul_0 w0 w1 + q_mul_1 w2 w3 + sum_i q_hash_i w_i^5 + q_ecc w0 w1 w2 w3 w4 - q_o w4
// All values in the internal Montgomery form (x * 2^261), normalized and below 2p - a table entry stored canonical, or
// what Fl::from_ext makes of a 32-byte value below 2^256.  23 products (six of them fused pairs with one reduction).
#pragma once
#include "field29.hpp"

namespace cap {
namespace wc29 {

constexpr int kWires = 5;
constexpr int kSelectors = 13;
constexpr int Q_LC = 0, Q_MUL = 4, Q_HASH = 6, Q_O = 10, Q_C = 11, Q_ECC = 12;
constexpr uint32_t kNoIndex = 0xffffffffu;

// constants of perm_index for one domain, internal form, canonical, packed: 1 / k_i and omega^(-2^b), b < log_n
struct PermConsts {
  fe kinv[kWires];
  fe winv[28];
  uint32_t log_n;
};

template <int SCHED = CAP_FL_SCHED>
struct Check {
  using F = Fl<FrP29, SCHED>;

  // The constraint's value (internal form, normalized, below 2^261): zero mod r iff the gate holds.
  // q(s): selector s of the row, fetched where it is used (a kernel that held all thirteen beside the five wires and the
  // partial terms ran out of registers); w: the five wire values.
  template <class Sel>
  static CAP_HD fl gate(Sel q, const fl* w, const fl& pi) {
    // every product is < 1.1 r and normalized; the running sum is carried after at most four addends (limbs < 2^31)
    fl acc = F::add(F::add(q(Q_C), pi), F::mul_add_mul(q(Q_LC), w[0], q(Q_LC + 1), w[1]));
    acc = F::normalize(F::add(acc, F::mul_add_mul(q(Q_LC + 2), w[2], q(Q_LC + 3), w[3])));
    {
      const fl w01 = F::mul(w[0], w[1]), w23 = F::mul(w[2], w[3]);
      acc = F::add(acc, F::mul_add_mul(q(Q_MUL), w01, q(Q_MUL + 1), w23));
      acc = F::normalize(F::add(acc, F::mul(q(Q_ECC), F::mul(F::mul(w01, w23), w[4]))));
    }
#pragma unroll 1
    for (int i = 0; i < 4; i += 2) {
      // (selected, not indexed: a run-time index would put the wires into scratch memory on the device)
      const fl wa = i ? w[2] : w[0], wb = i ? w[3] : w[1];
      const fl a5 = F::mul(F::sqr(F::sqr(wa)), wa), b5 = F::mul(F::sqr(F::sqr(wb)), wb);
      acc = F::add_norm(acc, F::mul_add_mul(q(Q_HASH + i), a5, q(Q_HASH + i + 1), b5));
    }
    return F::sub(acc, F::mul(q(Q_O), w[4]));  // < 8 * 1.1 r + 16 r
  }
  template <class Sel>
  static CAP_HD bool gate_holds(Sel q, const fl* w, const fl& pi) {
    return F::is_zero(gate(q, w, pi));
  }

  static CAP_HD bool is_one(const fl& a) { return F::is_zero(F::sub(a, F::one())); }

  // Index form of v = sigma_i(omega^j) = k_i' omega^j' (internal form): i' * 2^log_n + j', or kNoIndex when v lies in
  // none of the five cosets.  i' is the coset with (v / k_i')^n = 1; j' comes bit by bit from the 2^log_n subgroup
  // (Pohlig-Hellman: bit b of the exponent of t is set iff t^(2^(log_n - 1 - b)) = -1 once the bits below b are
  // cleared): 5 (log_n + 1) + log_n (log_n + 1) / 2 products.
  static CAP_HD uint32_t perm_index(const fl& v, const PermConsts& pc) {
    const uint32_t log_n = pc.log_n;
#pragma unroll 1
    for (uint32_t i = 0; i < (uint32_t)kWires; i++) {
      fl t = F::mul(v, F::load(pc.kinv[i]));
      fl u = t;
#pragma unroll 1
      for (uint32_t k = 0; k < log_n; k++) u = F::sqr(u);
      if (!is_one(u)) continue;
      uint32_t j = 0;
#pragma unroll 1
      for (uint32_t b = 0; b < log_n; b++) {
        u = t;
#pragma unroll 1
        for (uint32_t k = b + 1; k < log_n; k++) u = F::sqr(u);
        if (!is_one(u)) {
          j |= 1u << b;
          t = F::mul(t, F::load(pc.winv[b]));
        }
      }
      return (i << log_n) + j;
    }
    return kNoIndex;
  }

  // two 32-byte values (any integers below 2^256) equal mod r
  static CAP_HD bool same_value(const fe& a, const fe& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a.v[i] ^ b.v[i];
    if (d == 0) return true;
    return F::eq(F::load(a), F::load(b));
  }
};

}  // namespace wc29
}  // namespace cap
