// capgpu_proof.hpp - C++17 host-side mirror of the reference's proof API above the C ABI of capgpu.h.
//
// The reference is compiled code (Rust); where its toolchain is missing this header is what a caller links instead of
// src/proof/: the same module layout, names, argument meaning and error behaviour -
//
//   capgpu::proof::universal_setup            src/proof/mod.rs:59-69
//   capgpu::proof::load_srs                   src/proof/mod.rs:74-109   (the bytes of data/aztec-crs-131072.bin - an
//                                             ark-serialized UniversalSrs, src/proof/mod.rs:106 - handed in by the caller:
//                                             the reference embeds them with include_bytes!, its tree does not ship them)
//   capgpu::proof::universal_setup_for_staging src/proof/mod.rs:121-141  (bn254: an alias of load_srs, rng ignored)
//   capgpu::proof::{transfer,mint,freeze}::preprocess   src/proof/transfer.rs:124-155, mint.rs:69-93, freeze.rs:93-121
//   capgpu::proof::{transfer,mint,freeze}::prove        src/proof/transfer.rs:159-188, mint.rs:97-120, freeze.rs:125-158
//   capgpu::proof::{transfer,mint,freeze}::verify       src/proof/transfer.rs:192-212, mint.rs:124-140, freeze.rs:162-178
//   capgpu::TransferProvingKey / ...VerifyingKey         src/proof/transfer.rs:55-108 (key + note shape)
//   capgpu::TxnApiError::FailedSnark                     src/errors.rs:25-63: what every SNARK failure maps to
//   capgpu::Result<T>                                    Rust's Result<T, TxnApiError>: is_ok / is_err / unwrap / error
//
// What differs, and why: the circuit builders (src/circuit/*.rs) stay on the CPU and are out of scope,
// so `preprocess` takes the finalised circuit they produce (selector columns + extended permutation) next to the note
// shape, and `prove` takes the finalised wire assignment + public-input scalars instead of Witness / PublicInput
// structs.  The random number generator argument of `prove` is any callable returning one Fr (Montgomery words): it is
// asked for the 13 blinders in jf-plonk's order.  Everything heavy runs in libcapgpu.so on the GPU; there is no CPU path
// and a missing device surfaces as Err(FailedSnark("... no CPU fallback ...")).
//
// Header only; link with -lcapgpu.  tests/cpp/proof_api_test.cpp is the reference's test_*_validity_proof restated on it.
#ifndef CAPGPU_PROOF_HPP
#define CAPGPU_PROOF_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "capgpu.h"

namespace capgpu {

using Fr = std::array<uint64_t, 4>;  // arkworks' in-memory form: 4 x u64, little-endian limbs, Montgomery (R = 2^256)

// src/errors.rs:25-63 - only the variants this path produces
struct TxnApiError {
  enum Kind { FailedSnark, InvalidParameter, FailedSerialization } kind;
  std::string msg;
  static TxnApiError failed_snark(std::string m) { return {FailedSnark, std::move(m)}; }
  std::string to_string() const {
    const char* k = kind == FailedSnark ? "FailedSnark" : (kind == InvalidParameter ? "InvalidParameter" : "FailedSerialization");
    return std::string(k) + "(" + msg + ")";
  }
};

struct Unit {};  // Rust's ()

template <class T>
class Result {
 public:
  Result(T v) : v_(std::move(v)) {}
  Result(TxnApiError e) : v_(std::move(e)) {}
  bool is_ok() const { return v_.index() == 0; }
  bool is_err() const { return !is_ok(); }
  T& unwrap() {
    if (is_err()) throw std::runtime_error("called unwrap() on Err: " + error().to_string());
    return std::get<0>(v_);
  }
  const TxnApiError& error() const { return std::get<1>(v_); }

 private:
  std::variant<T, TxnApiError> v_;
};

namespace detail {
inline std::string lib_error(int rc) {
  const char* m = capgpu_last_error();
  return "capgpu error " + std::to_string(rc) + (m && *m ? std::string(": ") + m : std::string());
}
inline TxnApiError map_error(int rc, const std::string& what) {
  // ark_serialize::SerializationError -> TxnApiError::FailedSerialization (src/errors.rs), everything else in the SNARK
  // calls -> FailedSnark (src/proof/transfer.rs:187)
  if (rc == CAPGPU_ERR_SERIALIZATION) return {TxnApiError::FailedSerialization, what + ": " + lib_error(rc)};
  return TxnApiError::failed_snark(what + ": " + lib_error(rc));
}
struct SrsHandle {
  uint64_t h = 0;
  explicit SrsHandle(uint64_t v) : h(v) {}
  SrsHandle(const SrsHandle&) = delete;
  SrsHandle& operator=(const SrsHandle&) = delete;
  ~SrsHandle() {
    if (h) capgpu_srs_free(h);
  }
};
struct KeyHandle {
  uint64_t h = 0;
  explicit KeyHandle(uint64_t v) : h(v) {}
  KeyHandle(const KeyHandle&) = delete;
  KeyHandle& operator=(const KeyHandle&) = delete;
  ~KeyHandle() {
    if (h) capgpu_plonk_free_key(h);
  }
};
}  // namespace detail

// jf-plonk's UniversalSrs: powers of tau in G1 (device resident) + the G2 part of the open key
struct UniversalSrs {
  std::shared_ptr<detail::SrsHandle> powers_of_g;
  size_t max_degree = 0;
  std::array<uint64_t, 16> h{}, beta_h{};
  uint64_t handle() const { return powers_of_g ? powers_of_g->h : 0; }
};

// jf-plonk's VerifyingKey (+ open key); plain data, host only
struct VerifyingKey {
  capgpu_verifying_key raw{};
  std::array<uint64_t, 16> h{}, beta_h{};
};

// jf-plonk's ProvingKey: selector / sigma polynomials and the commit key, resident on the device; `vk` as in the crate
struct ProvingKey {
  std::shared_ptr<detail::KeyHandle> key;
  UniversalSrs srs;  // keeps the commit key alive
  VerifyingKey vk;
  uint64_t handle() const { return key ? key->h : 0; }
  size_t domain_size() const { return (size_t)vk.raw.domain_size; }
  size_t num_inputs() const { return (size_t)vk.raw.num_inputs; }
};

// jf-plonk's Proof<Bn254> (13 G1 + 10 Fr), in the C ABI's field order
using Proof = capgpu_proof;

// The finalised circuit the reference's builders hand to jf-plonk (PlonkCircuit after finalize_for_arithmetization):
// column-major Montgomery field elements.  Out of scope to build here; tests and benches use a synthetic satisfiable one.
struct FinalisedCircuit {
  size_t domain_size = 0;            // n, a power of two (Arithmetization::eval_domain_size)
  size_t num_inputs = 0;             // public inputs (the first gates)
  const uint64_t* selectors = nullptr;  // 13 x n x 4 words, gate order of capgpu.h
  const uint64_t* sigma = nullptr;      // 5 x n x 4 words: the extended permutation as field elements
  size_t num_gates = 0;              // constraints before padding (preprocess returns it, transfer.rs:155)
  // CAPGPU_INPUT_EVALS: the columns are tables of values on the domain; CAPGPU_INPUT_COEFFS: they are the polynomials
  // jf-relation's Arithmetization trait returns (compute_selector_polynomials / compute_extended_permutation_polynomials),
  // n coefficients each, passed through untransformed
  int input_form = CAPGPU_INPUT_EVALS;
  // Key generation from the circuit's wire -> variable table (PlonkCircuit::wire_variables[..5], 5 x n ids below
  // num_vars, column-major) instead of `sigma`: the permutation is built on the device and the key keeps the table, so
  // that prove() takes a VariableAssignment.  `input_form` is then the selectors' form alone.
  const uint32_t* wire_vars = nullptr;
  size_t num_vars = 0;
};
struct Assignment {
  const uint64_t* wires = nullptr;       // 5 x n x 4 words
  const uint64_t* pub_inputs = nullptr;  // num_inputs x 4 words  (PublicInput::to_scalars())
  int input_form = CAPGPU_INPUT_EVALS;   // CAPGPU_INPUT_COEFFS: wires = compute_wire_polynomials(), unblinded
};
// What a jf-relation PlonkCircuit holds after witness generation: one value per variable (`witness: Vec<F>`,
// CAPGPU_INPUT_VARS).  For keys preprocessed from a FinalisedCircuit with wire_vars (or given the table by
// capgpu_plonk_key_set_vars); the five columns are gathered on the device.
struct VariableAssignment {
  const uint64_t* values = nullptr;      // num_vars x 4 words
  const uint64_t* pub_inputs = nullptr;  // num_inputs x 4 words
  Assignment as_assignment() const { return Assignment{values, pub_inputs, CAPGPU_INPUT_VARS}; }
};

namespace proof {

// src/proof/mod.rs:59-69.  The reference samples tau from its rng (benches: test_rng); here the caller passes it
// (canonical words) - the SRS is generated on the device.
// `gamma`, when given, also produces the hiding powers [gamma tau^i] G, i <= max_degree + 1, that KZG10::setup samples
// next to tau: they travel with stored parameter files and keys; the prover does not use them.
inline Result<UniversalSrs> universal_setup(size_t max_degree, const Fr& tau, const Fr* gamma = nullptr) {
  int rc = capgpu_init(nullptr, 0);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Failed to generate universal SRS");
  uint64_t h = 0;
  rc = gamma ? capgpu_srs_generate_hiding(tau.data(), gamma->data(), max_degree + 1, &h)
             : capgpu_srs_generate(tau.data(), max_degree + 1, &h);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Failed to generate universal SRS");
  UniversalSrs s;
  s.powers_of_g = std::make_shared<detail::SrsHandle>(h);
  s.max_degree = max_degree;
  capgpu_g2_generator(s.h.data());
  capgpu_g2_mul(s.h.data(), tau.data(), s.beta_h.data());
  return s;
}

// SHA-256 (FIPS 180-4) of a byte string: load_srs checks the integrity of the CRS file like the reference does
// (sha2::Sha256, src/proof/mod.rs:95-102).  Host only, ~1 GB/s: the 4 MB file is 4 ms.
inline std::array<uint8_t, 32> sha256(const uint8_t* data, size_t len) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
      0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
      0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
      0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
      0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  auto block = [&](const uint8_t* p) {
    uint32_t w[64];
    for (int i = 0; i < 16; i++)
      w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
  };
  size_t i = 0;
  for (; i + 64 <= len; i += 64) block(data + i);
  uint8_t tail[128] = {0};
  const size_t rem = len - i;
  std::memcpy(tail, data + i, rem);
  tail[rem] = 0x80;
  const size_t tl = rem < 56 ? 64 : 128;
  const uint64_t bits = (uint64_t)len * 8;
  for (int k = 0; k < 8; k++) tail[tl - 1 - k] = (uint8_t)(bits >> (8 * k));
  block(tail);
  if (tl == 128) block(tail + 64);
  std::array<uint8_t, 32> out;
  for (int k = 0; k < 8; k++)
    for (int b2 = 0; b2 < 4; b2++) out[4 * k + b2] = (uint8_t)(h[k] >> (24 - 8 * b2));
  return out;
}

// SHA-256 of data/aztec-crs-131072.bin as pinned by the reference (src/proof/mod.rs:100)
inline const std::array<uint8_t, 32>& aztec_crs_sha256() {
  static const std::array<uint8_t, 32> d = {0x6b, 0x81, 0xe7, 0x5f, 0xb9, 0xc1, 0x4f, 0xd0, 0xe5, 0x8f, 0xb2,
                                            0xb2, 0x9e, 0x48, 0x97, 0x8c, 0xda, 0xd5, 0x51, 0x15, 0x03, 0x68,
                                            0x5a, 0x61, 0xf1, 0x39, 0x1d, 0xc4, 0xa4, 0xfc, 0x7c, 0xbf};
  return d;
}

// src/proof/mod.rs:74-109.  `bytes`: the CRS file the reference embeds (an ark-serialized UniversalSrs).  As there:
//   - max_degree > 2^17 is refused with the reference's message (mod.rs:83-88);
//   - the SHA-256 of the bytes must equal `expected_sha256` - the reference's pinned digest unless the caller states
//     another one (a test SRS) - or the call PANICS like the reference's assert_eq! (mod.rs:96-102): std::runtime_error;
//   - the WHOLE file is deserialized and returned; max_degree plays no other role (mod.rs:106).
// check = true (no counterpart in the reference, which stops at the digest): the loaded powers are audited on the device
// against the blob's own open key (capgpu_srs_check, seed from the OS); a faulty point or powers that are no sequence
// [tau^i] g under beta_h give Err(FailedSnark) naming the fault.  The default leaves loading as it was.
inline Result<UniversalSrs> load_srs(size_t max_degree, const std::vector<uint8_t>& bytes,
                                     const std::array<uint8_t, 32>& expected_sha256 = aztec_crs_sha256(),
                                     bool check = false) {
  if (max_degree > ((size_t)1 << 17))
    return TxnApiError::failed_snark("Currently only supports 2^17. Please update Aztec's CRS data file if needed.");
  if (sha256(bytes.data(), bytes.size()) != expected_sha256)
    throw std::runtime_error("Mismatched sha256sum digest, file might be corrupted!");
  int rc = capgpu_init(nullptr, 0);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Failed to load SRS");
  UniversalSrs s;
  uint64_t h = 0;
  size_t used = 0, n = 0;
  rc = capgpu_srs_deserialize(bytes.data(), bytes.size(), 0, &h, s.h.data(), s.beta_h.data(), &used);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Failed to load SRS");
  s.powers_of_g = std::make_shared<detail::SrsHandle>(h);
  if (check) {
    capgpu_srs_report rep;
    rc = capgpu_srs_check(h, s.h.data(), s.beta_h.data(), nullptr, CAPGPU_SRS_CHECK_LOCATE, &rep);
    if (rc != CAPGPU_OK) return detail::map_error(rc, "Failed to load SRS");
    if (rep.verdict == 1)
      return TxnApiError::failed_snark("Failed to load SRS: point " + std::to_string(rep.first_bad_point) +
                                       (rep.point_fault == 1 ? " is the point at infinity" : " is not on the curve"));
    if (rep.verdict == 2)
      return TxnApiError::failed_snark("Failed to load SRS: not a power sequence under the open key; first bad link: " +
                                       std::to_string(rep.first_bad_link));
  }
  capgpu_srs_size(h, &n);
  s.max_degree = n ? n - 1 : 0;
  return s;
}

// src/proof/mod.rs:121-141: "a unified API for SRS generation for testing/staging" - under the reference's default
// feature (bn254, the one this library implements) it IGNORES its rng and loads Aztec's CRS: a one-line alias of
// load_srs.  The rng parameter is kept (any type, unused) so that call sites read like the reference's.
template <class Rng>
inline Result<UniversalSrs> universal_setup_for_staging(size_t max_degree, Rng& /*rng*/, const std::vector<uint8_t>& crs_bytes,
                                                        const std::array<uint8_t, 32>& expected_sha256 = aztec_crs_sha256()) {
  return load_srs(max_degree, crs_bytes, expected_sha256);
}

namespace detail_snark {
inline Result<std::pair<ProvingKey, VerifyingKey>> preprocess(const UniversalSrs& srs, const FinalisedCircuit& c,
                                                              const std::string& what) {
  if (!c.selectors || (!c.sigma && !c.wire_vars)) return TxnApiError::failed_snark(what + ": circuit not finalised");
  ProvingKey pk;
  uint64_t h = 0;
  int rc = c.wire_vars ? capgpu_plonk_preprocess_vars(srs.handle(), c.domain_size, c.num_inputs, c.selectors, c.input_form,
                                                      c.wire_vars, c.num_vars, &h, &pk.vk.raw)
                       : capgpu_plonk_preprocess_ex(srs.handle(), c.domain_size, c.num_inputs, c.selectors, c.sigma,
                                                    c.input_form, &h, &pk.vk.raw);
  if (rc != CAPGPU_OK) return detail::map_error(rc, what);
  pk.key = std::make_shared<detail::KeyHandle>(h);
  pk.srs = srs;
  pk.vk.h = srs.h;
  pk.vk.beta_h = srs.beta_h;
  VerifyingKey vk = pk.vk;
  return std::make_pair(std::move(pk), vk);
}
template <class Rng>
Result<Proof> prove(Rng& rng, const ProvingKey& pk, const Assignment& a, const std::vector<uint8_t>* ext_msg,
                    const std::string& what) {
  if (!a.wires || (!a.pub_inputs && pk.num_inputs())) return TxnApiError::failed_snark(what + ": empty assignment");
  std::array<uint64_t, 13 * 4> blinders;  // 2 per wire polynomial, 3 for the permutation product (jf-plonk's order)
  for (int i = 0; i < 13; i++) {
    Fr b = rng();
    std::memcpy(&blinders[4 * i], b.data(), 32);
  }
  Proof p;
  int rc = capgpu_plonk_prove_ex(pk.handle(), a.wires, a.pub_inputs, pk.num_inputs(),
                                 ext_msg ? ext_msg->data() : nullptr, ext_msg ? ext_msg->size() : 0, blinders.data(),
                                 a.input_form, &p);
  if (rc != CAPGPU_OK) return detail::map_error(rc, what);
  return p;
}
inline Result<Unit> verify(const VerifyingKey& vk, const std::vector<Fr>& pub_inputs, const Proof& proof,
                           const std::vector<uint8_t>* ext_msg, const std::string& what) {
  int ok = 0;
  int rc = capgpu_plonk_verify(&vk.raw, vk.h.data(), vk.beta_h.data(),
                               pub_inputs.empty() ? nullptr : pub_inputs[0].data(), pub_inputs.size(), &proof,
                               ext_msg ? ext_msg->data() : nullptr, ext_msg ? ext_msg->size() : 0, &ok);
  if (rc != CAPGPU_OK) return detail::map_error(rc, what);
  if (!ok) return TxnApiError::failed_snark(what + ": WrongProof");
  return Unit{};
}
// ext_msg = CanonicalSerialize(ver_key) || extra_proof_bound_data (src/proof/transfer.rs:177-180); the caller passes
// the 32 serialised bytes of the Schnorr verification key (the embedded-curve point, out of scope to compute here)
inline std::vector<uint8_t> bound_message(const std::vector<uint8_t>& ver_key_bytes,
                                          const std::vector<uint8_t>& extra_proof_bound_data) {
  std::vector<uint8_t> m(ver_key_bytes);
  m.insert(m.end(), extra_proof_bound_data.begin(), extra_proof_bound_data.end());
  return m;
}
}  // namespace detail_snark

// Opt-in counterpart of the `check_circuit_satisfiability` call the reference makes inside prove() (src/proof/
// transfer.rs:167-177, mint.rs, freeze.rs): Ok when the assignment satisfies the key's circuit, else Err(FailedSnark)
// naming the first failing gate or copy constraint ("gate 1234 not satisfied", "copy constraint (2,40) -> (0,7)
// violated").  Runs on the device (capgpu_plonk_check_witness); prove() itself does not call it - a caller who wants the
// reference's order calls this first, or switches the check on for every prove call with capgpu_plonk_set_precheck(1).
inline Result<Unit> check_satisfiability(const ProvingKey& pk, const Assignment& a) {
  if (!a.wires || (!a.pub_inputs && pk.num_inputs())) return TxnApiError::failed_snark("check_satisfiability: empty assignment");
  capgpu_witness_fault f;
  int rc = capgpu_plonk_check_witness(pk.handle(), a.wires, a.pub_inputs, pk.num_inputs(), a.input_form, &f);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "check_satisfiability");
  if (f.kind == 1) return TxnApiError::failed_snark("gate " + std::to_string(f.row) + " not satisfied");
  if (f.kind == 2)
    return TxnApiError::failed_snark("copy constraint (" + std::to_string(f.wire) + "," + std::to_string(f.row) + ") -> (" +
                                     std::to_string(f.wire2) + "," + std::to_string(f.row2) + ") violated");
  return Unit{};
}

// A batch of proofs being made by a worker thread of the library (capgpu_plonk_prove_batch_async).  The handle OWNS the
// blinders and the output array; the witnesses and public inputs stay the caller's and must outlive it.  wait() hands the
// proofs out; the destructor waits for a ticket nobody waited for, so the library never writes into freed memory.
class ProveTicket {
 public:
  ProveTicket() = default;
  ProveTicket(uint64_t ticket, std::vector<uint64_t> blinders, std::unique_ptr<std::vector<Proof>> proofs)
      : ticket_(ticket), pending_(true), blinders_(std::move(blinders)), proofs_(std::move(proofs)) {}
  ProveTicket(ProveTicket&& o) noexcept { *this = std::move(o); }
  ProveTicket& operator=(ProveTicket&& o) noexcept {
    if (this != &o) {
      finish();
      ticket_ = o.ticket_;
      pending_ = o.pending_;
      blinders_ = std::move(o.blinders_);
      proofs_ = std::move(o.proofs_);
      o.pending_ = false;
    }
    return *this;
  }
  ProveTicket(const ProveTicket&) = delete;
  ProveTicket& operator=(const ProveTicket&) = delete;
  ~ProveTicket() { finish(); }
  // true: done (then `result` holds the proofs or the proving call's error); false: not within timeout_ms (0 polls)
  bool wait_for(uint32_t timeout_ms, Result<std::vector<Proof>>* result) {
    if (!pending_) {
      *result = TxnApiError::failed_snark("prove_batch_async: the ticket's result was already taken");
      return true;
    }
    int done = 0;
    const int rc = capgpu_wait(ticket_, timeout_ms, &done);
    if (rc == CAPGPU_OK && !done) return false;
    pending_ = false;
    if (rc != CAPGPU_OK) *result = detail::map_error(rc, "prove_batch_async");
    else *result = std::move(*proofs_);
    return true;
  }
  Result<std::vector<Proof>> wait() {
    Result<std::vector<Proof>> r(TxnApiError::failed_snark("prove_batch_async"));
    (void)wait_for(UINT32_MAX, &r);
    return r;
  }

 private:
  void finish() {
    if (!pending_) return;
    int done = 0;
    (void)capgpu_wait(ticket_, UINT32_MAX, &done);
    pending_ = false;
  }
  uint64_t ticket_ = 0;
  bool pending_ = false;
  std::vector<uint64_t> blinders_;                // borrowed by the library until the ticket is done
  std::unique_ptr<std::vector<Proof>> proofs_;    // written by the library: a stable address across moves of the handle
};

// `count` proofs under one key from host memory without waiting for them: a.wires holds count x 5 x n field elements,
// a.pub_inputs count x num_inputs; the blinders are drawn now, in proof order, as count calls of prove() would draw them.
// One thread that keeps two tickets in flight reaches the rate of two bound threads.
template <class Rng>
Result<ProveTicket> prove_batch_async(Rng& rng, const ProvingKey& pk, const Assignment& a, size_t count,
                                      const std::vector<uint8_t>* ext_msg = nullptr) {
  if (!a.wires || (!a.pub_inputs && pk.num_inputs())) return TxnApiError::failed_snark("prove_batch_async: empty assignment");
  std::vector<uint64_t> blinders(count * 13 * 4);
  for (size_t i = 0; i < count * 13; i++) {
    Fr b = rng();
    std::memcpy(&blinders[4 * i], b.data(), 32);
  }
  auto proofs = std::make_unique<std::vector<Proof>>(count);
  uint64_t ticket = 0;
  int rc = capgpu_plonk_prove_batch_async(pk.handle(), (int)count, a.wires, a.pub_inputs, pk.num_inputs(),
                                          ext_msg ? ext_msg->data() : nullptr, ext_msg ? ext_msg->size() : 0,
                                          blinders.data(), a.input_form, proofs->data(), &ticket);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "prove_batch_async");
  return ProveTicket(ticket, std::move(blinders), std::move(proofs));
}

// One entry per note of prove_each: the proof, or the message its own prove() would have failed with (the reference's
// Vec<Result<..>> of one prove() per note, src/utils/params_builder.rs:194-226).
struct ProveEachEntry {
  std::optional<Proof> proof;
  std::string error;  // empty when the proof was made
};
// One proof per entry of `pks` (keys of ONE domain size under ONE SRS) in a single device batch that goes on PAST an
// unsatisfied witness (capgpu_plonk_prove_each): assignment i belongs to key i and is in the input form of the first.  A
// proof that was made is bit for bit what prove() makes of the same assignment and blinders; a note whose witness does
// not satisfy its circuit gets its error and costs the others nothing.  Err only when the batch could not run.
template <class Rng>
Result<std::vector<ProveEachEntry>> prove_each(Rng& rng, const std::vector<const ProvingKey*>& pks,
                                               const std::vector<Assignment>& as,
                                               const std::vector<std::vector<uint8_t>>* ext_msgs = nullptr) {
  const size_t count = pks.size();
  if (as.size() != count || (ext_msgs && ext_msgs->size() != count))
    return TxnApiError::failed_snark("prove_each: one assignment (and message) per key");
  std::vector<ProveEachEntry> out(count);
  if (!count) return out;
  size_t n = 0, ni = 0, per = 0;
  std::vector<uint64_t> handles(count);
  for (size_t i = 0; i < count; i++) {
    if (!pks[i] || !as[i].wires || (!as[i].pub_inputs && pks[i]->num_inputs()) || as[i].input_form != as[0].input_form)
      return TxnApiError::failed_snark("prove_each: empty assignment, or assignments of different input forms");
    handles[i] = pks[i]->handle();
    ni = std::max(ni, pks[i]->num_inputs());
  }
  int rc = capgpu_plonk_key_info(handles[0], &n, nullptr, nullptr);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "prove_each");
  per = 5 * n;
  if (as[0].input_form == CAPGPU_INPUT_VARS)
    for (size_t i = per = 0; i < count; i++) {
      size_t nv = 0;
      if ((rc = capgpu_plonk_key_num_vars(handles[i], &nv)) != CAPGPU_OK) return detail::map_error(rc, "prove_each");
      per = std::max(per, nv);
    }
  // the library takes one array of rows: the notes' own buffers are gathered (rows of the largest count, zero-filled)
  std::vector<uint64_t> wires(count * per * 4, 0), pubs(count * ni * 4 + 4, 0), blinders(count * 13 * 4);
  std::vector<const uint8_t*> mp(count, nullptr);
  std::vector<size_t> ml(count, 0);
  for (size_t i = 0; i < count; i++) {
    size_t own = per;
    if (as[0].input_form == CAPGPU_INPUT_VARS) capgpu_plonk_key_num_vars(handles[i], &own);
    std::memcpy(&wires[i * per * 4], as[i].wires, own * 32);
    if (pks[i]->num_inputs()) std::memcpy(&pubs[i * ni * 4], as[i].pub_inputs, pks[i]->num_inputs() * 32);
    for (int k = 0; k < 13; k++) {  // drawn in proof order, as count calls of prove() would draw them
      Fr b = rng();
      std::memcpy(&blinders[(i * 13 + k) * 4], b.data(), 32);
    }
    if (ext_msgs && !(*ext_msgs)[i].empty()) {
      mp[i] = (*ext_msgs)[i].data();
      ml[i] = (*ext_msgs)[i].size();
    }
  }
  std::vector<Proof> proofs(count);
  std::vector<capgpu_prove_outcome> oc(count);
  rc = capgpu_plonk_prove_each(handles.data(), (int)count, wires.data(), ni ? pubs.data() : nullptr, ni,
                               ext_msgs ? mp.data() : nullptr, ext_msgs ? ml.data() : nullptr, blinders.data(),
                               as[0].input_form, proofs.data(), oc.data());
  if (rc != CAPGPU_OK) return detail::map_error(rc, "prove_each");
  for (size_t i = 0; i < count; i++) {
    if (oc[i].status == CAPGPU_OK) {
      out[i].proof = proofs[i];
      continue;
    }
    char text[512];
    capgpu_prove_outcome_text(&oc[i], text, sizeof text);
    out[i].error = text;
  }
  return out;
}

// prove_each over keys of SEVERAL domain sizes (or SRS) - the reference's Vec<TransactionNote> of transfers, mints and
// freezes - in ONE call (capgpu_plonk_prove_notes): assignment i belongs to key i, all in the input form of the first, and
// is read where it is - no row array is built.  Every entry is bit for bit what prove_each makes of the notes of its
// group (same domain size and SRS) alone.  Err only when the call could not run.
template <class Rng>
Result<std::vector<ProveEachEntry>> prove_notes(Rng& rng, const std::vector<const ProvingKey*>& pks,
                                                const std::vector<Assignment>& as,
                                                const std::vector<std::vector<uint8_t>>* ext_msgs = nullptr) {
  const size_t count = pks.size();
  if (as.size() != count || (ext_msgs && ext_msgs->size() != count))
    return TxnApiError::failed_snark("prove_notes: one assignment (and message) per key");
  std::vector<ProveEachEntry> out(count);
  if (!count) return out;
  size_t ni = 0;
  std::vector<uint64_t> handles(count);
  std::vector<const uint64_t*> rows(count);
  for (size_t i = 0; i < count; i++) {
    if (!pks[i] || !as[i].wires || (!as[i].pub_inputs && pks[i]->num_inputs()) || as[i].input_form != as[0].input_form)
      return TxnApiError::failed_snark("prove_notes: empty assignment, or assignments of different input forms");
    handles[i] = pks[i]->handle();
    rows[i] = as[i].wires;
    ni = std::max(ni, pks[i]->num_inputs());
  }
  std::vector<uint64_t> pubs(count * ni * 4 + 4, 0), blinders(count * 13 * 4);
  std::vector<const uint8_t*> mp(count, nullptr);
  std::vector<size_t> ml(count, 0);
  for (size_t i = 0; i < count; i++) {
    if (pks[i]->num_inputs()) std::memcpy(&pubs[i * ni * 4], as[i].pub_inputs, pks[i]->num_inputs() * 32);
    for (int k = 0; k < 13; k++) {  // drawn in note order, as count calls of prove() would draw them
      Fr b = rng();
      std::memcpy(&blinders[(i * 13 + k) * 4], b.data(), 32);
    }
    if (ext_msgs && !(*ext_msgs)[i].empty()) {
      mp[i] = (*ext_msgs)[i].data();
      ml[i] = (*ext_msgs)[i].size();
    }
  }
  std::vector<Proof> proofs(count);
  std::vector<capgpu_prove_outcome> oc(count);
  const int rc = capgpu_plonk_prove_notes(handles.data(), (int)count, rows.data(), ni ? pubs.data() : nullptr, ni,
                                          ext_msgs ? mp.data() : nullptr, ext_msgs ? ml.data() : nullptr, blinders.data(),
                                          as[0].input_form, proofs.data(), oc.data());
  if (rc != CAPGPU_OK) return detail::map_error(rc, "prove_notes");
  for (size_t i = 0; i < count; i++) {
    if (oc[i].status == CAPGPU_OK) {
      out[i].proof = proofs[i];
      continue;
    }
    char text[512];
    capgpu_prove_outcome_text(&oc[i], text, sizeof text);
    out[i].error = text;
  }
  return out;
}

// The form of the schedule a key's solver runs (capgpu_plonk_key_set_solve_form): CAPGPU_SOLVE_FORM_DIRECT, what every
// set-up call leaves, or CAPGPU_SOLVE_FORM_DEFERRED, which inverts the denominators of a chain of additions together.  Either
// form gives prove_given the same assignments and the same proofs.  The key needs a solver.
inline Result<capgpu_solve_form_info> set_solve_form(const ProvingKey& pk, int form) {
  capgpu_solve_form_info info{};
  int rc = capgpu_plonk_key_set_solve_form(pk.handle(), form, &info);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "set_solve_form");
  return info;
}
inline Result<capgpu_solve_form_info> solve_form_info(const ProvingKey& pk) {
  capgpu_solve_form_info info{};
  int rc = capgpu_plonk_key_solve_form_info(pk.handle(), &info);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "solve_form_info");
  return info;
}

// The values one circuit is given, for prove_given: `given` in the order of the key's given list (Montgomery words,
// capgpu_plonk_key_set_given), pub_inputs as in an Assignment.
struct GivenValues {
  const uint64_t* given = nullptr;
  size_t num_given = 0;
  const uint64_t* pub_inputs = nullptr;
};
// prove_each from the values each circuit is GIVEN (capgpu_plonk_prove_given): the library completes every assignment on
// the device and proves it in the same call.  Every key needs a solver.  A proof that was made is bit for bit what
// solving and then prove_each in variable form make of it.
template <class Rng>
Result<std::vector<ProveEachEntry>> prove_given(Rng& rng, const std::vector<const ProvingKey*>& pks,
                                                const std::vector<GivenValues>& gs,
                                                const std::vector<std::vector<uint8_t>>* ext_msgs = nullptr) {
  const size_t count = pks.size();
  if (gs.size() != count || (ext_msgs && ext_msgs->size() != count))
    return TxnApiError::failed_snark("prove_given: one set of given values (and message) per key");
  std::vector<ProveEachEntry> out(count);
  if (!count) return out;
  size_t ni = 0, per = 0;
  std::vector<uint64_t> handles(count);
  for (size_t i = 0; i < count; i++) {
    if (!pks[i] || (!gs[i].given && gs[i].num_given) || (!gs[i].pub_inputs && pks[i]->num_inputs()))
      return TxnApiError::failed_snark("prove_given: empty given values or public inputs");
    handles[i] = pks[i]->handle();
    ni = std::max(ni, pks[i]->num_inputs());
    per = std::max(per, gs[i].num_given);
  }
  // one array of rows of the largest length, zero-filled
  std::vector<uint64_t> given(count * per * 4 + 4, 0), pubs(count * ni * 4 + 4, 0), blinders(count * 13 * 4);
  std::vector<const uint8_t*> mp(count, nullptr);
  std::vector<size_t> ml(count, 0);
  for (size_t i = 0; i < count; i++) {
    if (gs[i].num_given) std::memcpy(&given[i * per * 4], gs[i].given, gs[i].num_given * 32);
    if (pks[i]->num_inputs()) std::memcpy(&pubs[i * ni * 4], gs[i].pub_inputs, pks[i]->num_inputs() * 32);
    for (int k = 0; k < 13; k++) {
      Fr b = rng();
      std::memcpy(&blinders[(i * 13 + k) * 4], b.data(), 32);
    }
    if (ext_msgs && !(*ext_msgs)[i].empty()) {
      mp[i] = (*ext_msgs)[i].data();
      ml[i] = (*ext_msgs)[i].size();
    }
  }
  std::vector<Proof> proofs(count);
  std::vector<capgpu_prove_outcome> oc(count);
  int rc = capgpu_plonk_prove_given(handles.data(), (int)count, given.data(), ni ? pubs.data() : nullptr, ni,
                                    ext_msgs ? mp.data() : nullptr, ext_msgs ? ml.data() : nullptr, blinders.data(),
                                    proofs.data(), oc.data(), nullptr);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "prove_given");
  for (size_t i = 0; i < count; i++) {
    if (oc[i].status == CAPGPU_OK) {
      out[i].proof = proofs[i];
      continue;
    }
    char text[512];
    capgpu_prove_outcome_text(&oc[i], text, sizeof text);
    out[i].error = text;
  }
  return out;
}

// prove_given without public inputs to pass (capgpu_plonk_prove_given_io): the library computes them from each completed
// assignment - the values the circuit ties to its public variables - proves against them and hands them back.
// GivenValues::pub_inputs is not read.  pub_inputs[i] holds the num_inputs() words x 4 of key i, whatever became of its
// proof.  Every key needs a solver (capgpu_plonk_key_set_solver with CAPGPU_SOLVER_DERIVE_PUBLIC for a key whose public
// inputs are not all given).
struct ProveGivenIo {
  std::vector<ProveEachEntry> proofs;
  std::vector<std::vector<uint64_t>> pub_inputs;
};
template <class Rng>
Result<ProveGivenIo> prove_given_io(Rng& rng, const std::vector<const ProvingKey*>& pks, const std::vector<GivenValues>& gs,
                                    const std::vector<std::vector<uint8_t>>* ext_msgs = nullptr) {
  const size_t count = pks.size();
  if (gs.size() != count || (ext_msgs && ext_msgs->size() != count))
    return TxnApiError::failed_snark("prove_given_io: one set of given values (and message) per key");
  ProveGivenIo out;
  out.proofs.resize(count);
  out.pub_inputs.resize(count);
  if (!count) return out;
  size_t ni = 0, per = 0;
  std::vector<uint64_t> handles(count);
  for (size_t i = 0; i < count; i++) {
    if (!pks[i] || (!gs[i].given && gs[i].num_given)) return TxnApiError::failed_snark("prove_given_io: empty given values");
    handles[i] = pks[i]->handle();
    ni = std::max(ni, pks[i]->num_inputs());
    per = std::max(per, gs[i].num_given);
  }
  std::vector<uint64_t> given(count * per * 4 + 4, 0), pubs(count * ni * 4 + 4, 0), blinders(count * 13 * 4);
  std::vector<const uint8_t*> mp(count, nullptr);
  std::vector<size_t> ml(count, 0);
  for (size_t i = 0; i < count; i++) {
    if (gs[i].num_given) std::memcpy(&given[i * per * 4], gs[i].given, gs[i].num_given * 32);
    for (int k = 0; k < 13; k++) {
      Fr b = rng();
      std::memcpy(&blinders[(i * 13 + k) * 4], b.data(), 32);
    }
    if (ext_msgs && !(*ext_msgs)[i].empty()) {
      mp[i] = (*ext_msgs)[i].data();
      ml[i] = (*ext_msgs)[i].size();
    }
  }
  std::vector<Proof> proofs(count);
  std::vector<capgpu_prove_outcome> oc(count);
  int rc = capgpu_plonk_prove_given_io(handles.data(), (int)count, given.data(), ni, ext_msgs ? mp.data() : nullptr,
                                       ext_msgs ? ml.data() : nullptr, blinders.data(), ni ? pubs.data() : nullptr,
                                       proofs.data(), oc.data(), nullptr);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "prove_given_io");
  for (size_t i = 0; i < count; i++) {
    out.pub_inputs[i].assign(pubs.begin() + i * ni * 4, pubs.begin() + (i * ni + pks[i]->num_inputs()) * 4);
    if (oc[i].status == CAPGPU_OK) {
      out.proofs[i].proof = proofs[i];
      continue;
    }
    char text[512];
    capgpu_prove_outcome_text(&oc[i], text, sizeof text);
    out.proofs[i].error = text;
  }
  return out;
}

// prove() for ONE note from the values its circuit is given (capgpu_plonk_prove_given_one): what each thread of a parallel
// loop over notes calls.  With capgpu_plonk_set_coalescing on, concurrent calls are gathered into one solve and one device
// batch; the proof is bit for bit the lone call's either way.  The outer error: the call could not run.
template <class Rng>
Result<ProveEachEntry> prove_given_one(Rng& rng, const ProvingKey& pk, const GivenValues& g,
                                       const std::vector<uint8_t>* ext_msg = nullptr) {
  if ((!g.given && g.num_given) || (!g.pub_inputs && pk.num_inputs()))
    return TxnApiError::failed_snark("prove_given_one: empty given values or public inputs");
  uint64_t blinders[13 * 4];
  for (int k = 0; k < 13; k++) {
    Fr b = rng();
    std::memcpy(&blinders[k * 4], b.data(), 32);
  }
  const bool msg = ext_msg && !ext_msg->empty();
  Proof proof;
  capgpu_prove_outcome oc{};
  int rc = capgpu_plonk_prove_given_one(pk.handle(), g.given, g.num_given, g.pub_inputs, pk.num_inputs(),
                                        msg ? ext_msg->data() : nullptr, msg ? ext_msg->size() : 0, blinders, &proof, &oc,
                                        nullptr);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "prove_given_one");
  ProveEachEntry out;
  if (oc.status == CAPGPU_OK) {
    out.proof = proof;
  } else {
    char text[512];
    capgpu_prove_outcome_text(&oc, text, sizeof text);
    out.error = text;
  }
  return out;
}
// ... without public inputs to pass (capgpu_plonk_prove_given_io_one): pub_inputs receives the key's num_inputs() x 4 words
// the library proved against, whatever became of the proof.
template <class Rng>
Result<ProveEachEntry> prove_given_io_one(Rng& rng, const ProvingKey& pk, const GivenValues& g,
                                          std::vector<uint64_t>* pub_inputs, const std::vector<uint8_t>* ext_msg = nullptr) {
  if ((!g.given && g.num_given) || !pub_inputs) return TxnApiError::failed_snark("prove_given_io_one: empty given values");
  uint64_t blinders[13 * 4];
  for (int k = 0; k < 13; k++) {
    Fr b = rng();
    std::memcpy(&blinders[k * 4], b.data(), 32);
  }
  const bool msg = ext_msg && !ext_msg->empty();
  const size_t ni = pk.num_inputs();
  pub_inputs->assign(ni * 4, 0);
  Proof proof;
  capgpu_prove_outcome oc{};
  int rc = capgpu_plonk_prove_given_io_one(pk.handle(), g.given, g.num_given, ni, msg ? ext_msg->data() : nullptr,
                                           msg ? ext_msg->size() : 0, blinders, ni ? pub_inputs->data() : nullptr, &proof, &oc,
                                           nullptr);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "prove_given_io_one");
  ProveEachEntry out;
  if (oc.status == CAPGPU_OK) {
    out.proof = proof;
  } else {
    char text[512];
    capgpu_prove_outcome_text(&oc, text, sizeof text);
    out.error = text;
  }
  return out;
}

}  // namespace proof

// ---- Transfer (src/proof/transfer.rs) ----------------------------------------------------------------------------
struct TransferProvingKey {
  ProvingKey proving_key;
  size_t n_inputs = 0, n_outputs = 0;
  uint8_t tree_depth = 0;
  size_t num_input() const { return n_inputs; }    // transfer.rs:100-102
  size_t num_output() const { return n_outputs; }  // transfer.rs:105-107
};
struct TransferVerifyingKey {
  VerifyingKey verifying_key;
  size_t n_inputs = 0, n_outputs = 0;
  uint8_t tree_depth = 0;
  TransferVerifyingKey() = default;
  explicit TransferVerifyingKey(const TransferProvingKey& pk)  // impl From<&TransferProvingKey>, transfer.rs:110-119
      : verifying_key(pk.proving_key.vk), n_inputs(pk.n_inputs), n_outputs(pk.n_outputs), tree_depth(pk.tree_depth) {}
};
// ---- Mint (src/proof/mint.rs:45-66) ------------------------------------------------------------------------------
struct MintProvingKey {
  ProvingKey proving_key;
  uint8_t tree_depth = 0;
};
struct MintVerifyingKey {
  VerifyingKey verifying_key;
  uint8_t tree_depth = 0;
  MintVerifyingKey() = default;
  explicit MintVerifyingKey(const MintProvingKey& pk) : verifying_key(pk.proving_key.vk), tree_depth(pk.tree_depth) {}
};
// ---- Freeze (src/proof/freeze.rs:44-90) --------------------------------------------------------------------------
struct FreezeProvingKey {
  ProvingKey proving_key;
  uint8_t tree_depth = 0;
  size_t num_input = 0;
};
struct FreezeVerifyingKey {
  VerifyingKey verifying_key;
  uint8_t tree_depth = 0;
  size_t num_input = 0;
  FreezeVerifyingKey() = default;
  explicit FreezeVerifyingKey(const FreezeProvingKey& pk)
      : verifying_key(pk.proving_key.vk), tree_depth(pk.tree_depth), num_input(pk.num_input) {}
};

namespace proof {
namespace transfer {
struct Preprocessed {
  TransferProvingKey proving_key;
  TransferVerifyingKey verifying_key;
  size_t n_constraints;
};
// transfer.rs:124-155.  `circuit` stands for TransferCircuit::build_for_preprocessing(n_inputs, n_outputs, tree_depth).
inline Result<Preprocessed> preprocess(const UniversalSrs& srs, size_t n_inputs, size_t n_outputs, uint8_t tree_depth,
                                       const FinalisedCircuit& circuit) {
  auto r = detail_snark::preprocess(srs, circuit,
                                    "Preprocessing Transfer circuit of " + std::to_string(n_inputs) + "-in-" +
                                        std::to_string(n_outputs) + "-out-" + std::to_string(tree_depth) + "-depth failed");
  if (r.is_err()) return r.error();
  TransferProvingKey pk{std::move(r.unwrap().first), n_inputs, n_outputs, tree_depth};
  TransferVerifyingKey vk(pk);
  return Preprocessed{std::move(pk), vk, circuit.num_gates};
}
// transfer.rs:159-188.  The satisfiability check of the reference (check_circuit_satisfiability, :169-176) is not made
// here: proof::check_satisfiability (above) is that step on the device, for callers who want it, and
// capgpu_plonk_set_precheck(1) puts it in front of every prove call.  Without either, an unsatisfied assignment is still
// caught: the quotient's degree check fails and the call returns Err(FailedSnark) like the reference does - naming no gate.
template <class Rng>
Result<Proof> prove(Rng& rng, const TransferProvingKey& pk, const Assignment& witness,
                    const std::vector<uint8_t>& txn_memo_ver_key, const std::vector<uint8_t>& extra_proof_bound_data) {
  const std::vector<uint8_t> ext_msg = detail_snark::bound_message(txn_memo_ver_key, extra_proof_bound_data);
  return detail_snark::prove(rng, pk.proving_key, witness, &ext_msg, "Transfer Proof Creation failure");
}
// the same from the circuit's variable assignment (a key whose circuit came with wire_vars)
template <class Rng>
Result<Proof> prove(Rng& rng, const TransferProvingKey& pk, const VariableAssignment& witness,
                    const std::vector<uint8_t>& txn_memo_ver_key) {
  return prove(rng, pk, witness.as_assignment(), txn_memo_ver_key);
}
// transfer.rs:192-212
inline Result<Unit> verify(const TransferVerifyingKey& vk, const std::vector<Fr>& public_inputs, const Proof& proof,
                           const std::vector<uint8_t>& recv_memos_ver_key,
                           const std::vector<uint8_t>& extra_proof_bound_data) {
  const std::vector<uint8_t> ext_msg = detail_snark::bound_message(recv_memos_ver_key, extra_proof_bound_data);
  return detail_snark::verify(vk.verifying_key, public_inputs, proof, &ext_msg, "Transfer Proof Verification failure");
}
}  // namespace transfer

namespace mint {
struct Preprocessed {
  MintProvingKey proving_key;
  MintVerifyingKey verifying_key;
  size_t n_constraints;
};
// mint.rs:69-93
inline Result<Preprocessed> preprocess(const UniversalSrs& srs, uint8_t tree_depth, const FinalisedCircuit& circuit) {
  auto r = detail_snark::preprocess(srs, circuit, "Preprocessing Mint circuit of depth " + std::to_string(tree_depth) + " failed");
  if (r.is_err()) return r.error();
  MintProvingKey pk{std::move(r.unwrap().first), tree_depth};
  MintVerifyingKey vk(pk);
  return Preprocessed{std::move(pk), vk, circuit.num_gates};
}
// mint.rs:97-120: ext_msg = serialised txn memo verification key, no extra bound data
template <class Rng>
Result<Proof> prove(Rng& rng, const MintProvingKey& pk, const Assignment& witness,
                    const std::vector<uint8_t>& txn_memo_ver_key) {
  return detail_snark::prove(rng, pk.proving_key, witness, &txn_memo_ver_key, "Mint Proof creation failure");
}
template <class Rng>
Result<Proof> prove(Rng& rng, const MintProvingKey& pk, const VariableAssignment& witness,
                    const std::vector<uint8_t>& txn_memo_ver_key) {
  return prove(rng, pk, witness.as_assignment(), txn_memo_ver_key);
}
// mint.rs:124-140
inline Result<Unit> verify(const MintVerifyingKey& vk, const std::vector<Fr>& public_inputs, const Proof& proof,
                           const std::vector<uint8_t>& recv_memos_ver_key) {
  return detail_snark::verify(vk.verifying_key, public_inputs, proof, &recv_memos_ver_key,
                              "Mint Proof verification failure");
}
}  // namespace mint

namespace freeze {
struct Preprocessed {
  FreezeProvingKey proving_key;
  FreezeVerifyingKey verifying_key;
  size_t n_constraints;
};
// freeze.rs:93-121
inline Result<Preprocessed> preprocess(const UniversalSrs& srs, size_t num_input, uint8_t tree_depth,
                                       const FinalisedCircuit& circuit) {
  auto r = detail_snark::preprocess(srs, circuit,
                                    "Preprocessing Freeze circuit of " + std::to_string(num_input) + "-inputs-" +
                                        std::to_string(tree_depth) + "-depth failed");
  if (r.is_err()) return r.error();
  FreezeProvingKey pk{std::move(r.unwrap().first), tree_depth, num_input};
  FreezeVerifyingKey vk(pk);
  return Preprocessed{std::move(pk), vk, circuit.num_gates};
}
// freeze.rs:125-158: ext_msg = serialised txn memo verification key only
template <class Rng>
Result<Proof> prove(Rng& rng, const FreezeProvingKey& pk, const Assignment& witness,
                    const std::vector<uint8_t>& txn_memo_ver_key) {
  return detail_snark::prove(rng, pk.proving_key, witness, &txn_memo_ver_key, "Freeze Proof creation failure");
}
template <class Rng>
Result<Proof> prove(Rng& rng, const FreezeProvingKey& pk, const VariableAssignment& witness,
                    const std::vector<uint8_t>& txn_memo_ver_key) {
  return prove(rng, pk, witness.as_assignment(), txn_memo_ver_key);
}
// freeze.rs:162-178
inline Result<Unit> verify(const FreezeVerifyingKey& vk, const std::vector<Fr>& public_inputs, const Proof& proof,
                           const std::vector<uint8_t>& recv_memos_ver_key) {
  return detail_snark::verify(vk.verifying_key, public_inputs, proof, &recv_memos_ver_key,
                              "Freeze Proof Verification failure");
}
}  // namespace freeze
}  // namespace proof

// txn_batch_verify's SNARK part (src/lib.rs:455-529, PlonkKzgSnark::batch_verify at :517-522): one pairing product for
// proofs of different keys under one SRS.  on_device: the group arithmetic runs on the GPU (capgpu_plonk_batch_verify_dev).
struct BatchItem {
  const VerifyingKey* verifying_key;
  const std::vector<Fr>* public_inputs;
  const Proof* proof;
  const std::vector<uint8_t>* ext_msg;  // the bound message of that note (may be null)
};
inline Result<Unit> batch_verify(const std::vector<BatchItem>& items, bool on_device = false) {
  if (items.empty()) return Unit{};
  std::vector<const capgpu_verifying_key*> vks;
  std::vector<const uint64_t*> pubs;
  std::vector<size_t> nin, lens;
  std::vector<const capgpu_proof*> proofs;
  std::vector<const uint8_t*> msgs;
  for (const BatchItem& it : items) {
    vks.push_back(&it.verifying_key->raw);
    pubs.push_back(it.public_inputs->empty() ? nullptr : (*it.public_inputs)[0].data());
    nin.push_back(it.public_inputs->size());
    proofs.push_back(it.proof);
    msgs.push_back(it.ext_msg && !it.ext_msg->empty() ? it.ext_msg->data() : nullptr);
    lens.push_back(it.ext_msg ? it.ext_msg->size() : 0);
  }
  const VerifyingKey& k0 = *items[0].verifying_key;
  int ok = 0;
  auto fn = on_device ? capgpu_plonk_batch_verify_dev : capgpu_plonk_batch_verify;
  int rc = fn(vks.data(), k0.h.data(), k0.beta_h.data(), pubs.data(), nin.data(), proofs.data(), msgs.data(), lens.data(),
              items.size(), &ok);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Batch Proof Verification failure");
  if (!ok) return TxnApiError::failed_snark("Batch Proof Verification failure: WrongProof");
  return Unit{};
}

// `Proof` inside a note is ark-serialize bytes (src/transfer.rs:60): CanonicalSerialize / CanonicalDeserialize
inline Result<std::vector<uint8_t>> serialize(const Proof& p) {
  std::vector<uint8_t> out(1024);
  size_t len = 0;
  int rc = capgpu_proof_serialize(&p, out.data(), out.size(), &len);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Proof serialization");
  out.resize(len);
  return out;
}
inline Result<Proof> deserialize_proof(const std::vector<uint8_t>& bytes) {
  Proof p;
  size_t used = 0;
  int rc = capgpu_proof_deserialize(bytes.data(), bytes.size(), &p, &used);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Proof deserialization");
  return p;
}


// The same for a block of notes, on the device (capgpu_proof_decode_batch / _encode_batch): `records` holds one
// CAPGPU_PROOF_BYTES record per proof, packed.  A record that does not decode is no error of the call: its status is
// 1 + the byte offset of the first malformed field and its Proof is all-ones words, which every verifier here refuses.
struct DecodedProofs {
  std::vector<Proof> proofs;
  std::vector<int> status;  // 0: decoded
};
inline Result<DecodedProofs> deserialize_proofs(const std::vector<uint8_t>& records) {
  DecodedProofs out;
  const size_t count = records.size() / CAPGPU_PROOF_BYTES;
  if (records.size() != count * CAPGPU_PROOF_BYTES) return TxnApiError::failed_snark("Proof deserialization: not a whole number of records");
  out.proofs.resize(count);
  out.status.resize(count);
  int rc = capgpu_proof_decode_batch(records.data(), CAPGPU_PROOF_BYTES, count, out.proofs.data(), out.status.data());
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Proof deserialization");
  return out;
}
inline Result<std::vector<uint8_t>> serialize_proofs(const std::vector<Proof>& proofs) {
  std::vector<uint8_t> out(proofs.size() * CAPGPU_PROOF_BYTES);
  int rc = capgpu_proof_encode_batch(proofs.data(), proofs.size(), out.data(), CAPGPU_PROOF_BYTES);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Proof serialization");
  return out;
}

// txn_batch_verify (src/lib.rs:455-529) for a validator that holds each note's proof as its bytes: keys uploaded once
// (capgpu_plonk_vk_upload), `records` as above, pub_inputs `count` rows of num_inputs elements, ext_msgs empty or one
// entry per proof.  Decoding, transcripts, scalars, group arithmetic and the pairing check run on the device behind one
// host wait (capgpu_plonk_verify_block_bytes); a record that does not decode fails the block like a wrong proof.
inline Result<Unit> batch_verify_bytes(const std::vector<uint64_t>& vk_handles, const std::array<uint64_t, 16>& h,
                                       const std::array<uint64_t, 16>& beta_h, const std::vector<Fr>& pub_inputs,
                                       size_t num_inputs, const std::vector<uint8_t>& records,
                                       const std::vector<std::vector<uint8_t>>& ext_msgs = {}) {
  const size_t count = vk_handles.size();
  if (records.size() != count * CAPGPU_PROOF_BYTES || pub_inputs.size() != count * num_inputs ||
      (!ext_msgs.empty() && ext_msgs.size() != count))
    return TxnApiError::failed_snark("Batch Proof Verification failure: one record, one row and one message per key handle");
  std::vector<const uint8_t*> msgs;
  std::vector<size_t> lens;
  for (const auto& m : ext_msgs) {
    msgs.push_back(m.empty() ? nullptr : m.data());
    lens.push_back(m.size());
  }
  int ok = 0;
  int rc = capgpu_plonk_verify_block_bytes(vk_handles.data(), h.data(), beta_h.data(),
                                           pub_inputs.empty() ? nullptr : pub_inputs[0].data(), num_inputs, records.data(),
                                           CAPGPU_PROOF_BYTES, msgs.empty() ? nullptr : msgs.data(),
                                           lens.empty() ? nullptr : lens.data(), count, &ok, nullptr, nullptr);
  if (rc != CAPGPU_OK) return detail::map_error(rc, "Batch Proof Verification failure");
  if (!ok) return TxnApiError::failed_snark("Batch Proof Verification failure: WrongProof");
  return Unit{};
}

}  // namespace capgpu

#endif  // CAPGPU_PROOF_HPP
