// What the host verifier (verify.hip) hands to the per-proof device verifier (verify_dev.hip).
#pragma once
#include <vector>

#include "../../include/capgpu.h"
#include "pairing.hpp"

namespace cap {

// One proof's pairing inputs A = sum a[k].s a[k].p, B = likewise; the proof holds iff e(A, [tau]H) e(-B, H) == 1.
// Points as in the ABI (arkworks Montgomery words, (0, 0) = infinity), scalars canonical integers (< r).
struct EachTerm {
  g1_affine p;
  fe s;
};
struct EachTerms {
  std::vector<EachTerm> a, b;
  int valid = 0;  // 0: already known to be invalid (off-curve or non-canonical input, zeta in the domain)
};

// The terms of every proof of a batch, on the host threads of capgpu_plonk_batch_verify.  A negative return code only for
// malformed arguments (the cases capgpu_plonk_batch_verify rejects); an invalid proof gets valid = 0.
int batch_terms_each(const capgpu_verifying_key* const* vks, const uint64_t* const* pub_inputs,
                     const size_t* num_inputs, const capgpu_proof* const* proofs, const uint8_t* const* ext_msgs,
                     const size_t* ext_msg_lens, size_t count, std::vector<EachTerms>* out);
// the open key's G2 elements from ABI words: CAPGPU_ERR_INVALID_ARG when off the twist or at infinity
int open_key_from_abi(const uint64_t g2_h[16], const uint64_t g2_beta_h[16], pairing::g2_affine* h,
                      pairing::g2_affine* beta_h);
// ABI words -> points (all-zero = infinity)
pairing::g2_affine g2_from_abi(const uint64_t w[16]);
g1_affine g1_from_abi(const uint64_t w[8]);
// canonical coordinates and on the curve (infinity included)
bool g1_abi_on_curve(const g1_affine& p);

// What verify_dev.hip offers the batch verifier: the pairing form in force (capgpu_pairing_set_form) and
// *ok_out = (e(p, q1) e(r, q2) == 1) decided on the device by one wave-form check ((0, 0) = infinity in p and r)
int pairing_form();
int pairing_check2_wave_dev(const g1_affine& p, const pairing::g2_affine& q1, const g1_affine& r,
                            const pairing::g2_affine& q2, int* ok_out);

}  // namespace cap
