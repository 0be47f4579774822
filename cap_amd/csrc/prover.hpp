// The seam of the prover: what plonk.hip - the one unit that holds the prover's kernels and launches them - offers to a
// unit without device code: plonk_keys.hip and plonk_solver.hip.  It declares what those two call and no more - the
// types of a proving call (ProveRequest, ProvePlan ...) are prove_run.hpp's, because the C boundary of proving that uses
// them stands in plonk.hip.  It is the only door: a host unit reaches nothing of plonk.hip or prove_run.hpp but what is
// declared here, so a change to such a unit recompiles no kernel.  Two rules keep it so
// (tests/test_plonk_units.py holds them):
//   * every `launch(` and every `__global__` of the prover is compiled in plonk.hip alone - this header includes no
//     *_kernels.hpp and not transcript_dev.hpp, and a host unit that needs a launch gets a wrapper from here;
//   * CAP_FL_SCHED is plonk.hip's own: nothing here depends on the multiplication schedule a unit compiles field29.hpp with.
#pragma once
#include <atomic>

#include "context.hpp"
#include "host_util.hpp"

namespace cap {

struct ProvingKey;  // plonk_key.hpp

// the layout of a scratch buffer: pieces at 256-byte steps; base == nullptr sizes only
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  template <class T>
  T* take(size_t count) {
    off = (off + 255) / 256 * 256;
    T* p = base ? (T*)(base + off) : nullptr;
    off += sizeof(T) * count;
    return p;
  }
};

// ---- the launch wrappers a key builder needs (prove_run.hpp) -------------------------------------------------------------
int run_ntt(hipStream_t s, uint32_t log_n, fe* data, size_t stride, uint32_t count, int dir, int coset);
int run_msm(hipStream_t s, const MsmBases& B, const fe* scalars, size_t outer_stride, uint32_t inner, size_t inner_stride,
            size_t n, uint32_t batch, g1_jac* d_out);
// pk::pad_copy (round_launch.hpp): columns copied and zero-extended
void pad_columns(hipStream_t s, fe* dst, size_t dst_outer, size_t dst_inner, const fe* src, size_t src_outer,
                 size_t src_inner, uint32_t inner, uint32_t count, size_t len, size_t total);
// the extended permutation from a wire -> variable table, its field form, and the first cell at which two permutations in
// index form differ (*d_first: ~0 going in, the smallest differing cell coming out) - vars_kernels.hpp, plonk.hip
int vars_build_perm(hipStream_t s, const uint32_t* d_table, size_t n, uint32_t* d_perm);
void vars_sigma_values(hipStream_t s, uint32_t log_n, const uint32_t* d_perm, fe* d_sigma);
void vars_first_difference(hipStream_t s, const uint32_t* d_perm, const uint32_t* d_key_perm, size_t cells,
                           unsigned long long* d_first);

// ---- the tables a key derives on the device (plonk.hip) --------------------------------------------------------------------
// everything derived from the coefficient table: constants of the quotient kernel, 1 / (n (x - 1)) on the coset,
// and the cached coset evaluations of the 18 fixed polynomials
int key_finish_tables(hipStream_t s, ProvingKey& K);
// selector values on the domain and the index form of sigma, on the current context's stream; synchronous
int key_check_tables(const ProvingKey& K);

// ---- modes and counters --------------------------------------------------------------------------------------------------
bool wire_commit_from_evals();  // round 1 commits on the Lagrange-form key: preprocess builds it ahead
extern std::atomic<uint64_t> g_witness_h2d, g_gather_launches;  // capgpu_plonk_input_stats

}  // namespace cap
