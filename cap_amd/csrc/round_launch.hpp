// Launch geometry of the round kernels of plonk_kernels.hpp: one place for the grid and block of every launch, shared by
// the prover (prove_run.hpp) and by the direct driver of these kernels (tests/hip/roundcheck.hip), so that the driver
// runs each kernel in the geometry the prover gives it.  Host side only; the order of the launches stays with the caller.
#pragma once
#include "launch.hpp"
#include "plonk_kernels.hpp"

namespace cap {

inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

namespace pk {

inline void pad_copy(hipStream_t s, fe* dst, size_t dst_outer, size_t dst_inner, const fe* src, size_t src_outer,
                     size_t src_inner, uint32_t inner, uint32_t count, size_t len, size_t total) {
  if (count == 0 || total == 0) return;
  launch("k_pad_copy", k_pad_copy, dim3(cdiv(total, kThreads), count), dim3(kThreads), 0, s, dst, dst_outer, dst_inner,
         src, src_outer, src_inner, inner, len, total);
}

// tot: batch * cdiv(len, kScanBlock) elements
template <int OP, int REV>
void scan_exclusive(hipStream_t s, const fe* in, fe* out, size_t len, size_t stride, uint32_t batch, fe* tot) {
  uint32_t nblocks = cdiv(len, kScanBlock);
  launch(OP == 0 ? "k_scan_local_mul" : "k_scan_local_add", k_scan_local<OP, REV>, dim3(nblocks, batch), dim3(kThreads),
         0, s, in, out, len, stride, tot, nblocks);
  if (nblocks > 1) {
    launch("k_scan_totals", k_scan_totals<OP>, dim3(batch), dim3(64), 0, s, tot, nblocks);
    launch("k_scan_apply", k_scan_apply<OP, REV>, dim3(nblocks, batch), dim3(kThreads), 0, s, out, len, stride,
           (const fe*)tot, nblocks);
  }
}

// ---- round 2 ---------------------------------------------------------------------------------------------------------
inline void perm_numden(hipStream_t s, const fe* wires, const fe* sig_eval, const fe* const* sig_of, const fe* tw_n,
                        const Chal* chal, const QuotConst& qc29, size_t n, uint32_t P, fe* num, fe* den) {
  launch("k_perm_numden", k_perm_numden, dim3(cdiv(n, kThreads), P), dim3(kThreads), 0, s, wires, sig_eval, sig_of, tw_n,
         chal, qc29, n, num, den);
}
inline void perm_inv_total(hipStream_t s, const fe* sfx, const fe* den, size_t n, fe* inv_total, uint32_t P) {
  launch("k_perm_inv_total", k_perm_inv_total, dim3(cdiv(P, 64)), dim3(64), 0, s, sfx, den, n, inv_total, P);
}
inline void perm_total(hipStream_t s, const fe* sfx, const fe* den, size_t n, fe* total, uint32_t P) {
  launch("k_perm_total", k_perm_total, dim3(cdiv(P, 64)), dim3(64), 0, s, sfx, den, n, total, P);
}
inline void perm_finish(hipStream_t s, const fe* pre, const fe* sfx, const fe* den, const fe* inv_total, size_t n,
                        uint32_t P, fe* z, size_t zstride) {
  launch("k_perm_finish", k_perm_finish, dim3(cdiv(zstride, kThreads), P), dim3(kThreads), 0, s, pre, sfx, den, inv_total,
         n, z, zstride);
}

// ---- round 3 ---------------------------------------------------------------------------------------------------------
inline void kx_columns(hipStream_t s, fe* dst, const fe* xs, const QuotConst& qc29, size_t m) {
  launch("k_kx_columns", k_kx_columns, dim3(cdiv(m, kThreads)), dim3(kThreads), 0, s, dst, xs, qc29, m);
}
// pts: points per proof - m, or 5 m / 6 under `five`
template <bool FOLD>
void quotient(hipStream_t s, uint32_t P, size_t pts, const fe* pkc, const fe* const* pkc_of, const fe* cos,
              const fe* xs, const fe* inv_nx1, const Chal* chal29, const QuotConst& qc29, size_t m,
              uint32_t only_unfoldable, uint32_t five, fe* t) {
  launch(FOLD ? "k_quotient" : "k_quotient_direct", k_quotient<FOLD>, dim3(P, cdiv(pts, kThreads)), dim3(kThreads), 0, s,
         pkc, pkc_of, cos, xs, inv_nx1, chal29, qc29, m, only_unfoldable, five, t);
}
inline void quotient_top(hipStream_t s, uint32_t P, const fe* wpoly, const fe* zpoly, const fe* coef,
                         const fe* const* coef_of, const fe* tw_n, const Chal* chal, size_t n, size_t ps, fe* top) {
  launch("k_quotient_top", k_quotient_top, dim3(P), dim3(64), 0, s, wpoly, zpoly, coef, coef_of, tw_n, chal, n, ps, top);
}
inline void check_degree(hipStream_t s, uint32_t P, const fe* t, size_t m, size_t lo, uint32_t* flags) {
  launch("k_check_degree", k_check_degree, dim3(cdiv(m - (lo - 1), kThreads), P), dim3(kThreads), 0, s, t, m, lo, flags);
}

// ---- round 4 ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kEvalChunks = 16;
inline uint32_t small_len(size_t ps) { return kPowLow + cdiv(ps, kPowLow); }
// tables[q][k] = base_q^k, k < ps, from pw[q][b] = base_q^(2^b); small: count * small_len(ps) elements
inline void powers(hipStream_t s, uint32_t count, const fe* pw, fe* small, fe* tables, size_t ps) {
  const uint32_t sl = small_len(ps);
  launch("k_powers_small", k_powers_small, dim3(cdiv(sl, kThreads), count), dim3(kThreads), 0, s, small, sl, pw);
  launch("k_powers", k_powers, dim3(cdiv(ps, kThreads), count), dim3(kThreads), 0, s, tables, ps, ps, (const fe*)small, sl);
}
// out[e] = sum_k desc[e].poly[k] desc[e].pows[k], every desc[e].len <= max_len; partial: count * kEvalChunks elements
inline void evaluate(hipStream_t s, uint32_t count, const EvalDesc* desc, size_t max_len, fe* partial, fe* out) {
  uint32_t per_chunk = cdiv(max_len, kEvalChunks);
  launch("k_eval_partial", k_eval_partial, dim3(kEvalChunks, count), dim3(kThreads), 0, s, desc, partial, kEvalChunks,
         per_chunk);
  launch("k_eval_final", k_eval_final, dim3(count), dim3(64), 0, s, (const fe*)partial, kEvalChunks, out);
}

// ---- round 5 ---------------------------------------------------------------------------------------------------------
inline void lincomb(hipStream_t s, uint32_t P, const LinTerm* terms, uint32_t nterms, fe* out, size_t out_stride,
                    size_t out_len) {
  launch("k_lincomb", k_lincomb, dim3(cdiv(out_len, kThreads), P), dim3(kThreads), 0, s, terms, nterms, out, out_stride,
         out_len);
}
// quot[q] = f[q] / (X - a_q), q < count (k_div_prepare's table choice: q = proof * 2 + {zeta, zeta omega}).  f is
// overwritten by the suffix sums (its contents are dead once h is formed); tot: count * cdiv(len, kScanBlock) elements
inline void divide_linear(hipStream_t s, uint32_t count, fe* f, const fe* pows, size_t stride, size_t len, fe* h,
                          fe* tot, fe* quot) {
  launch("k_div_prepare", k_div_prepare, dim3(cdiv(len, kThreads), count), dim3(kThreads), 0, s, (const fe*)f, pows,
         stride, len, h);
  scan_exclusive<1, 1>(s, h, f, len, stride, count, tot);
  launch("k_div_finish", k_div_finish, dim3(cdiv(stride, kThreads), count), dim3(kThreads), 0, s, (const fe*)f, pows,
         stride, len, quot);
}

}  // namespace pk
}  // namespace cap
