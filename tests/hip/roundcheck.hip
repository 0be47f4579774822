// Drives the O(n) kernels of the five prover rounds (cap_amd/csrc/plonk_kernels.hpp) directly, on inputs a proof never
// presents: chosen challenges, tables the kernels did not make, values at the edges of each input's contract.  This
// program compiles the kernels itself: it includes plonk_kernels.hpp - built with the product's flags and with
// CAP_FL_SCHED as plonk.hip sets it, so it needs no export from the library - and launches through
// round_launch.hpp, the geometry the prover uses.  It links libcapgpu.so for what launch.hpp needs.
//
//   roundcheck <cases.bin> <results.bin>
//
// cases.bin (little-endian, written by tests/round_model.py): u64 magic, u64 ncases, then per case kHeaderWords u64 -
// kind, nin, dst_elems, dst_init, p[0 .. 19] - followed by nin input buffers, each u64 elems and elems field elements
// (32 bytes; structures travel as field elements too: a Chal is 6, a QuotConst 14, records of offsets are 4 u64).  The
// destination buffer of dst_elems elements is filled with the sentinel byte 0xA5 before the launches (dst_init: it
// starts as a copy of input 0, for the kernels that work in place).
// results.bin: u64 magic, u64 ncases, then per case u64 rc, u64 dst_elems and the WHOLE destination buffer, gaps
// included.  rc: 0, the HIP error of a launch, or kRefused when a case would address memory outside its buffers (checked
// on the host before anything is launched).
#define CAP_FL_SCHED 1
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "capgpu.h"
#include "round_launch.hpp"

using namespace cap;
using namespace cap::pk;

namespace {

constexpr uint64_t kMagicIn = 0x524f554e44434153ull, kMagicOut = 0x524f554e444f5554ull;
constexpr uint64_t kRefused = 1000000;
constexpr uint64_t kMaxElems = 1ull << 22;  // 128 MB: far above any case, far below the device
enum Kind : uint64_t {
  kScan = 0, kPerm, kKx, kQuot, kQuotTop, kDegree, kPowers, kEval, kLincomb, kDivide, kPadCopy, kBlind, kStage, kKinds
};
constexpr size_t kParams = 20, kHeaderWords = 4 + kParams;
struct CaseHeader {
  uint64_t kind, nin, dst_elems, dst_init, p[kParams];
};
static_assert(sizeof(CaseHeader) == 8 * kHeaderWords, "header layout");
static_assert(sizeof(Chal) == 6 * sizeof(fe) && sizeof(QuotConst) == 14 * sizeof(fe), "structures as field elements");

#define HIP_OK(x)                                                                      \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "roundcheck: %s: %s\n", #x, hipGetErrorString(e_));             \
      return 2;                                                                        \
    }                                                                                  \
  } while (0)

struct Rec {  // a record of offsets, one field element wide
  uint64_t a, b, c, d;
};
static_assert(sizeof(Rec) == sizeof(fe), "record width");

struct Case {
  CaseHeader h;
  std::vector<std::vector<fe>> in;
  size_t len(size_t i) const { return i < in.size() ? in[i].size() : 0; }
  const Rec* recs(size_t i) const { return reinterpret_cast<const Rec*>(in[i].data()); }
};

bool pow2(uint64_t x) { return x && !(x & (x - 1)); }

// ---- bounds: every element a case's launches read or write lies inside its buffers --------------------------------
// (small: every size is at most kMaxElems, so the products below cannot wrap)
bool in_bounds(const Case& c) {
  const uint64_t* p = c.h.p;
  const uint64_t D = c.h.dst_elems;
  for (size_t i = 0; i < kParams; i++)
    if (p[i] > kMaxElems) return false;
  switch (c.h.kind) {
    case kScan: {  // op, rev, len, stride, batch
      const uint64_t len = p[2], stride = p[3], batch = p[4];
      if (p[0] > 1 || p[1] > 1 || !len || !batch || len > stride) return false;
      const uint64_t need = (batch - 1) * stride + len;
      return c.len(0) >= need && D >= need;
    }
    case kPerm: {  // n, P, per_key, zstride, inv_on_device
      const uint64_t n = p[0], P = p[1], per_key = p[2], zs = p[3];
      if (!n || !P || zs < n) return false;
      return c.len(0) >= P * 5 * n && c.len(1) >= (per_key ? P : 1) * 5 * n && c.len(2) >= n && c.len(3) >= 6 * P &&
             c.len(4) >= 14 && (p[4] || c.len(5) >= P) && D >= P * zs + 8 + P + 8 + 2 * P * n;
    }
    case kKx:  // m
      return p[0] && c.len(0) >= p[0] && c.len(1) >= 14 && D >= 4 * p[0];
    case kQuot: {  // m, P, five, forms (1: folded, 2: direct, 3: folded then direct), only_unfoldable, per_key
      const uint64_t m = p[0], P = p[1], per_key = p[5];
      if (!m || m % 6 || !pow2(m / 3) || m / 3 < 4 || !P || p[2] > 1 || !p[3] || p[3] > 3 || p[4] > 1) return false;
      return c.len(0) >= (per_key ? P : 1) * kPkcCols * m && c.len(1) >= P * 6 * m && c.len(2) >= m && c.len(3) >= m &&
             c.len(4) >= 6 * P && c.len(5) >= 14 && D >= P * m;
    }
    case kQuotTop: {  // n, ps, P, per_key
      const uint64_t n = p[0], ps = p[1], P = p[2], per_key = p[3];
      if (n < 8 || ps < n + 3 || !P) return false;
      return c.len(0) >= P * 5 * ps && c.len(1) >= P * ps && c.len(2) >= (per_key ? P : 1) * 18 * ps && c.len(3) >= n &&
             c.len(4) >= 6 * P && D >= 8 * P;
    }
    case kDegree:  // m, lo, P
      return p[1] >= 1 && p[1] <= p[0] && p[2] && c.len(0) >= p[2] * p[0] && D >= p[2];
    case kPowers:  // ps, count
      return p[0] && p[0] <= (1ull << 24) - 65536 && p[1] && c.len(0) >= 24 * p[1] && D >= p[0] * p[1];
    case kEval: {  // count, max_len;  in 0: polynomials, 1: power tables, 2: count records (poly offset, table offset, len)
      const uint64_t count = p[0], max_len = p[1];
      if (!count || !max_len || c.len(2) < count || D < count) return false;
      for (uint64_t e = 0; e < count; e++) {
        const Rec& r = c.recs(2)[e];
        if (r.c > max_len || r.a > kMaxElems || r.b > kMaxElems || r.a + r.c > c.len(0) || r.b + r.c > c.len(1)) return false;
      }
      return true;
    }
    case kLincomb: {  // P, nterms, out_stride, out_len;  in 0: polynomials, 1: P * nterms pairs (scalar; poly offset, len)
      const uint64_t P = p[0], nt = p[1], os = p[2], ol = p[3];
      if (!P || !nt || !ol || ol > os || c.len(1) < 2 * P * nt || D < (P - 1) * os + ol) return false;
      for (uint64_t t = 0; t < P * nt; t++) {
        const Rec& r = c.recs(1)[2 * t + 1];
        if (r.a > kMaxElems || r.b > kMaxElems || r.a + std::min(r.b, ol) > c.len(0)) return false;
      }
      return true;
    }
    case kDivide: {  // len, stride, count
      const uint64_t len = p[0], stride = p[1], count = p[2];
      if (!len || len > stride || !count || count % 2) return false;
      return c.len(0) >= count * stride && c.len(1) >= count / 2 * 4 * stride && D >= count * stride;
    }
    case kPadCopy: {  // dst_outer, dst_inner, src_outer, src_inner, inner, count, len, total
      const uint64_t inner = p[4], count = p[5], len = p[6], total = p[7];
      if (!inner || !count || !total || count > 65535) return false;
      for (uint64_t q = 0; q < count; q++) {
        if ((q / inner) * p[0] + (q % inner) * p[1] + total > D) return false;
        if (len && (q / inner) * p[2] + (q % inner) * p[3] + std::min(len, total) > c.len(0)) return false;
      }
      return true;
    }
    case kBlind: {  // set_tail, stride, n, inner, bl_off, nb, count  (in place: dst starts as input 0)
      const uint64_t stride = p[1], n = p[2], inner = p[3], nb = p[5], count = p[6];
      if (p[0] > 1 || !inner || !count || nb > 64 || n + nb > stride || !c.h.dst_init || count * stride > D) return false;
      const uint64_t q = count - 1;  // the largest blinder index is reached by the last proof's last column
      uint64_t top = 0;
      for (uint64_t r = q - std::min(q, inner - 1); r <= q; r++) top = std::max(top, (r / inner) * 13 + p[4] + (r % inner) * nb + nb);
      return c.len(1) >= top;
    }
    case kStage: {  // src_stride, n, inner, bl_off, nb, count
      const uint64_t ss = p[0], n = p[1], inner = p[2], nb = p[4], count = p[5];
      if (!inner || !count || count > 65535 || !n || n > ss) return false;
      uint64_t top = 0;
      for (uint64_t r = 0; r < count; r++) top = std::max(top, (r / inner) * 13 + p[3] + (r % inner) * nb + nb);
      return c.len(0) >= (count - 1) * ss + n && c.len(1) >= top && D >= count * (n + nb);
    }
  }
  return false;
}

struct DevBufs {
  std::vector<void*> all;
  ~DevBufs() {
    for (void* p : all) hipFree(p);
  }
  template <class T>
  T* take(size_t k) {
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(T) * std::max<size_t>(k, 1)) != hipSuccess) return nullptr;
    all.push_back(p);
    return (T*)p;
  }
};

template <class T>
T* upload(DevBufs& b, const T* src, size_t k, hipStream_t s) {
  T* d = b.take<T>(k);
  if (d && k && hipMemcpyAsync(d, src, sizeof(T) * k, hipMemcpyHostToDevice, s) != hipSuccess) return nullptr;
  return d;
}

// a table of per-proof pointers base + p * each (device memory), or null
const fe* const* pointer_table(DevBufs& b, const fe* base, size_t each, uint64_t P, bool wanted, hipStream_t s,
                               std::vector<std::vector<const fe*>>& keep) {
  if (!wanted) return nullptr;
  keep.emplace_back(P);
  for (uint64_t p = 0; p < P; p++) keep.back()[p] = base + p * each;
  return upload(b, keep.back().data(), P, s);
}

template <int OP>
void scan_either(hipStream_t s, bool rev, const fe* in, fe* out, size_t len, size_t stride, uint32_t batch, fe* tot) {
  if (rev) scan_exclusive<OP, 1>(s, in, out, len, stride, batch, tot);
  else scan_exclusive<OP, 0>(s, in, out, len, stride, batch, tot);
}

// the launches of one case; 0, or 2 when the host side (allocation, upload) failed
int run_case(const Case& c, fe* d_dst, hipStream_t s) {
  const uint64_t* p = c.h.p;
  DevBufs b;
  std::vector<fe*> in;
  std::vector<std::vector<const fe*>> keep;
  for (auto& v : c.in) {
    in.push_back(upload(b, v.data(), v.size(), s));
    if (!in.back()) return 2;
  }
#define NEED(ptr) \
  if (!(ptr)) return 2
  switch (c.h.kind) {
    case kScan: {
      fe* tot = b.take<fe>(p[4] * cdiv(p[2], kScanBlock));
      NEED(tot);
      if (p[0] == 0) scan_either<0>(s, p[1], in[0], d_dst, p[2], p[3], (uint32_t)p[4], tot);
      else scan_either<1>(s, p[1], in[0], d_dst, p[2], p[3], (uint32_t)p[4], tot);
      break;
    }
    case kPerm: {
      const size_t n = p[0], zs = p[3];
      const uint32_t P = (uint32_t)p[1];
      const uint32_t nb = cdiv(n, kScanBlock);
      fe *pre = b.take<fe>(P * n), *sfx = b.take<fe>(P * n), *tot = b.take<fe>((size_t)2 * P * nb);
      NEED(pre && sfx && tot);
      const fe* const* sig_of = pointer_table(b, in[1], 5 * n, P, p[2], s, keep);
      NEED(!p[2] || sig_of);
      QuotConst qc;
      memcpy(&qc, c.in[4].data(), sizeof(qc));
      fe *z = d_dst, *total = d_dst + P * zs + 8, *num = total + P + 8, *den = num + (size_t)P * n;
      perm_numden(s, in[0], in[1], sig_of, in[2], (const Chal*)in[3], qc, n, P, num, den);
      scan_exclusive<0, 0>(s, num, pre, n, n, P, tot);
      scan_exclusive<0, 1>(s, den, sfx, n, n, P, tot + (size_t)P * nb);
      if (p[4]) {
        perm_inv_total(s, sfx, den, n, total, P);
        perm_finish(s, pre, sfx, den, total, n, P, z, zs);
      } else {  // the host's inverse of the total arrives with the case
        perm_total(s, sfx, den, n, total, P);
        perm_finish(s, pre, sfx, den, in[5], n, P, z, zs);
      }
      break;
    }
    case kKx: {
      QuotConst qc;
      memcpy(&qc, c.in[1].data(), sizeof(qc));
      kx_columns(s, d_dst, in[0], qc, p[0]);
      break;
    }
    case kQuot: {
      const size_t m = p[0];
      const uint32_t P = (uint32_t)p[1], five = (uint32_t)p[2];
      const size_t pts = five ? m - m / 6 : m;
      const fe* const* pkc_of = pointer_table(b, in[0], kPkcCols * m, P, p[5], s, keep);
      NEED(!p[5] || pkc_of);
      QuotConst qc;
      memcpy(&qc, c.in[5].data(), sizeof(qc));
      if (p[3] & 1) quotient<true>(s, P, pts, in[0], pkc_of, in[1], in[2], in[3], (const Chal*)in[4], qc, m, 1u, five, d_dst);
      if (p[3] & 2)
        quotient<false>(s, P, pts, in[0], pkc_of, in[1], in[2], in[3], (const Chal*)in[4], qc, m, (uint32_t)p[4], five, d_dst);
      break;
    }
    case kQuotTop: {
      const fe* const* coef_of = pointer_table(b, in[2], 18 * p[1], p[2], p[3], s, keep);
      NEED(!p[3] || coef_of);
      quotient_top(s, (uint32_t)p[2], in[0], in[1], in[2], coef_of, in[3], (const Chal*)in[4], p[0], p[1], d_dst);
      break;
    }
    case kDegree: {
      const uint32_t P = (uint32_t)p[2];
      uint32_t* flags = b.take<uint32_t>(P);
      NEED(flags);
      if (hipMemsetAsync(flags, 0, 4 * P, s) != hipSuccess) return 2;
      check_degree(s, P, in[0], p[0], p[1], flags);
      // flag p -> word 0 of element p of the destination, the other seven words zero
      if (hipMemsetAsync(d_dst, 0, sizeof(fe) * P, s) != hipSuccess ||
          hipMemcpy2DAsync(d_dst, sizeof(fe), flags, 4, 4, P, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return 2;
      break;
    }
    case kPowers: {
      fe* small = b.take<fe>(p[1] * small_len(p[0]));
      NEED(small);
      powers(s, (uint32_t)p[1], in[0], small, d_dst, p[0]);
      break;
    }
    case kEval: {
      std::vector<EvalDesc> ed(p[0]);
      for (uint64_t e = 0; e < p[0]; e++) {
        const Rec& r = c.recs(2)[e];
        ed[e] = EvalDesc{in[0] + r.a, in[1] + r.b, (uint32_t)r.c, 0};
      }
      EvalDesc* d_ed = upload(b, ed.data(), ed.size(), s);
      fe* partial = b.take<fe>(p[0] * kEvalChunks);
      NEED(d_ed && partial);
      if (hipStreamSynchronize(s) != hipSuccess) return 2;  // ed leaves scope
      evaluate(s, (uint32_t)p[0], d_ed, p[1], partial, d_dst);
      break;
    }
    case kLincomb: {
      std::vector<LinTerm> T(p[0] * p[1]);
      for (size_t t = 0; t < T.size(); t++) {
        const Rec& r = c.recs(1)[2 * t + 1];
        T[t] = LinTerm{};
        T[t].poly = in[0] + r.a;
        T[t].scalar = c.in[1][2 * t];
        T[t].len = (uint32_t)r.b;
      }
      LinTerm* d_T = upload(b, T.data(), T.size(), s);
      NEED(d_T);
      if (hipStreamSynchronize(s) != hipSuccess) return 2;  // T leaves scope
      lincomb(s, (uint32_t)p[0], d_T, (uint32_t)p[1], d_dst, p[2], p[3]);
      break;
    }
    case kDivide: {
      fe *h = b.take<fe>(p[2] * p[1]), *tot = b.take<fe>(p[2] * cdiv(p[0], kScanBlock));
      NEED(h && tot);
      divide_linear(s, (uint32_t)p[2], in[0], in[1], p[1], p[0], h, tot, d_dst);
      break;
    }
    case kPadCopy:
      pad_copy(s, d_dst, p[0], p[1], in[0], p[2], p[3], (uint32_t)p[4], (uint32_t)p[5], p[6], p[7]);
      break;
    case kBlind:  // the prover's geometry: one workgroup of 64 per polynomial
      if (p[0])
        launch("k_blind", k_blind<1>, dim3((uint32_t)p[6]), dim3(64), 0, s, d_dst, (size_t)p[1], (size_t)p[2],
               (const fe*)in[1], (uint32_t)p[3], (uint32_t)p[4], (uint32_t)p[5], (uint32_t)p[6]);
      else
        launch("k_blind", k_blind<0>, dim3((uint32_t)p[6]), dim3(64), 0, s, d_dst, (size_t)p[1], (size_t)p[2],
               (const fe*)in[1], (uint32_t)p[3], (uint32_t)p[4], (uint32_t)p[5], (uint32_t)p[6]);
      break;
    case kStage:
      launch("k_stage_evals", k_stage_evals, dim3(cdiv(p[1] + p[4], kThreads), (uint32_t)p[5]), dim3(kThreads), 0, s,
             (const fe*)in[0], (size_t)p[0], (size_t)p[1], (const fe*)in[1], (uint32_t)p[2], (uint32_t)p[3],
             (uint32_t)p[4], d_dst);
      break;
  }
#undef NEED
  // the device buffers of this case are freed when b leaves scope: wait for the launches first
  return hipStreamSynchronize(s) == hipSuccess ? 0 : 3;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: roundcheck <cases.bin> <results.bin>\n");
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fi ? fopen(argv[2], "wb") : nullptr;
  if (!fi || !fo) {
    fprintf(stderr, "roundcheck: cannot open the case or the result file\n");
    return 2;
  }
  uint64_t head[2];
  if (fread(head, 8, 2, fi) != 2 || head[0] != kMagicIn) {
    fprintf(stderr, "roundcheck: not a case file\n");
    return 2;
  }
  const uint64_t ncases = head[1];
  int dev = 0;
  if (capgpu_init(&dev, 1) != CAPGPU_OK) {
    fprintf(stderr, "roundcheck: capgpu_init: %s\n", capgpu_last_error());
    return 2;
  }
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  const uint64_t out_head[2] = {kMagicOut, ncases};
  fwrite(out_head, 8, 2, fo);

  for (uint64_t ci = 0; ci < ncases; ci++) {
    Case c;
    if (fread(&c.h, 8, kHeaderWords, fi) != kHeaderWords || c.h.kind >= kKinds || c.h.nin > 8 || c.h.dst_elems > kMaxElems) {
      fprintf(stderr, "roundcheck: case %llu: bad header\n", (unsigned long long)ci);
      return 2;
    }
    for (uint64_t i = 0; i < c.h.nin; i++) {
      uint64_t elems;
      if (fread(&elems, 8, 1, fi) != 1 || elems > kMaxElems) {
        fprintf(stderr, "roundcheck: case %llu: bad buffer\n", (unsigned long long)ci);
        return 2;
      }
      c.in.emplace_back(elems);
      if (fread(c.in.back().data(), sizeof(fe), elems, fi) != elems) {
        fprintf(stderr, "roundcheck: case %llu: short read\n", (unsigned long long)ci);
        return 2;
      }
    }
    std::vector<fe> dst(c.h.dst_elems);
    memset(dst.data(), 0xA5, sizeof(fe) * c.h.dst_elems);
    const bool init_ok = !c.h.dst_init || (c.len(0) == c.h.dst_elems);
    if (c.h.dst_init && init_ok) dst = c.in[0];
    uint64_t rc = kRefused;
    if (init_ok && in_bounds(c)) {
      fe* d_dst = nullptr;
      HIP_OK(hipMalloc(&d_dst, sizeof(fe) * std::max<uint64_t>(c.h.dst_elems, 1)));
      HIP_OK(hipMemcpyAsync(d_dst, dst.data(), sizeof(fe) * c.h.dst_elems, hipMemcpyHostToDevice, stream));
      int r = run_case(c, d_dst, stream);
      LaunchError& le = launch_error();
      if (r == 3) {  // a fault: nothing more is started on the device
        fprintf(stderr, "roundcheck: case %llu (kind %llu): %s\n", (unsigned long long)ci, (unsigned long long)c.h.kind,
                hipGetErrorString(hipGetLastError()));
        return 3;
      }
      if (r) {
        fprintf(stderr, "roundcheck: case %llu: allocation or upload failed\n", (unsigned long long)ci);
        return 2;
      }
      if (le.code != hipSuccess) {
        fprintf(stderr, "roundcheck: case %llu: launch of %s failed\n", (unsigned long long)ci, le.kernel ? le.kernel : "?");
        r = (int)le.code;
        le = LaunchError{};
      }
      HIP_OK(hipMemcpy(dst.data(), d_dst, sizeof(fe) * c.h.dst_elems, hipMemcpyDeviceToHost));
      hipFree(d_dst);
      rc = (uint64_t)(int64_t)r;
    }
    const uint64_t rec[2] = {rc, c.h.dst_elems};
    fwrite(rec, 8, 2, fo);
    fwrite(dst.data(), sizeof(fe), c.h.dst_elems, fo);
  }
  fclose(fi);
  if (fclose(fo) != 0) return 2;
  hipStreamDestroy(stream);
  capgpu_shutdown();
  return 0;
}
