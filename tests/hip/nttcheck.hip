// Drives the NTT's addressing forms (NttIo) and the 3 * 2^k transforms of cap_amd/csrc/ntt.hpp directly - none of them can
// be reached from the C ABI - in the code the product ships: this program links libcapgpu.so and calls cap::ntt_run,
// cap::ntt3_forward and cap::ntt3_inverse there; it compiles no kernel of its own.
//
//   nttcheck <cases.bin> <results.bin>
//
// cases.bin (little-endian, written by tests/ntt_io_model.py):  u64 magic, u64 ncases, then per case a header of
// kHeaderWords u64 (CaseHeader below) followed by src_elems field elements (the source buffer), and pre_elems field
// elements (a caller pre-scale table, internal form).  The destination buffer of dst_elems elements is filled with the
// sentinel byte 0xA5 before the call (kinds that work in place copy the source into it), `data` is dst + dst_offset.
// results.bin: u64 magic, u64 ncases, then per case u64 rc, u64 dst_elems and the WHOLE destination buffer, gaps
// included.  rc: 0, the HIP error of the call, or kRefused when a case would address memory outside its buffers (checked
// on the host before anything is launched).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "capgpu.h"
#include "launch.hpp"
#include "ntt.hpp"

using namespace cap;

namespace {

constexpr uint64_t kMagicIn = 0x4e54544943415345ull, kMagicOut = 0x4e54544f55545055ull;
constexpr uint64_t kRefused = 1000000;
enum Kind : uint64_t { kNttRun = 0, kNtt3Forward = 1, kNtt3Inverse = 2, kNtt3RoundTrip = 3 };

struct CaseHeader {
  uint64_t kind, log_n, count, dir, coset;
  uint64_t src_elems, dst_elems, pre_elems, dst_offset;
  uint64_t src_outer, src_inner, src_len, src_group;
  uint64_t dst_outer, dst_inner, dst_group;
  uint64_t src_elem_stride, src_group2, src_inner2, dst_group2, dst_inner2, pre_inner, lazy_out;
};
constexpr size_t kHeaderWords = sizeof(CaseHeader) / 8;

#define HIP_OK(x)                                                                      \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "nttcheck: %s: %s\n", #x, hipGetErrorString(e_));               \
      return 2;                                                                        \
    }                                                                                  \
  } while (0)

NttIo io_of(const CaseHeader& h, const fe* src, const fe* pre) {
  NttIo io{};
  io.src = src;
  io.src_outer = h.src_outer;
  io.src_inner = h.src_inner;
  io.src_len = h.src_len;
  io.src_group = (uint32_t)h.src_group;
  io.dst_outer = h.dst_outer;
  io.dst_inner = h.dst_inner;
  io.dst_group = (uint32_t)h.dst_group;
  io.src_elem_stride = (uint32_t)h.src_elem_stride;
  io.src_group2 = (uint32_t)h.src_group2;
  io.src_inner2 = h.src_inner2;
  io.dst_group2 = (uint32_t)h.dst_group2;
  io.dst_inner2 = h.dst_inner2;
  io.pre_inner = h.pre_inner;
  io.pre_scale = h.pre_elems ? pre : nullptr;
  io.lazy_out = (int)h.lazy_out;
  return io;
}

// every element ntt_run(..., &io) reads or writes lies inside the buffers (the addressing of col_tile / row_tile)
bool ntt_run_in_bounds(const CaseHeader& h) {
  const uint64_t n = 1ull << h.log_n;
  const uint64_t sg_ = std::max<uint64_t>(h.src_group, 1), dg_ = std::max<uint64_t>(h.dst_group, 1);
  const uint64_t sg2 = std::max<uint64_t>(h.src_group2, 1), dg2 = std::max<uint64_t>(h.dst_group2, 1);
  const uint64_t es = std::max<uint64_t>(h.src_elem_stride, 1);
  if (h.dst_offset > h.dst_elems) return false;
  for (uint64_t q = 0; q < h.count; q++) {
    const uint64_t q2 = q / sg_, a = q % sg_;
    const uint64_t base = (q2 / sg2) * h.src_outer + (sg2 > 1 ? (q2 % sg2) * h.src_inner2 : 0) + a * h.src_inner;
    const uint64_t off = es == 1 ? 0 : a * h.src_inner;  // position inside the source array of element 0
    // elements g < n with g * es + off < src_len are read, at base + g * es; their pre-scale factor at position + a * pre_inner
    if (h.src_len > off) {
      const uint64_t gmax = std::min<uint64_t>(n - 1, (h.src_len - off - 1) / es);
      if (base + gmax * es >= h.src_elems) return false;
      if (h.pre_elems && gmax * es + off + a * h.pre_inner >= h.pre_elems) return false;
    }
    const uint64_t o2 = q / dg_;
    const uint64_t ob = (o2 / dg2) * h.dst_outer + (dg2 > 1 ? (o2 % dg2) * h.dst_inner2 : 0) + (q % dg_) * h.dst_inner;
    if (h.dst_offset + ob + n > h.dst_elems) return false;
  }
  return true;
}

// ntt3_forward hands ntt_run 3 * count arrays: the caller's grouping one level up, three blocks of M per polynomial
bool ntt3_forward_in_bounds(const CaseHeader& h) {
  CaseHeader s = h;
  const uint64_t M = 1ull << h.log_n;
  if (h.src_len > M) return true;  // refused by ntt3_forward itself
  s.count = 3 * h.count;
  s.src_inner = 0;
  s.src_group = 3;
  s.src_group2 = std::max<uint64_t>(h.src_group, 1);
  s.src_inner2 = h.src_inner;
  s.dst_inner = M;
  s.dst_group = 3;
  s.dst_group2 = std::max<uint64_t>(h.dst_group, 1);
  s.dst_inner2 = h.dst_inner;
  s.src_elem_stride = 1;
  s.pre_elems = 0;
  return ntt_run_in_bounds(s);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: nttcheck <cases.bin> <results.bin>\n");
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fi ? fopen(argv[2], "wb") : nullptr;
  if (!fi || !fo) {
    fprintf(stderr, "nttcheck: cannot open the case or the result file\n");
    return 2;
  }
  uint64_t head[2];
  if (fread(head, 8, 2, fi) != 2 || head[0] != kMagicIn) {
    fprintf(stderr, "nttcheck: not a case file\n");
    return 2;
  }
  const uint64_t ncases = head[1];
  int dev = 0;
  if (capgpu_init(&dev, 1) != CAPGPU_OK) {
    fprintf(stderr, "nttcheck: capgpu_init: %s\n", capgpu_last_error());
    return 2;
  }
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  NttSmallTables small;
  if (int rc = ntt_build_small_tables(&small, stream)) {
    fprintf(stderr, "nttcheck: ntt_build_small_tables: %d\n", rc);
    return 2;
  }
  std::map<uint32_t, NttDomain> doms;
  std::map<uint32_t, Ntt3Domain> doms3;
  const uint64_t out_head[2] = {kMagicOut, ncases};
  fwrite(out_head, 8, 2, fo);

  for (uint64_t ci = 0; ci < ncases; ci++) {
    CaseHeader h;
    if (fread(&h, 8, kHeaderWords, fi) != kHeaderWords || h.log_n > 14 || h.count == 0 || h.count > 4096 ||
        h.src_elems > (1ull << 24) || h.dst_elems > (1ull << 24) || h.pre_elems > (1ull << 24) || h.kind > kNtt3RoundTrip) {
      fprintf(stderr, "nttcheck: case %llu: bad header\n", (unsigned long long)ci);
      return 2;
    }
    std::vector<fe> src(h.src_elems), pre(h.pre_elems), dst(h.dst_elems);
    if (fread(src.data(), sizeof(fe), h.src_elems, fi) != h.src_elems ||
        fread(pre.data(), sizeof(fe), h.pre_elems, fi) != h.pre_elems) {
      fprintf(stderr, "nttcheck: case %llu: short read\n", (unsigned long long)ci);
      return 2;
    }
    const uint32_t log_n = (uint32_t)h.log_n;
    const uint64_t n = 1ull << log_n, N = 3 * n;
    const bool three = h.kind != kNttRun;
    bool ok;
    if (h.kind == kNttRun) ok = ntt_run_in_bounds(h);
    else if (h.kind == kNtt3Inverse) ok = h.src_elems == h.dst_elems && h.dst_offset + h.count * N <= h.dst_elems;
    else ok = ntt3_forward_in_bounds(h);
    if (h.kind == kNtt3RoundTrip)  // the inverse runs in place on count contiguous arrays of N: the forward must have put them there
      ok = ok && h.dst_group <= 1 && h.dst_outer == N && h.dst_offset + h.count * N <= h.dst_elems;
    uint64_t rc = kRefused;
    memset(dst.data(), 0xA5, sizeof(fe) * h.dst_elems);
    if (h.kind == kNtt3Inverse) dst = src;
    if (ok) {
      if (!doms.count(log_n)) {
        NttDomain d;
        if (int r = ntt_build_domain(&d, log_n, stream)) {
          fprintf(stderr, "nttcheck: ntt_build_domain(%u): %d\n", log_n, r);
          return 2;
        }
        doms[log_n] = d;
      }
      if (three && !doms3.count(log_n)) {
        Ntt3Domain d;
        if (int r = ntt3_build_domain(&d, log_n, stream)) {
          fprintf(stderr, "nttcheck: ntt3_build_domain(%u): %d\n", log_n, r);
          return 2;
        }
        doms3[log_n] = d;
      }
      // scratch: count arrays of n (ntt_run through io), 3 M count (ntt3_forward), 6 M count (ntt3_inverse)
      const uint64_t scratch_elems = (three ? 6 : 1) * n * h.count;
      fe *d_src = nullptr, *d_dst = nullptr, *d_pre = nullptr, *d_scratch = nullptr;
      HIP_OK(hipMalloc(&d_src, sizeof(fe) * std::max<uint64_t>(h.src_elems, 1)));
      HIP_OK(hipMalloc(&d_dst, sizeof(fe) * std::max<uint64_t>(h.dst_elems, 1)));
      HIP_OK(hipMalloc(&d_pre, sizeof(fe) * std::max<uint64_t>(h.pre_elems, 1)));
      HIP_OK(hipMalloc(&d_scratch, sizeof(fe) * scratch_elems));
      HIP_OK(hipMemcpyAsync(d_src, src.data(), sizeof(fe) * h.src_elems, hipMemcpyHostToDevice, stream));
      HIP_OK(hipMemcpyAsync(d_dst, dst.data(), sizeof(fe) * h.dst_elems, hipMemcpyHostToDevice, stream));
      HIP_OK(hipMemcpyAsync(d_pre, pre.data(), sizeof(fe) * h.pre_elems, hipMemcpyHostToDevice, stream));
      fe* data = d_dst + h.dst_offset;
      const NttIo io = io_of(h, d_src, d_pre);
      int r = 0;
      if (h.kind == kNttRun) {
        r = ntt_run(doms[log_n], small, data, d_scratch, n, (uint32_t)h.count, (int)h.dir, (int)h.coset, stream, &io);
      } else if (h.kind == kNtt3Inverse) {
        r = ntt3_inverse(doms3[log_n], doms[log_n], small, data, (uint32_t)h.count, d_scratch, stream);
      } else {
        r = ntt3_forward(doms3[log_n], doms[log_n], small, data, io, (uint32_t)h.count, d_scratch, stream);
        if (!r && h.kind == kNtt3RoundTrip)
          r = ntt3_inverse(doms3[log_n], doms[log_n], small, data, (uint32_t)h.count, d_scratch, stream);
      }
      hipError_t es = hipStreamSynchronize(stream);
      LaunchError& le = launch_error();
      if (!r && le.code != hipSuccess) {
        fprintf(stderr, "nttcheck: case %llu: launch of %s failed\n", (unsigned long long)ci, le.kernel ? le.kernel : "?");
        r = (int)le.code;
        le = LaunchError{};
      }
      if (es != hipSuccess) {  // a fault: nothing more is started on the device
        fprintf(stderr, "nttcheck: case %llu: %s\n", (unsigned long long)ci, hipGetErrorString(es));
        return 3;
      }
      HIP_OK(hipMemcpy(dst.data(), d_dst, sizeof(fe) * h.dst_elems, hipMemcpyDeviceToHost));
      hipFree(d_src);
      hipFree(d_dst);
      hipFree(d_pre);
      hipFree(d_scratch);
      rc = (uint64_t)(int64_t)r;
    }
    const uint64_t rec[2] = {rc, h.dst_elems};
    fwrite(rec, 8, 2, fo);
    fwrite(dst.data(), sizeof(fe), h.dst_elems, fo);
  }
  fclose(fi);
  if (fclose(fo) != 0) return 2;
  for (auto& kv : doms) ntt_free_domain(&kv.second);
  for (auto& kv : doms3) ntt3_free_domain(&kv.second);
  ntt_free_small_tables(&small);
  hipStreamDestroy(stream);
  capgpu_shutdown();
  return 0;
}
