// Drives the block verifier's kernels from k_verify_front through k_verify_affine (cap_amd/csrc/verify_kernels.hpp)
// directly and dumps every value between a block's proofs and its two sums, which the verifier itself never shows: the
// verdicts of capgpu_plonk_verify_block_* say nothing about a fold whose weights are all equal.  The kernels are out of
// the library's reach, so this program includes their header itself - built with the product's flags and with
// CAP_FL_SCHED and CAP_TD_NO_KERNELS as verify_dev.hip sets them - launches through verify_launch.hpp's fold_launch, the
// sequence verify_block runs, and builds its keys with vf::dev_vk_fill, as capgpu_plonk_vk_upload does.  It links
// libcapgpu.so for launch.hpp, msm_var_plan and msm_var_run.  Its copies of the kernels live in cap::vkcheck (CAP_VK_NS):
// under the library's names their handles would resolve to the library's, and the library's code would run.
//
//   verifycheck <cases.bin> <results.bin>
//
// cases.bin (little-endian, written by tests/verify_block_model.py): u64 magic, u64 ncases, then per case u64 count,
// nkeys, pub_stride, msg_bytes; nkeys capgpu_verifying_key; count x 4 u32 (key index, message offset, message length,
// 0); count capgpu_proof; count rows of pub_stride field elements; msg_bytes bytes.
// results.bin: u64 magic, u64 ncases, then per case u64 rc, count, points (15 count + 19 nkeys) and eight buffers, each
// followed by the kGuard bytes behind it: valid (count int), the u bytes (32 count), the scalars (34 count), S (32
// bytes), the weights (count), the gathered points and scalars (points each), A and -B.  Every buffer the kernels write
// starts as the sentinel byte 0xA5, its guard included.  rc: 0, the code of a failed launch or of msm_var_run, or
// kRefused when a case would address memory outside its buffers (checked on the host before anything is launched).
#define CAP_FL_SCHED 0
#define CAP_TD_NO_KERNELS
#define CAP_VK_NS vkcheck
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "capgpu.h"
#include "verify_launch.hpp"

using namespace cap;

namespace {

constexpr uint64_t kMagicIn = 0x5645524946434153ull, kMagicOut = 0x56455249464f5554ull;
constexpr uint64_t kRefused = 1000000;
constexpr uint64_t kMaxCount = 4096, kMaxKeys = 16, kMaxInputs = 1024, kMaxMsgBytes = 1 << 20;
constexpr size_t kGuard = 256;
constexpr uint8_t kSentinel = 0xA5;

#define HIP_OK(x)                                                                      \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      fprintf(stderr, "verifycheck: %s: %s\n", #x, hipGetErrorString(e_));            \
      return 2;                                                                        \
    }                                                                                  \
  } while (0)

struct Case {
  uint64_t count, nkeys, pub_stride, msg_bytes;
  std::vector<capgpu_verifying_key> keys;
  std::vector<uint32_t> meta;
  std::vector<capgpu_proof> proofs;
  std::vector<fe> pubs;
  std::vector<uint8_t> msgs;
};

struct DevBufs {
  std::vector<void*> all;
  ~DevBufs() {
    for (void* p : all) hipFree(p);
  }
  // `bytes` and a guard behind them, all sentinel
  void* take(size_t bytes, hipStream_t s) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes + kGuard) != hipSuccess) return nullptr;
    all.push_back(p);
    if (hipMemsetAsync(p, kSentinel, bytes + kGuard, s) != hipSuccess) return nullptr;
    return p;
  }
  void* upload(const void* src, size_t bytes, hipStream_t s) {
    void* p = take(bytes, s);
    if (p && bytes && hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return nullptr;
    return p;
  }
};

// every index a case's launches follow lies inside its buffers; the keys are well formed
bool in_bounds(const Case& c, std::vector<vf::DevVk>* keys) {
  if (!c.count || c.count > kMaxCount || !c.nkeys || c.nkeys > kMaxKeys || c.pub_stride > kMaxInputs ||
      c.msg_bytes > kMaxMsgBytes)
    return false;
  keys->resize(c.nkeys);
  for (uint64_t k = 0; k < c.nkeys; k++) {
    const uint64_t n = c.keys[k].domain_size;
    if (n < 4 || (n & (n - 1)) || n > ((uint64_t)1 << 28) || c.keys[k].num_inputs > n ||
        c.keys[k].num_inputs > c.pub_stride)
      return false;
    if (vf::dev_vk_fill(&c.keys[k], &(*keys)[k]) >= 0) return false;
  }
  for (uint64_t i = 0; i < c.count; i++) {
    const uint32_t* m = &c.meta[4 * i];
    if (m[0] >= c.nkeys || m[1] > c.msg_bytes || m[2] > c.msg_bytes - m[1]) return false;
  }
  return true;
}

struct Dumped {
  void* d;
  size_t bytes;
};

// the launches of one case; 0, 2 when the host side (allocation, upload) failed, 3 when the device did
int run_case(const Case& c, const std::vector<vf::DevVk>& keys, hipStream_t s, uint64_t* rc_out,
             std::vector<std::vector<uint8_t>>* dump) {
  const size_t count = c.count, nkeys = c.nkeys;
  DevBufs b;
#define NEED(ptr) \
  if (!(ptr)) return 2
  uint32_t max_msg = 0;
  for (size_t i = 0; i < count; i++) max_msg = std::max(max_msg, c.meta[4 * i + 2]);
  const size_t pre_stride = ((size_t)max_msg + vf::kPrefixBytes + 32 * c.pub_stride + 15) / 16 * 16;  // as verify_block
  const size_t msm_pts = vf::kOwnTerms * count + vf::kKeyTerms * nkeys;
  vf::DevVk* d_keyrecs = (vf::DevVk*)b.upload(keys.data(), sizeof(vf::DevVk) * nkeys, s);
  NEED(d_keyrecs);
  std::vector<const vf::DevVk*> keytab(nkeys);
  for (size_t k = 0; k < nkeys; k++) keytab[k] = d_keyrecs + k;
  const MsmVarDesc desc[2] = {{0, 0, (uint32_t)(vf::kATerms * count)},
                              {(uint64_t)(vf::kATerms * count), (uint32_t)(vf::kATerms * count),
                               (uint32_t)(msm_pts - vf::kATerms * count)}};
  const MsmVarPlan pl = msm_var_plan(desc[1].n, msm_pts, 2);
  void* d_keys = b.upload(keytab.data(), sizeof(void*) * nkeys, s);
  void* d_meta = b.upload(c.meta.data(), 16 * count, s);
  void* d_proofs = b.upload(c.proofs.data(), sizeof(capgpu_proof) * count, s);
  void* d_pubs = b.upload(c.pubs.data(), sizeof(fe) * c.pubs.size(), s);
  void* d_msgs = b.upload(c.msgs.data(), c.msgs.size(), s);
  void* d_desc = b.upload(desc, sizeof desc, s);
  void *d_state = b.take(64 * count, s), *d_pre = b.take(pre_stride * count, s),
       *d_app = b.take((size_t)vf::kAppBytes * count, s), *d_sums = b.take(sizeof(g1_jac) * 2, s),
       *d_ws = b.take(pl.workspace_bytes, s);
  NEED(d_keys && d_meta && d_proofs && d_pubs && d_msgs && d_desc && d_state && d_pre && d_app && d_sums && d_ws);
  const Dumped out[8] = {{b.take(sizeof(int) * count, s), sizeof(int) * count},
                         {b.take(32 * count, s), 32 * count},
                         {b.take(sizeof(fe) * vf::kTerms * count, s), sizeof(fe) * vf::kTerms * count},
                         {b.take(32, s), 32},
                         {b.take(sizeof(fe) * count, s), sizeof(fe) * count},
                         {b.take(sizeof(g1_affine) * msm_pts, s), sizeof(g1_affine) * msm_pts},
                         {b.take(sizeof(fe) * msm_pts, s), sizeof(fe) * msm_pts},
                         {b.take(sizeof(g1_affine) * 2, s), sizeof(g1_affine) * 2}};
  for (const Dumped& o : out) NEED(o.d);
  const vkcheck::FrontArgs fa{(const uint8_t*)d_proofs, (const fe*)d_pubs, (const vf::DevVk* const*)d_keys,
                              (const uint32_t*)d_meta, (const uint8_t*)d_msgs, (uint8_t*)d_state, (uint8_t*)d_pre,
                              (uint8_t*)d_app, (uint8_t*)out[1].d, (int*)out[0].d, (fe*)out[2].d, (uint32_t)c.pub_stride,
                              (uint32_t)pre_stride, (uint32_t)count};
  const vkcheck::FoldArgs fold{fa, (uint32_t)nkeys, (uint8_t*)out[3].d, (fe*)out[4].d, (g1_affine*)out[5].d, (fe*)out[6].d,
                               (const MsmVarDesc*)d_desc, (g1_jac*)d_sums, d_ws, pl.workspace_bytes, (g1_affine*)out[7].d};
#undef NEED
  int rc = vkcheck::fold_launch(fold, s);
  LaunchError& le = launch_error();
  if (le.code != hipSuccess) {
    fprintf(stderr, "verifycheck: launch of %s failed\n", le.kernel ? le.kernel : "?");
    rc = (int)le.code;
    le = LaunchError{};
  }
  // the buffers go when b leaves scope: wait for the launches first (keytab and desc are host arrays of this frame)
  if (hipStreamSynchronize(s) != hipSuccess) return 3;
  *rc_out = (uint64_t)(int64_t)rc;
  dump->clear();
  for (const Dumped& o : out) {
    dump->emplace_back(o.bytes + kGuard);
    if (hipMemcpy(dump->back().data(), o.d, o.bytes + kGuard, hipMemcpyDeviceToHost) != hipSuccess) return 3;
  }
  return 0;
}

template <class T>
bool read_vec(FILE* f, std::vector<T>* v, size_t k) {
  v->resize(k);
  return k == 0 || fread(v->data(), sizeof(T), k, f) == k;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: verifycheck <cases.bin> <results.bin>\n");
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fi ? fopen(argv[2], "wb") : nullptr;
  if (!fi || !fo) {
    fprintf(stderr, "verifycheck: cannot open the case or the result file\n");
    return 2;
  }
  uint64_t head[2];
  if (fread(head, 8, 2, fi) != 2 || head[0] != kMagicIn) {
    fprintf(stderr, "verifycheck: not a case file\n");
    return 2;
  }
  const uint64_t ncases = head[1];
  int dev = 0;
  if (capgpu_init(&dev, 1) != CAPGPU_OK) {
    fprintf(stderr, "verifycheck: capgpu_init: %s\n", capgpu_last_error());
    return 2;
  }
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  const uint64_t out_head[2] = {kMagicOut, ncases};
  fwrite(out_head, 8, 2, fo);

  for (uint64_t ci = 0; ci < ncases; ci++) {
    Case c;
    uint64_t h[4];
    if (fread(h, 8, 4, fi) != 4 || h[0] > kMaxCount || h[1] > kMaxKeys || h[2] > kMaxInputs || h[3] > kMaxMsgBytes) {
      fprintf(stderr, "verifycheck: case %llu: bad header\n", (unsigned long long)ci);
      return 2;
    }
    c.count = h[0], c.nkeys = h[1], c.pub_stride = h[2], c.msg_bytes = h[3];
    if (!read_vec(fi, &c.keys, c.nkeys) || !read_vec(fi, &c.meta, 4 * c.count) || !read_vec(fi, &c.proofs, c.count) ||
        !read_vec(fi, &c.pubs, c.count * c.pub_stride) || !read_vec(fi, &c.msgs, c.msg_bytes)) {
      fprintf(stderr, "verifycheck: case %llu: short read\n", (unsigned long long)ci);
      return 2;
    }
    const size_t msm_pts = vf::kOwnTerms * c.count + vf::kKeyTerms * c.nkeys;
    const size_t sizes[8] = {sizeof(int) * c.count, 32 * c.count, sizeof(fe) * vf::kTerms * c.count, 32,
                             sizeof(fe) * c.count, sizeof(g1_affine) * msm_pts, sizeof(fe) * msm_pts,
                             sizeof(g1_affine) * 2};
    uint64_t rc = kRefused;
    std::vector<std::vector<uint8_t>> dump;
    std::vector<vf::DevVk> keys;
    if (in_bounds(c, &keys)) {
      const int r = run_case(c, keys, stream, &rc, &dump);
      if (r == 3) {  // a fault: nothing more is started on the device
        fprintf(stderr, "verifycheck: case %llu: %s\n", (unsigned long long)ci, hipGetErrorString(hipGetLastError()));
        return 3;
      }
      if (r) {
        fprintf(stderr, "verifycheck: case %llu: allocation or upload failed\n", (unsigned long long)ci);
        return 2;
      }
    } else {
      for (size_t k = 0; k < 8; k++) dump.emplace_back(sizes[k] + kGuard, kSentinel);
    }
    const uint64_t rec[3] = {rc, c.count, (uint64_t)msm_pts};
    fwrite(rec, 8, 3, fo);
    for (const auto& d : dump) fwrite(d.data(), 1, d.size(), fo);
  }
  fclose(fi);
  if (fclose(fo) != 0) return 2;
  hipStreamDestroy(stream);
  capgpu_shutdown();
  return 0;
}
