// Proofs between their 769 wire bytes and capgpu_proof on the device (K14 of DESIGN.md §4): what Proof::deserialize does
// when a note arrives as bytes (src/transfer.rs:54-66), for a whole block in one launch sequence.  The rule is
// proof_codec.hpp's, the one capgpu_proof_deserialize (params.hip) and capgpu_proof_serialize (verify.hip) follow on the host.
//   k_proof_decode         blocks [0, point_blocks): one lane per POINT, densely packed - lane g works on point g % 13 of
//                          proof g / 13 - so that whole wavefronts run the (p + 1) / 4 power with a wave-uniform exponent,
//                          as g1_decompress_kernel does; the blocks behind them: 11 lanes per proof, one per evaluation
//                          and one for the four length prefixes and the tag.  A lane whose field is malformed lowers the
//                          proof's status word (preset to all ones) to 1 + the field's offset.
//   k_proof_decode_finish  one wavefront per proof: status all ones -> 0; any other status -> the struct to all-ones words.
//   k_proof_encode         one lane per field of a proof (13 points, 10 evaluations, the frame): td::compress_g1 /
//                          td::serialize_fr into the record.
// Records sit at any byte address: every access to them is a byte access.
#define CAP_FL_SCHED 0
#define CAP_TD_NO_KERNELS
#include <string.h>

#include <vector>

#include "context.hpp"
#include "launch.hpp"
#include "proof_codec.hpp"

namespace cap {
namespace pc {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTailLanes = kScalars + 1;  // per proof: its evaluations, then the frame
constexpr uint32_t kEncodeLanes = kPoints + kScalars + 1;
constexpr size_t kMaxCount = (size_t)1 << 24;  // 13 lanes per proof stay far below 2^32

__global__ __launch_bounds__(kThreads) void k_proof_decode(const uint8_t* __restrict__ bytes, size_t stride, uint32_t count,
                                                           uint32_t point_blocks, uint8_t* __restrict__ proofs,
                                                           uint32_t* __restrict__ status, SqrtExp e) {
  if (blockIdx.x < point_blocks) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= count * kPoints) return;
    const uint32_t i = g / kPoints, k = g % kPoints, off = point_offset(k);
    g1_affine p;
    const bool ok = decode_point(bytes + (size_t)i * stride + off, e, &p);
    *(g1_affine*)(proofs + (size_t)i * td::kPrBytes + 64 * k) = p;
    if (!ok) atomicMin(&status[i], 1 + off);
    return;
  }
  const uint32_t g = (blockIdx.x - point_blocks) * kThreads + threadIdx.x;
  if (g >= count * kTailLanes) return;
  const uint32_t i = g / kTailLanes, k = g % kTailLanes;
  const uint8_t* rec = bytes + (size_t)i * stride;
  if (k < kScalars) {
    const uint32_t off = scalar_offset(k);
    fe v;
    const bool ok = decode_scalar(rec + off, &v);
    *(fe*)(proofs + (size_t)i * td::kPrBytes + td::kPrWireEvals + 32 * k) = v;
    if (!ok) atomicMin(&status[i], 1 + off);
  } else {
    const uint32_t st = frame_status(rec);
    if (st != kStatusUnset) atomicMin(&status[i], st);
  }
}

__global__ __launch_bounds__(64) void k_proof_decode_finish(uint32_t count, uint8_t* __restrict__ proofs,
                                                            uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  if (i >= count) return;
  const uint32_t st = status[i];
  __syncthreads();  // every lane has read the word lane 0 rewrites
  if (st == kStatusUnset) {
    if (t == 0) status[i] = 0;
    return;
  }
  uint4* w = (uint4*)(proofs + (size_t)i * td::kPrBytes);
  for (uint32_t k = t; k < td::kPrBytes / 16; k += 64) w[k] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

__global__ __launch_bounds__(kThreads) void k_proof_encode(const uint8_t* __restrict__ proofs, uint32_t count,
                                                           uint8_t* __restrict__ bytes, size_t stride) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= count * kEncodeLanes) return;
  const uint32_t i = g / kEncodeLanes, k = g % kEncodeLanes;
  const uint8_t* pr = proofs + (size_t)i * td::kPrBytes;
  uint8_t* rec = bytes + (size_t)i * stride;
  if (k < kPoints) {
    td::compress_g1(*(const g1_affine*)(pr + 64 * k), rec + point_offset(k));
  } else if (k < kPoints + kScalars) {
    td::serialize_fr(*(const fe*)(pr + td::kPrWireEvals + 32 * (k - kPoints)), rec + scalar_offset(k - kPoints));
  } else {
    encode_frame(rec);
  }
}

unsigned blocks_for(size_t lanes) { return (unsigned)((lanes + kThreads - 1) / kThreads); }

}  // namespace

int decode_launch(const uint8_t* d_bytes, size_t stride, size_t count, void* d_proofs, int* d_status, hipStream_t s) {
  const uint32_t n = (uint32_t)count;
  const unsigned point_blocks = blocks_for(count * kPoints), tail_blocks = blocks_for(count * kTailLanes);
  CAP_HIP(hipMemsetAsync(d_status, 0xff, sizeof(int) * count, s));
  launch("k_proof_decode", k_proof_decode, dim3(point_blocks + tail_blocks), dim3(kThreads), 0, s, d_bytes, stride, n,
         (uint32_t)point_blocks, (uint8_t*)d_proofs, (uint32_t*)d_status, sqrt_exponent());
  launch("k_proof_decode_finish", k_proof_decode_finish, dim3(n), dim3(64), 0, s, n, (uint8_t*)d_proofs,
         (uint32_t*)d_status);
  return take_launch_error();
}
int encode_launch(const void* d_proofs, size_t count, uint8_t* d_bytes, size_t stride, hipStream_t s) {
  launch("k_proof_encode", k_proof_encode, dim3(blocks_for(count * kEncodeLanes)), dim3(kThreads), 0, s,
         (const uint8_t*)d_proofs, (uint32_t)count, d_bytes, stride);
  return take_launch_error();
}

namespace {
bool bad_args(const char* who, const void* a, const void* b, const void* c, size_t stride, size_t count) {
  if (stride >= kBytes && count <= kMaxCount && (!count || (a && b && c))) return false;
  set_error("%s: bad argument (null pointer, stride %zu below %u, or more than 2^24 records)", who, stride, kBytes);
  return true;
}
// bytes the records span: the last one ends at its 769th byte
size_t span(size_t stride, size_t count) { return (count - 1) * stride + kBytes; }
}  // namespace

}  // namespace pc
}  // namespace cap

using namespace cap;

extern "C" {

int capgpu_proof_decode_batch_dev(const void* d_bytes, size_t stride, size_t count, void* d_proofs_out, int* d_status_out) {
  if (pc::bad_args("capgpu_proof_decode_batch_dev", d_bytes, d_proofs_out, d_status_out, stride, count))
    return CAPGPU_ERR_INVALID_ARG;
  CAP_CHECK_INIT();
  if (count == 0) return CAPGPU_OK;
  Context& c = ctx();
  Entry lk(c);
  return pc::decode_launch((const uint8_t*)d_bytes, stride, count, d_proofs_out, d_status_out, c.stream);
}

int capgpu_proof_decode_batch(const uint8_t* bytes, size_t stride, size_t count, capgpu_proof* proofs_out, int* status_out) {
  if (pc::bad_args("capgpu_proof_decode_batch", bytes, proofs_out, status_out, stride, count)) return CAPGPU_ERR_INVALID_ARG;
  CAP_CHECK_INIT();
  if (count == 0) return CAPGPU_OK;
  Context& c = ctx();
  Entry lk(c);
  // records, proofs and statuses side by side in the context's staging scratch
  const size_t in_bytes = pc::span(stride, count), o_proofs = (in_bytes + 255) / 256 * 256,
               o_status = o_proofs + sizeof(capgpu_proof) * count;
  int rc = scratch_reserve(c.stage_a, o_status + sizeof(int) * count);
  if (rc) return rc;
  char* d = (char*)c.stage_a.p;
  CAP_HIP(hipMemcpyAsync(d, bytes, in_bytes, hipMemcpyHostToDevice, c.stream));
  if ((rc = pc::decode_launch((const uint8_t*)d, stride, count, d + o_proofs, (int*)(d + o_status), c.stream))) return rc;
  CAP_HIP(hipMemcpyAsync(proofs_out, d + o_proofs, sizeof(capgpu_proof) * count, hipMemcpyDeviceToHost, c.stream));
  CAP_HIP(hipMemcpyAsync(status_out, d + o_status, sizeof(int) * count, hipMemcpyDeviceToHost, c.stream));
  CAP_HIP(hipStreamSynchronize(c.stream));
  return CAPGPU_OK;
}

int capgpu_proof_encode_batch_dev(const void* d_proofs, size_t count, void* d_bytes_out, size_t stride) {
  if (pc::bad_args("capgpu_proof_encode_batch_dev", d_proofs, d_bytes_out, d_bytes_out, stride, count))
    return CAPGPU_ERR_INVALID_ARG;
  CAP_CHECK_INIT();
  if (count == 0) return CAPGPU_OK;
  Context& c = ctx();
  Entry lk(c);
  return pc::encode_launch(d_proofs, count, (uint8_t*)d_bytes_out, stride, c.stream);
}

int capgpu_proof_encode_batch(const capgpu_proof* proofs, size_t count, uint8_t* bytes_out, size_t stride) {
  if (pc::bad_args("capgpu_proof_encode_batch", proofs, bytes_out, bytes_out, stride, count)) return CAPGPU_ERR_INVALID_ARG;
  CAP_CHECK_INIT();
  if (count == 0) return CAPGPU_OK;
  Context& c = ctx();
  Entry lk(c);
  // the records are written packed on the device and spread to the caller's stride on the way back, so that the bytes
  // between the caller's records stay what they were
  const size_t o_bytes = sizeof(capgpu_proof) * count;
  int rc = scratch_reserve(c.stage_a, o_bytes + (size_t)pc::kBytes * count);
  if (rc) return rc;
  char* d = (char*)c.stage_a.p;
  CAP_HIP(hipMemcpyAsync(d, proofs, sizeof(capgpu_proof) * count, hipMemcpyHostToDevice, c.stream));
  if ((rc = pc::encode_launch(d, count, (uint8_t*)(d + o_bytes), pc::kBytes, c.stream))) return rc;
  std::vector<uint8_t> packed((size_t)pc::kBytes * count);
  CAP_HIP(hipMemcpyAsync(packed.data(), d + o_bytes, packed.size(), hipMemcpyDeviceToHost, c.stream));
  CAP_HIP(hipStreamSynchronize(c.stream));
  for (size_t i = 0; i < count; i++) memcpy(bytes_out + i * stride, &packed[i * pc::kBytes], pc::kBytes);
  return CAPGPU_OK;
}

}  // extern "C"
