// The functions of cap_amd/csrc/ntt_elem29.hpp on gfx950, built with the product's flags: one lane per record of
// elemcheck_ops.hpp - the stage butterflies singly, with given twiddle pairs, each element step, the combine bodies.
// tests/test_gpu_elemcheck.py compares every output word with the host twin's (tests/cpp/ntt_elem_check.cpp elem).
// The kernel holds no assert, trap or printf.  usage: elemcheck <records> <results>; every HIP call's status is checked.
#include <hip/hip_runtime.h>

#include "elemcheck_ops.hpp"

using namespace cap;

#define EC_HIP(call)                                                                             \
  do {                                                                                           \
    const hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                      \
      fprintf(stderr, "elemcheck: %s failed: %s\n", #call, hipGetErrorString(e_));               \
      exit(3);                                                                                   \
    }                                                                                            \
  } while (0)

constexpr int kLanes = 64;

__global__ __launch_bounds__(kLanes) void k_elem(const ElemRec* __restrict__ in, ElemOut* __restrict__ out,
                                                uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  ElemOut o;
  elem_apply<Fr29>(in[i], o);  // Fr29 as ntt.hip has it: the translation unit's default schedule
  out[i] = o;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: elemcheck <records> <results>\n");
    return 3;
  }
  const std::vector<ElemRec> recs = elem_read(argv[1]);
  std::vector<ElemOut> outs(recs.size());
  const uint32_t n = (uint32_t)recs.size();
  if (n) {
    EC_HIP(hipSetDevice(0));
    ElemRec* d_in = nullptr;
    ElemOut* d_out = nullptr;
    EC_HIP(hipMalloc(&d_in, recs.size() * sizeof(ElemRec)));
    EC_HIP(hipMalloc(&d_out, outs.size() * sizeof(ElemOut)));
    EC_HIP(hipMemcpy(d_in, recs.data(), recs.size() * sizeof(ElemRec), hipMemcpyHostToDevice));
    EC_HIP(hipMemset(d_out, 0xff, outs.size() * sizeof(ElemOut)));
    hipLaunchKernelGGL(k_elem, dim3((n + kLanes - 1) / kLanes), dim3(kLanes), 0, 0, d_in, d_out, n);
    EC_HIP(hipGetLastError());
    EC_HIP(hipDeviceSynchronize());
    EC_HIP(hipMemcpy(outs.data(), d_out, outs.size() * sizeof(ElemOut), hipMemcpyDeviceToHost));
    EC_HIP(hipFree(d_in));
    EC_HIP(hipFree(d_out));
  }
  elem_write(argv[2], outs);
  fprintf(stderr, "elemcheck: %u records\n", n);
  return 0;
}
