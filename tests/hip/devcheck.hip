// Device conformance check, gfx950 driver: the operation table of devcheck_ops.hpp in kernels built with the product's
// flags, one record per lane (one per quad - four real lanes, QuadDev - for the quad group).  The kernels hold no assert,
// trap or printf: bounds are checked afterwards from the raw limbs (tests/devcheck_vectors.py).
// usage: devcheck <vectors> <results>.  Every HIP call's status is checked; one synchronisation per group.
#include <hip/hip_runtime.h>

#include "devcheck_io.hpp"

using namespace devcheck;

#define DC_HIP(call)                                                                             \
  do {                                                                                           \
    const hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                      \
      fprintf(stderr, "devcheck: %s failed: %s\n", #call, hipGetErrorString(e_));                \
      exit(3);                                                                                   \
    }                                                                                            \
  } while (0)

constexpr int kLanes = 64;

template <int G>
__global__ __launch_bounds__(kLanes) void k_group(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                 uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t* r = in + (size_t)i * kInWords[G];
  uint32_t* o = out + (size_t)i * kOutWords[G];
  if constexpr (G == G_FIELD) run_field(r, o);
  else if constexpr (G == G_FIELD32) run_field32(r, o);
  else if constexpr (G == G_CURVE) run_curve(r, o);
  else run_tower(r, o);
}
__global__ __launch_bounds__(kLanes) void k_pair(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                uint32_t count, const p29::line_coeffs* __restrict__ lines,
                                                uint32_t nq) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  run_pair(in + (size_t)i * kInWords[G_PAIR], out + (size_t)i * kOutWords[G_PAIR], lines, nq);
}
// one wave = 16 quads; the records of a wave are mixed by the generator (infinity, P + P, P - P, ordinary)
__global__ __launch_bounds__(kLanes) void k_quad(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                uint32_t count) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, q = t >> 2;
  if (q >= count) return;  // whole quads leave: the last wave may be partial
  const uint32_t* r = in + (size_t)q * kInWords[G_QUAD];
  uint32_t* o = out + (size_t)q * kOutWords[G_QUAD];
  const bool writer = (t & 3) == 0;
  if (r[2] == 0) quad_ops<0, QuadDev>(r, o, QuadSlowT<G1LT<0>>(), writer);
  else if (r[2] == 1) quad_ops<1, QuadDev>(r, o, QuadSlowT<G1LT<1>>(), writer);
}

int main(int argc, char** argv) {
  if (argc != 3) die("usage: devcheck <vectors> <results>");
  const Vectors v = read_vectors(argv[1]);
  const std::vector<p29::line_coeffs> lines = prepare_all_lines(v);
  DC_HIP(hipSetDevice(0));
  p29::line_coeffs* d_lines = nullptr;
  if (!lines.empty()) {
    DC_HIP(hipMalloc(&d_lines, lines.size() * sizeof(p29::line_coeffs)));
    DC_HIP(hipMemcpy(d_lines, lines.data(), lines.size() * sizeof(p29::line_coeffs), hipMemcpyHostToDevice));
  }
  std::vector<uint32_t> out[G_COUNT];
  for (uint32_t g = 0; g < G_COUNT; g++) {
    const uint32_t n = v.count[g];
    out[g].assign((size_t)n * kOutWords[g], 0xffffffffu);
    if (n == 0) continue;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    const size_t in_bytes = v.in[g].size() * sizeof(uint32_t), out_bytes = out[g].size() * sizeof(uint32_t);
    DC_HIP(hipMalloc(&d_in, in_bytes));
    DC_HIP(hipMalloc(&d_out, out_bytes));
    DC_HIP(hipMemcpy(d_in, v.in[g].data(), in_bytes, hipMemcpyHostToDevice));
    DC_HIP(hipMemset(d_out, 0xff, out_bytes));
    const dim3 block(kLanes), grid((n + kLanes - 1) / kLanes), qgrid((4 * n + kLanes - 1) / kLanes);
    switch (g) {
      case G_FIELD: hipLaunchKernelGGL(k_group<G_FIELD>, grid, block, 0, 0, d_in, d_out, n); break;
      case G_FIELD32: hipLaunchKernelGGL(k_group<G_FIELD32>, grid, block, 0, 0, d_in, d_out, n); break;
      case G_CURVE: hipLaunchKernelGGL(k_group<G_CURVE>, grid, block, 0, 0, d_in, d_out, n); break;
      case G_QUAD: hipLaunchKernelGGL(k_quad, qgrid, block, 0, 0, d_in, d_out, n); break;
      case G_TOWER: hipLaunchKernelGGL(k_group<G_TOWER>, grid, block, 0, 0, d_in, d_out, n); break;
      default: hipLaunchKernelGGL(k_pair, grid, block, 0, 0, d_in, d_out, n, d_lines, v.nq); break;
    }
    DC_HIP(hipGetLastError());
    DC_HIP(hipDeviceSynchronize());
    DC_HIP(hipMemcpy(out[g].data(), d_out, out_bytes, hipMemcpyDeviceToHost));
    DC_HIP(hipFree(d_in));
    DC_HIP(hipFree(d_out));
    fprintf(stderr, "devcheck: group %u: %u records\n", g, n);
  }
  if (d_lines) DC_HIP(hipFree(d_lines));
  write_results(argv[2], v, out);
  return 0;
}
