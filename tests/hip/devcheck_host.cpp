// Device conformance check, host driver: the operation table of devcheck_ops.hpp compiled for the CPU with field29.hpp's
// bound assertions on.  usage: devcheck_host <vectors> <results>.  The quad group runs on four simulated lanes (QuadSim).
#define CAP_FL_CHECK 1
#include "devcheck_io.hpp"

using namespace devcheck;

template <int S>
struct SlowHost {
  g1x operator()(const g1x& a, const g1x& b) const { return G1LT<S>::add(a, b); }
};

int main(int argc, char** argv) {
  if (argc != 3) die("usage: devcheck_host <vectors> <results>");
  const Vectors v = read_vectors(argv[1]);
  const std::vector<p29::line_coeffs> lines = prepare_all_lines(v);
  std::vector<uint32_t> out[G_COUNT];
  for (uint32_t g = 0; g < G_COUNT; g++) {
    out[g].assign((size_t)v.count[g] * kOutWords[g], 0xffffffffu);
    for (uint32_t i = 0; i < v.count[g]; i++) {
      const uint32_t* in = &v.in[g][(size_t)i * kInWords[g]];
      uint32_t* o = &out[g][(size_t)i * kOutWords[g]];
      switch (g) {
        case G_FIELD: run_field(in, o); break;
        case G_FIELD32: run_field32(in, o); break;
        case G_CURVE: run_curve(in, o); break;
        case G_QUAD:
          if (in[2] == 0) quad_ops<0, QuadSim>(in, o, SlowHost<0>(), true);
          else if (in[2] == 1) quad_ops<1, QuadSim>(in, o, SlowHost<1>(), true);
          break;
        case G_TOWER: run_tower(in, o); break;
        default: run_pair(in, o, lines.data(), v.nq); break;
      }
    }
  }
  write_results(argv[2], v, out);
  return 0;
}
