// capgpu::proof::check_satisfiability (include/capgpu_proof.hpp) on the golden instance tests/cpp/proof_api_test.cpp also
// loads: the assignment as it is, then with bit 0 of one cell's first Montgomery word flipped.
//   check_satisfiability_test instance.bin wire row [wire row ...]
// prints "OK" or "ERR <message>" for the unmodified assignment and for each mutation (one cell at a time);
// tests/test_gpu_check_witness.py compares the messages with oracle/plonk.py.  Exit 2: no usable GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "capgpu_proof.hpp"

using namespace capgpu;

static std::vector<uint64_t> words(std::ifstream& f, size_t count) {
  std::vector<uint64_t> v(count);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(8 * count));
  if (!f) {
    std::fprintf(stderr, "short input file\n");
    std::exit(1);
  }
  return v;
}

static void report(const Result<Unit>& r) {
  if (r.is_ok()) std::printf("OK\n");
  else std::printf("ERR %s\n", r.error().msg.c_str());
}

int main(int argc, char** argv) {
  if (argc < 2 || argc % 2 != 0) {
    std::fprintf(stderr, "usage: %s instance.bin [wire row]...\n", argv[0]);
    return 1;
  }
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) {
    std::perror(argv[1]);
    return 1;
  }
  auto hdr = words(f, 4);
  if (std::memcmp(hdr.data(), "CAPH\0\0\0\0", 8) != 0) return 1;
  const size_t n = (size_t)1 << hdr[1], num_inputs = (size_t)hdr[2];
  Fr tau{};
  auto t = words(f, 4);
  std::memcpy(tau.data(), t.data(), 32);
  const auto selectors = words(f, 13 * n * 4), sigma = words(f, 5 * n * 4);
  auto wires = words(f, 5 * n * 4);
  const auto pubs = words(f, num_inputs * 4);

  auto setup = proof::universal_setup(n + 2, tau);
  if (setup.is_err()) {
    std::fprintf(stderr, "universal_setup: %s\n", setup.error().to_string().c_str());
    return 2;
  }
  const FinalisedCircuit circuit{n, num_inputs, selectors.data(), sigma.data(), n};
  auto pre = proof::transfer::preprocess(setup.unwrap(), 2, 2, 26, circuit);
  if (pre.is_err()) {
    std::fprintf(stderr, "preprocess: %s\n", pre.error().to_string().c_str());
    return 1;
  }
  const ProvingKey& pk = pre.unwrap().proving_key.proving_key;
  report(proof::check_satisfiability(pk, Assignment{wires.data(), pubs.data()}));
  for (int a = 2; a + 1 < argc; a += 2) {
    const size_t cell = ((size_t)std::atoi(argv[a]) * n + (size_t)std::atoi(argv[a + 1])) * 4;
    wires[cell] ^= 1;
    report(proof::check_satisfiability(pk, Assignment{wires.data(), pubs.data()}));
    wires[cell] ^= 1;
  }
  report(proof::check_satisfiability(pk, Assignment{}));  // an empty assignment is refused, not read
  return 0;
}
