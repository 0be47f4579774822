// Device conformance check: the vector and result files (host code shared by the two drivers).
//   vectors:  kMagic, G_COUNT, nq, nq x 32 words (G2 points: x.c0, x.c1, y.c0, y.c1 as 2^256-Montgomery words),
//             then for every group in order: group id, record count, records of kInWords[group]
//   results:  kMagic, G_COUNT, then for every group: group id, record count, records of kOutWords[group]
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "devcheck_ops.hpp"

namespace devcheck {

struct Vectors {
  std::vector<uint32_t> g2;  // 32 words per point
  std::vector<uint32_t> in[G_COUNT];
  uint32_t count[G_COUNT];
  uint32_t nq = 0;
};

[[noreturn]] inline void die(const char* what) {
  fprintf(stderr, "devcheck: %s\n", what);
  exit(2);
}
inline void read_words(FILE* f, uint32_t* w, size_t n) {
  if (n && fread(w, sizeof(uint32_t), n, f) != n) die("vector file is truncated");
}
inline Vectors read_vectors(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) die("cannot open the vector file");
  uint32_t head[3];
  read_words(f, head, 3);
  if (head[0] != kMagic || head[1] != G_COUNT || head[2] > 4096) die("not a devcheck vector file");
  Vectors v;
  v.nq = head[2];
  v.g2.resize((size_t)v.nq * 32);
  read_words(f, v.g2.data(), v.g2.size());
  for (uint32_t g = 0; g < G_COUNT; g++) {
    uint32_t gh[2];
    read_words(f, gh, 2);
    if (gh[0] != g || gh[1] > (1u << 22)) die("bad group header");
    v.count[g] = gh[1];
    v.in[g].resize((size_t)gh[1] * kInWords[g]);
    read_words(f, v.in[g].data(), v.in[g].size());
  }
  fclose(f);
  return v;
}
inline void write_results(const char* path, const Vectors& v, const std::vector<uint32_t> out[G_COUNT]) {
  FILE* f = fopen(path, "wb");
  if (!f) die("cannot open the result file");
  const uint32_t head[2] = {kMagic, G_COUNT};
  bool ok = fwrite(head, sizeof(uint32_t), 2, f) == 2;
  for (uint32_t g = 0; g < G_COUNT && ok; g++) {
    const uint32_t gh[2] = {g, v.count[g]};
    ok = fwrite(gh, sizeof(uint32_t), 2, f) == 2 &&
         (out[g].empty() || fwrite(out[g].data(), sizeof(uint32_t), out[g].size(), f) == out[g].size());
  }
  if (fclose(f) != 0 || !ok) die("cannot write the result file");
}
// the prepared line tables of the file's G2 points (pairing29.hpp: prepare_lines), kLines per point
inline std::vector<p29::line_coeffs> prepare_all_lines(const Vectors& v) {
  std::vector<p29::line_coeffs> l((size_t)v.nq * p29::kLines);
  for (uint32_t i = 0; i < v.nq; i++) {
    const uint32_t* w = &v.g2[(size_t)i * 32];
    pairing::g2_affine q;
    q.x.c0 = rd_fe(w);
    q.x.c1 = rd_fe(w + 8);
    q.y.c0 = rd_fe(w + 16);
    q.y.c1 = rd_fe(w + 24);
    p29::prepare_lines(q, &l[(size_t)i * p29::kLines]);
  }
  return l;
}

}  // namespace devcheck
