// Host check of cap_amd/csrc/compact.hpp (tests/test_compact_plan_host.py builds it plain and under ASan + UBSan): every
// refusal mask of P = 1 .. 12 proofs and random masks at P = 256 through compact_plan.  For each: P' is the number of
// survivors; orig is an injection onto exactly the surviving indices and the identity on every slot that no move writes;
// every move takes a surviving row at or above P' to a refused slot below it; sources are pairwise distinct and so are
// destinations; there is one move per refused slot below P'; and applying the moves to an array of row tags - all reads
// before all writes, as one launch of k_move_rows may order them - leaves orig in the first P' slots.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../cap_amd/csrc/compact.hpp"

using namespace cap::cp;

static long g_bad = 0, g_masks = 0, g_zero_moves = 0, g_max_moves = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      if (g_bad++ < 20) printf("FAIL line %d: %s (P=%u)\n", __LINE__, #cond, P); \
    }                                                                        \
  } while (0)

static void check_mask(const std::vector<uint8_t>& refused) {
  const uint32_t P = (uint32_t)refused.size();
  g_masks++;
  const Plan pl = compact_plan(refused.data(), P);
  uint32_t survivors = 0, refused_below = 0;
  for (uint32_t p = 0; p < P; p++) survivors += !refused[p];
  const uint32_t S = survivors, bad = P - S;
  for (uint32_t p = 0; p < S; p++) refused_below += refused[p] != 0;
  CHECK(pl.survivors == S);
  CHECK(pl.orig.size() == S);
  CHECK(pl.moves.size() == refused_below);
  CHECK(pl.moves.size() <= (bad < S ? bad : S));
  if (pl.orig.size() != S) return;
  // orig: into the survivors, no index twice - with S entries that is onto
  std::vector<uint8_t> seen(P, 0), is_dst(P, 0), is_src(P, 0);
  for (uint32_t i = 0; i < S; i++) {
    CHECK(pl.orig[i] < P);
    if (pl.orig[i] >= P) return;
    CHECK(!refused[pl.orig[i]]);
    CHECK(!seen[pl.orig[i]]);
    seen[pl.orig[i]] = 1;
  }
  for (const Move& mv : pl.moves) {
    CHECK(mv.src < P && mv.src >= S && mv.dst < S);
    if (!(mv.src < P && mv.dst < S)) return;
    CHECK(refused[mv.dst]);
    CHECK(!refused[mv.src]);
    CHECK(!is_src[mv.src]);
    CHECK(!is_dst[mv.dst]);
    is_src[mv.src] = 1;
    is_dst[mv.dst] = 1;
  }
  for (uint32_t i = 0; i < S; i++)
    if (!is_dst[i]) CHECK(pl.orig[i] == i);
  // the moves on row tags: every source is read before any destination is written
  std::vector<uint32_t> rows(P), loaded(pl.moves.size());
  for (uint32_t p = 0; p < P; p++) rows[p] = p;
  for (size_t k = 0; k < pl.moves.size(); k++) loaded[k] = rows[pl.moves[k].src];
  for (size_t k = pl.moves.size(); k-- > 0;) rows[pl.moves[k].dst] = loaded[k];  // (in any order: here the reverse)
  for (uint32_t i = 0; i < S; i++) CHECK(rows[i] == pl.orig[i]);
  if (bad && pl.moves.empty()) g_zero_moves++;
  if (bad && pl.moves.size() == (bad < S ? bad : S)) g_max_moves++;
  if (bad) CHECK(copy_route_pays(bad, S) == ((uint64_t)bad * kCompactCopyRatio >= S));
}

int main() {
  for (uint32_t P = 1; P <= 12; P++)
    for (uint32_t mask = 0; mask < (1u << P); mask++) {
      std::vector<uint8_t> refused(P);
      for (uint32_t p = 0; p < P; p++) refused[p] = (mask >> p) & 1;
      check_mask(refused);
    }
  // P = 256: random masks of several densities, and the shapes with no move and with the most
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  const uint32_t P = 256;
  for (uint32_t density : {1u, 8u, 32u, 128u, 224u, 255u})
    for (int rep = 0; rep < 8; rep++) {
      std::vector<uint8_t> refused(P);
      for (uint32_t p = 0; p < P; p++) refused[p] = next() % 256 < density;
      check_mask(refused);
    }
  for (uint32_t bad : {1u, 32u, 128u, 255u}) {
    std::vector<uint8_t> tail(P, 0), front(P, 0);
    for (uint32_t p = 0; p < bad; p++) {
      tail[P - 1 - p] = 1;  // all refused slots in the tail: nothing moves
      front[p] = 1;         // all at the front: min(bad, P') moves
    }
    const long z0 = g_zero_moves, m0 = g_max_moves;
    check_mask(tail);
    CHECK(g_zero_moves == z0 + 1);
    check_mask(front);
    CHECK(g_max_moves == m0 + 1);
    CHECK(compact_plan(front.data(), P).moves.size() == (bad < P - bad ? bad : P - bad));
  }
  printf("masks=%ld zero_moves=%ld max_moves=%ld bad=%ld\n", g_masks, g_zero_moves, g_max_moves, g_bad);
  return g_bad ? 1 : 0;
}
