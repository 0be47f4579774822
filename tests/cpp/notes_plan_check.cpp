// Host check of cap_amd/csrc/notes_plan.hpp (tests/test_notes_plan_host.py builds it plain and under ASan + UBSan): every
// assignment of 1 .. 8 notes to four (domain size, SRS) classes - two domain sizes that differ, two classes that differ
// only by SRS - and random assignments of 256 notes through notes_plan.  For each: the groups partition the notes; two
// notes share a group exactly when they share the class; groups are numbered by first appearance; members keep the
// caller's order; the run order is a permutation of the groups by count * n descending, ties by group number; max_inputs
// and max_row are the brute-force maxima.  constant_stride is compared with the definition written out in signed
// arithmetic over several layouts of the blocks.  The CAP_HD index functions of k_move_rows_at are run as the kernel runs
// them - every tile, every lane, every move - over a virtual source whose offsets lie past 2^33 elements, with rows whose
// length is no multiple of the tile.
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <vector>

#include "../../cap_amd/csrc/notes_plan.hpp"

using namespace cap::np;

static long g_bad = 0, g_assignments = 0, g_random = 0, g_direct = 0, g_gathered = 0, g_moves = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (g_bad++ < 20) printf("FAIL line %d: %s\n", __LINE__, #cond); \
    }                                                               \
  } while (0)

static const uint64_t kClassN[4] = {16, 64, 512, 64}, kClassSrs[4] = {7, 7, 7, 9};

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
  g_x ^= g_x << 13;
  g_x ^= g_x >> 7;
  g_x ^= g_x << 17;
  return g_x;
}

// the definition: block k of the group lies at offsets[m0] + k * s for ONE s, which is `exact` when that is given and
// otherwise at least min_stride (a lone block: any s will do)
static bool stride_by_definition(const std::vector<uint64_t>& off, const std::vector<uint32_t>& mem, uint64_t exact,
                                 uint64_t min_stride, int64_t* s_out) {
  if (mem.size() == 1) {
    *s_out = (int64_t)(exact ? exact : min_stride);
    return true;
  }
  const int64_t s = (int64_t)off[mem[1]] - (int64_t)off[mem[0]];
  if (exact ? s != (int64_t)exact : s < (int64_t)min_stride) return false;
  for (size_t k = 0; k < mem.size(); k++)
    if ((int64_t)off[mem[k]] != (int64_t)off[mem[0]] + (int64_t)k * s) return false;
  *s_out = s;
  return true;
}

static void check_strides(const Plan& pl, const std::vector<Note>& notes, bool vars) {
  const size_t N = notes.size();
  // layouts: 0 each group contiguous at its own stride, groups one behind the other; 1 the same with a gap of 3 per block
  // (a constant stride that is not the row length); 2 blocks in note order (groups interleaved); 3 reversed; 4 shuffled
  for (int layout = 0; layout < 5; layout++) {
    std::vector<uint64_t> off(N, 0);
    uint64_t at = 0;
    if (layout <= 1) {
      for (const Group& G : pl.groups)
        for (uint32_t i : G.members) {
          off[i] = at;
          at += G.max_row + (layout == 1 ? 3 : 0);
        }
    } else {
      std::vector<uint32_t> seq(N);
      for (size_t i = 0; i < N; i++) seq[i] = (uint32_t)(layout == 3 ? N - 1 - i : i);
      if (layout == 4)
        for (size_t i = N; i > 1; i--) std::swap(seq[i - 1], seq[next() % i]);
      for (uint32_t i : seq) {
        off[i] = at;
        at += notes[i].row + next() % 2;
      }
    }
    for (const Group& G : pl.groups) {
      const uint64_t exact = vars ? 0 : 5 * G.n;
      uint64_t got = 0;
      int64_t want = 0;
      const bool a = constant_stride(off.data(), G.members.data(), G.members.size(), exact, G.max_row, &got);
      const bool b = stride_by_definition(off, G.members, exact, G.max_row, &want);
      CHECK(a == b);
      if (a && b) CHECK((int64_t)got == want);
      if (a) CHECK(got >= G.max_row);
      (a ? g_direct : g_gathered)++;
      if (layout == 0) CHECK(a);
      if (layout == 1 && G.members.size() > 1) CHECK(a == vars);
    }
  }
}

static void check_assignment(const std::vector<uint8_t>& cls, bool vars) {
  const size_t N = cls.size();
  std::vector<Note> notes(N);
  for (size_t i = 0; i < N; i++) {
    const uint64_t n = kClassN[cls[i]];
    notes[i] = Note{n, kClassSrs[cls[i]], (i * 7 + cls[i]) % 5, vars ? n + 1 + (i * 5) % 11 : 5 * n};
  }
  const Plan pl = notes_plan(notes.data(), N);
  CHECK(pl.group_of.size() == N && pl.place_of.size() == N);
  if (pl.group_of.size() != N || pl.place_of.size() != N) return;
  // partition, member order, classes
  std::vector<uint8_t> seen(N, 0);
  size_t total = 0;
  uint64_t call_max = 0;
  for (size_t g = 0; g < pl.groups.size(); g++) {
    const Group& G = pl.groups[g];
    CHECK(!G.members.empty());
    if (G.members.empty()) return;
    uint64_t mi = 0, mr = 0;
    for (size_t k = 0; k < G.members.size(); k++) {
      const uint32_t i = G.members[k];
      CHECK(i < N);
      if (i >= N) return;
      CHECK(!seen[i]);
      seen[i] = 1;
      CHECK(k == 0 || G.members[k - 1] < i);
      CHECK(pl.group_of[i] == g && pl.place_of[i] == k);
      CHECK(notes[i].n == G.n && notes[i].srs == G.srs);
      mi = notes[i].num_inputs > mi ? notes[i].num_inputs : mi;
      mr = notes[i].row > mr ? notes[i].row : mr;
    }
    CHECK(G.max_inputs == mi && G.max_row == mr);
    call_max = mi > call_max ? mi : call_max;
    total += G.members.size();
    if (g) CHECK(pl.groups[g - 1].members[0] < G.members[0]);  // numbered by first appearance
    for (size_t h = 0; h < g; h++) CHECK(pl.groups[h].n != G.n || pl.groups[h].srs != G.srs);
  }
  CHECK(total == N);
  CHECK(pl.max_inputs == call_max);
  // run order
  CHECK(pl.order.size() == pl.groups.size());
  if (pl.order.size() != pl.groups.size()) return;
  std::vector<uint8_t> ran(pl.groups.size(), 0);
  for (size_t k = 0; k < pl.order.size(); k++) {
    const uint32_t g = pl.order[k];
    CHECK(g < pl.groups.size());
    if (g >= pl.groups.size()) return;
    CHECK(!ran[g]);
    ran[g] = 1;
    CHECK(pl.groups[g].run_order == k);
    if (k) {
      const uint32_t f = pl.order[k - 1];
      const uint64_t wf = pl.groups[f].members.size() * pl.groups[f].n, wg = pl.groups[g].members.size() * pl.groups[g].n;
      CHECK(wf > wg || (wf == wg && f < g));
    }
  }
  check_strides(pl, notes, vars);
}

// k_move_rows_at as its grid runs it, on a virtual source: unit u of the caller's buffer holds tag(u)
static uint64_t tag(uint64_t u) { return u * 0x9E3779B97F4A7C15ull + 12345; }
static void check_moves(uint64_t row16, const std::vector<MoveAt>& moves) {
  const uint64_t kUntouched = 0xFFFFFFFFFFFFFFFFull;
  std::vector<uint64_t> to(row16 * moves.size(), kUntouched);
  const uint32_t tiles = notes_tiles(row16), grid_y = moves.size() > 3 ? 3 : (uint32_t)moves.size();  // (y strides over the moves)
  CHECK((uint64_t)tiles * kNotesTile >= row16 && (uint64_t)(tiles - 1) * kNotesTile < row16);
  for (uint32_t bx = 0; bx < tiles; bx++)
    for (uint32_t by = 0; by < grid_y; by++)
      for (uint32_t lane = 0; lane < kNotesTile; lane++) {
        const uint64_t t = notes_lane(bx, lane);
        if (t >= row16) continue;
        for (uint32_t k = by; k < moves.size(); k += grid_y) {
          if (t >= moves[k].len16) continue;
          const uint64_t d = notes_dst16(k, row16, t), s = notes_src16(moves[k].src, t);
          CHECK(d < to.size());
          if (d >= to.size()) return;
          CHECK(s == moves[k].src * 2 + t && s >= moves[k].src * 2 && s < moves[k].src * 2 + moves[k].len16);
          CHECK(s / 2 >= moves[k].src);  // (no wrap: the byte offset 16 s is the block's 32 src plus 16 t)
          CHECK(to[d] == kUntouched);    // no unit written twice
          to[d] = tag(s);
          g_moves++;
        }
      }
  for (size_t k = 0; k < moves.size(); k++)
    for (uint64_t t = 0; t < row16; t++)
      CHECK(to[k * row16 + t] == (t < moves[k].len16 ? tag(moves[k].src * 2 + t) : kUntouched));
}

int main() {
  for (uint32_t N = 1; N <= 8; N++)
    for (uint32_t code = 0; code < (1u << (2 * N)); code++) {
      std::vector<uint8_t> cls(N);
      for (uint32_t i = 0; i < N; i++) cls[i] = (code >> (2 * i)) & 3;
      check_assignment(cls, (code ^ N) & 1);
      g_assignments++;
    }
  for (int rep = 0; rep < 64; rep++) {
    std::vector<uint8_t> cls(256);
    const uint32_t classes = 1 + rep % 4;
    for (auto& c : cls) c = (uint8_t)(next() % classes);
    check_assignment(cls, rep & 1);
    g_random++;
  }
  // ties: two groups of equal count * n (4 notes at n = 16, 1 at n = 64) run in group order, whichever comes first
  {
    const Note a{16, 7, 0, 80}, b{64, 7, 0, 320};
    const Note first_small[5] = {a, b, a, a, a}, first_large[5] = {b, a, a, a, a};
    const Plan p1 = notes_plan(first_small, 5), p2 = notes_plan(first_large, 5);
    CHECK(p1.order.size() == 2 && p1.order[0] == 0 && p1.order[1] == 1 && p1.groups[0].n == 16);
    CHECK(p2.order.size() == 2 && p2.order[0] == 0 && p2.order[1] == 1 && p2.groups[0].n == 64);
  }
  // the index functions: sources past 2^33 elements, rows shorter than a tile, of several tiles and a part, of exact tiles;
  // members of the variable form shorter than the row
  const uint64_t big = (uint64_t)1 << 33;
  check_moves(2 * 80, {{big + 5, 160}, {big * 3 + 1, 160}, {0, 160}});
  check_moves(2 * 333, {{big + 999, 666}, {7, 2 * 301}, {big * 2, 2}, {big - 1, 666}, {big + 4096, 2 * 17}});
  check_moves(512, {{big, 512}, {big + 256, 510}});
  check_moves(2 * 2560 + 2, {{big * 7 + 3, 2 * 2560 + 2}, {1, 2 * 2560}, {big, 0}, {big + 1, 258}});
  CHECK(notes_src16(big, 0) == (uint64_t)1 << 34);
  printf("assignments=%ld random=%ld direct=%ld gathered=%ld moves=%ld bad=%ld\n", g_assignments, g_random, g_direct, g_gathered,
         g_moves, g_bad);
  return g_bad ? 1 : 0;
}
