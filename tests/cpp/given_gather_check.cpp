// cap_amd/csrc/given_gather.hpp on the host: the packing rule of a gathered part of capgpu_plonk_prove_given_one /
// _io_one requests.  Every assignment of 1 .. 8 requests to three keys of different (num_given, num_inputs), with every
// choice of 0 .. 2 of them set aside for each of the three reasons in turn:
//   * the slots are given in arrival order, the packed offsets are disjoint and ascending, the strides are the largest
//     lengths among the keys of the requests that RUN;
//   * a short row is zero-filled to the part's maximum and no row touches its neighbour (the arrays are pre-filled with a
//     pattern and have exactly the planned length: the sanitizers see a write past them);
//   * the scatter returns each request the words of its own slot;
//   * a faulted outcome has degree_flags 0, a clean or merely flagged one keeps its record.
// Built by tests/test_given_gather_host.py, plain and with -fsanitize=address,undefined.  Prints one summary line.
#include <stdio.h>

#include <vector>

#include "../../cap_amd/csrc/given_gather.hpp"

using namespace cap;

struct KeyShape {
  size_t num_given, num_inputs;
};
static const KeyShape kKeys[3] = {{3, 1}, {7, 4}, {5, 0}};
static const uint64_t kPattern = 0xa5a5a5a5a5a5a5a5ull;

static unsigned long long bad = 0, plans = 0, aside_seen[4] = {0, 0, 0, 0}, filled = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      if (bad++ < 20) printf("FAIL line %d: %s\n", __LINE__, #c);    \
    }                                                                \
  } while (0)

// the word request i brings at element e, word w of its given row / public inputs / blinders (never 0, never the pattern)
static uint64_t word(int what, size_t i, size_t e, size_t w) { return ((uint64_t)(what + 1) << 56) | (i << 40) | (e << 8) | (w + 1); }

static gg::Ask ask_of(const KeyShape& k, int why) {
  gg::Ask a;
  a.key_found = why != gg::kKeyGone;
  a.has_solver = why != gg::kNoSolver;
  a.key_given = k.num_given;
  a.key_inputs = k.num_inputs;
  a.num_given = k.num_given + (why == gg::kLengths ? 1 : 0);
  a.num_inputs = k.num_inputs;
  return a;
}

static void one_case(const std::vector<int>& key_of, const std::vector<int>& why) {
  const size_t R = key_of.size();
  std::vector<gg::Ask> asks(R);
  for (size_t i = 0; i < R; i++) asks[i] = ask_of(kKeys[key_of[i]], why[i]);
  const gg::Plan pl = gg::plan(asks.data(), R);
  plans++;
  CHECK(pl.why.size() == R && pl.slot_of.size() == R);
  // who runs, in arrival order, and the strides
  size_t want_slots = 0, gs = 0, ps = 0;
  for (size_t i = 0; i < R; i++) {
    CHECK(pl.why[i] == why[i]);
    aside_seen[pl.why[i]]++;
    if (why[i] != gg::kRuns) {
      CHECK(pl.slot_of[i] == gg::kNone);
      continue;
    }
    CHECK(pl.slot_of[i] == want_slots);
    CHECK(want_slots < pl.req_of.size() && pl.req_of[want_slots] == i);
    want_slots++;
    gs = std::max(gs, kKeys[key_of[i]].num_given);
    ps = std::max(ps, kKeys[key_of[i]].num_inputs);
  }
  CHECK(pl.slots() == want_slots && pl.given_stride == gs && pl.pub_stride == ps);
  for (size_t s = 0; s + 1 < pl.slots(); s++) {
    CHECK(pl.req_of[s] < pl.req_of[s + 1]);
    CHECK(pl.given_at(s) + gg::kWords * gs == pl.given_at(s + 1));
    CHECK(pl.pub_at(s) + gg::kWords * ps == pl.pub_at(s + 1));
    CHECK(pl.blind_at(s) + gg::kWords * gg::kBlinders == pl.blind_at(s + 1));
  }
  // pack
  std::vector<uint64_t> given(pl.given_words(), kPattern), pubs(pl.pub_words(), kPattern), blind(pl.blind_words(), kPattern);
  for (size_t s = 0; s < pl.slots(); s++) {
    const size_t i = pl.req_of[s];
    const KeyShape& k = kKeys[key_of[i]];
    std::vector<uint64_t> g(gg::kWords * k.num_given), p(gg::kWords * k.num_inputs);
    for (size_t e = 0; e < k.num_given; e++)
      for (size_t w = 0; w < gg::kWords; w++) g[gg::kWords * e + w] = word(0, i, e, w);
    for (size_t e = 0; e < k.num_inputs; e++)
      for (size_t w = 0; w < gg::kWords; w++) p[gg::kWords * e + w] = word(1, i, e, w);
    CHECK(pl.given_at(s) + gg::kWords * gs <= given.size() && pl.pub_at(s) + gg::kWords * ps <= pubs.size());
    gg::pack_row(&given[pl.given_at(s)], pl.given_stride, g.data(), k.num_given);
    gg::pack_row(&pubs[pl.pub_at(s)], pl.pub_stride, k.num_inputs ? p.data() : nullptr, k.num_inputs);
    for (size_t e = 0; e < gg::kBlinders; e++)
      for (size_t w = 0; w < gg::kWords; w++) blind[pl.blind_at(s) + gg::kWords * e + w] = word(2, i, e, w);
  }
  // every word of the packed arrays: the owner's, or the zero fill; the tail keeps the pattern
  for (size_t s = 0; s < pl.slots(); s++) {
    const size_t i = pl.req_of[s];
    const KeyShape& k = kKeys[key_of[i]];
    for (size_t e = 0; e < gs; e++)
      for (size_t w = 0; w < gg::kWords; w++) {
        const uint64_t got = given[pl.given_at(s) + gg::kWords * e + w];
        CHECK(got == (e < k.num_given ? word(0, i, e, w) : 0));
        filled += e >= k.num_given;
      }
    for (size_t e = 0; e < ps; e++)
      for (size_t w = 0; w < gg::kWords; w++)
        CHECK(pubs[pl.pub_at(s) + gg::kWords * e + w] == (e < k.num_inputs ? word(1, i, e, w) : 0));
  }
  for (size_t w = pl.given_at(pl.slots()); w < given.size(); w++) CHECK(given[w] == kPattern);
  for (size_t w = pl.pub_at(pl.slots()); w < pubs.size(); w++) CHECK(pubs[w] == kPattern);
  for (size_t w = pl.blind_at(pl.slots()); w < blind.size(); w++) CHECK(blind[w] == kPattern);
  // scatter: each request its own slot
  for (size_t i = 0; i < R; i++) {
    if (pl.slot_of[i] == gg::kNone) continue;
    const KeyShape& k = kKeys[key_of[i]];
    std::vector<uint64_t> back(gg::kWords * k.num_inputs + 1, kPattern);
    gg::take_row(back.data(), &pubs[pl.pub_at(pl.slot_of[i])], k.num_inputs);
    for (size_t e = 0; e < k.num_inputs; e++)
      for (size_t w = 0; w < gg::kWords; w++) CHECK(back[gg::kWords * e + w] == word(1, i, e, w));
    CHECK(back.back() == kPattern);
    CHECK(blind[pl.blind_at(pl.slot_of[i])] == word(2, i, 0, 0));
  }
}

static void outcomes() {
  for (uint32_t kind = 0; kind < 3; kind++)
    for (uint32_t flags : {0u, 1u, 6u}) {
      capgpu_prove_outcome o;
      memset(&o, 0, sizeof o);
      o.fault.kind = kind;
      o.fault.row = 77;
      o.degree_flags = flags;
      o.status = (kind || flags) ? CAPGPU_ERR_PROOF : CAPGPU_OK;
      const capgpu_prove_outcome before = o;
      gg::normalise(&o);
      CHECK(o.degree_flags == (kind ? 0u : flags));
      CHECK(o.status == before.status && o.fault.kind == kind && o.fault.row == 77);
      if (!kind) CHECK(memcmp(&o, &before, sizeof o) == 0);
    }
  // the order of the reasons: a missing key before a missing solver before the lengths
  gg::Ask a = ask_of(kKeys[0], gg::kLengths);
  a.has_solver = false;
  CHECK(gg::set_aside(a) == gg::kNoSolver);
  a.key_found = false;
  CHECK(gg::set_aside(a) == gg::kKeyGone);
  a = ask_of(kKeys[1], gg::kRuns);
  a.num_inputs++;
  CHECK(gg::set_aside(a) == gg::kLengths);
}

int main() {
  unsigned long long assignments = 0;
  for (size_t R = 1; R <= 8; R++) {
    size_t total = 1;
    for (size_t i = 0; i < R; i++) total *= 3;
    for (size_t code = 0; code < total; code++) {
      std::vector<int> key_of(R);
      size_t c = code;
      for (size_t i = 0; i < R; i++, c /= 3) key_of[i] = (int)(c % 3);
      assignments++;
      std::vector<int> why(R, gg::kRuns);
      one_case(key_of, why);  // nobody set aside
      for (size_t a = 0; a < R; a++) {
        why.assign(R, gg::kRuns);
        why[a] = 1 + (int)((a + code) % 3);
        one_case(key_of, why);  // one
        for (size_t b = a + 1; b < R; b++) {
          why[b] = 1 + (int)((b + code / 3) % 3);
          one_case(key_of, why);  // two
          why[b] = gg::kRuns;
        }
      }
    }
  }
  outcomes();
  printf("assignments=%llu plans=%llu runs=%llu key_gone=%llu no_solver=%llu lengths=%llu zero_filled=%llu bad=%llu\n", assignments,
         plans, aside_seen[0], aside_seen[1], aside_seen[2], aside_seen[3], filled, bad);
  return bad ? 1 : 0;
}
