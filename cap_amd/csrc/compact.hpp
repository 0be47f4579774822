// Batch compaction of capgpu_plonk_prove_each* (capgpu_plonk_set_compaction): the plan.  Host only, no HIP - like
// outcome.hpp's host half; tests/cpp/compact_plan_check.cpp runs every mask of up to 12 proofs through it, under the
// sanitizers too.
//
// The witness check (capgpu_plonk_set_precheck) has refused `bad` of the P witnesses of an outcome call before the prover
// has reserved anything.  The survivors are proved as a batch of P' = P - bad: a survivor that sits in a slot below P'
// stays there, every refused slot below P' is filled with a survivor from a slot at or above P', both in ascending order.
// That is one row of witness data moved per refused slot below P' - at most min(bad, P') rows, never the whole batch - and
// no move reads a slot another move writes: k_move_rows (compact_kernels.hpp) does them all in one launch.
#pragma once
#include <stdint.h>

#include <vector>

namespace cap {
namespace cp {

// `_dev` evals / coeffs input is the caller's buffer and is never written: its survivors are COPIED into library staging
// (P' rows, about 10.5 MB of traffic each at n = 2^15) before the smaller batch runs.  The copy is taken when
// bad * kCompactCopyRatio >= P' - when the proofs saved are worth the rows copied; below that the call runs uncompacted.
// Measured at n = 2^15 with the route forced (profiles/prove_compact_ab.txt): copying 255 rows takes
// 0.41 ms, a proof 0.64 ms; with 1 or 2 of 256 refused the compacted call is faster by no more than the arms' spread, with
// 4 of 256 by 1.4 %, four times the spread - 64 takes the route from 4 of 256 on and not below.
// (-DCAP_COMPACT_COPY_RATIO=...: A/B builds that force the route, tools/gpu_prove_compact_ab.py --refused.)
#ifndef CAP_COMPACT_COPY_RATIO
#define CAP_COMPACT_COPY_RATIO 64
#endif
constexpr uint32_t kCompactCopyRatio = CAP_COMPACT_COPY_RATIO;

struct Move {
  uint32_t src, dst;  // rows: src >= P' > dst
};
struct Plan {
  uint32_t survivors = 0;      // P'
  std::vector<uint32_t> orig;  // [P']: the caller's index of the proof in slot i
  std::vector<Move> moves;     // one per refused slot below P'; sources pairwise distinct, destinations too
};

// refused[p] != 0: proof p was refused (fault.kind != 0).  (bad == 0 gives the identity and no moves, bad == P an empty
// plan: neither is worth a call.)
inline Plan compact_plan(const uint8_t* refused, uint32_t P) {
  Plan pl;
  for (uint32_t p = 0; p < P; p++) pl.survivors += refused[p] == 0;
  const uint32_t S = pl.survivors;
  pl.orig.resize(S);
  uint32_t src = S;  // the next candidate source: survivors at or above P', ascending
  for (uint32_t dst = 0; dst < S; dst++) {
    if (!refused[dst]) {
      pl.orig[dst] = dst;
      continue;
    }
    // refused slots below P' and survivors at or above it are equally many: src stays below P
    while (refused[src]) src++;
    pl.moves.push_back(Move{src, dst});
    pl.orig[dst] = src++;
  }
  return pl;
}

// whether the copy route of `_dev` columns is worth taking (see kCompactCopyRatio)
inline bool copy_route_pays(uint32_t bad, uint32_t survivors) {
  return (uint64_t)bad * kCompactCopyRatio >= survivors;
}

}  // namespace cp
}  // namespace cap
