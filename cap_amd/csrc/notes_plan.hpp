// capgpu_plonk_prove_notes*: the plan of a call whose keys have several domain sizes (or SRS).  Host only, no HIP - like
// compact.hpp and solve_plan.hpp; tests/cpp/notes_plan_check.cpp runs every assignment of up to 8 notes to 4 classes
// through it, under the sanitizers too.
//
// One device batch holds keys of ONE domain size under ONE SRS (key_set, plonk.hip).  A GROUP is all notes of a call whose
// keys share (domain size, SRS): what one such batch may hold.  Groups are numbered by first appearance, a group's members
// keep the caller's order, and the groups RUN by count * n descending - the heaviest first, so that the light ones fill in
// behind it on the other contexts -, ties by group number.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#ifndef CAP_HD
#if defined(__HIPCC__)
#define CAP_HD __host__ __device__ __forceinline__
#else
#define CAP_HD inline
#endif
#endif

namespace cap {
namespace np {

struct Note {
  uint64_t n = 0;           // domain size of the note's key
  uint64_t srs = 0;         // ... and its SRS handle
  uint64_t num_inputs = 0;  // public inputs of the key
  uint64_t row = 0;         // field elements of the note's witness block: 5 n, or - variable form - the key's num_vars
};
struct Group {
  uint64_t n = 0, srs = 0;
  std::vector<uint32_t> members;  // note indices, ascending
  uint64_t max_inputs = 0;        // the largest num_inputs among the members' keys
  uint64_t max_row = 0;           // the largest row among them (variable form: the stride of the group's batch)
  uint32_t run_order = 0;         // position in Plan::order
};
struct Plan {
  std::vector<uint32_t> group_of;  // [notes]
  std::vector<uint32_t> place_of;  // [notes]: index in its group's members
  std::vector<Group> groups;       // by first appearance
  std::vector<uint32_t> order;     // group numbers in run order
  uint64_t max_inputs = 0;         // over the whole call: the row length of its public inputs
};

inline Plan notes_plan(const Note* notes, size_t count) {
  Plan pl;
  pl.group_of.resize(count);
  pl.place_of.resize(count);
  for (size_t i = 0; i < count; i++) {
    size_t g = 0;
    while (g < pl.groups.size() && (pl.groups[g].n != notes[i].n || pl.groups[g].srs != notes[i].srs)) g++;
    if (g == pl.groups.size()) {
      pl.groups.emplace_back();
      pl.groups[g].n = notes[i].n;
      pl.groups[g].srs = notes[i].srs;
    }
    Group& G = pl.groups[g];
    pl.group_of[i] = (uint32_t)g;
    pl.place_of[i] = (uint32_t)G.members.size();
    G.members.push_back((uint32_t)i);
    G.max_inputs = std::max(G.max_inputs, notes[i].num_inputs);
    G.max_row = std::max(G.max_row, notes[i].row);
    pl.max_inputs = std::max(pl.max_inputs, notes[i].num_inputs);
  }
  pl.order.resize(pl.groups.size());
  for (size_t g = 0; g < pl.order.size(); g++) pl.order[g] = (uint32_t)g;
  std::stable_sort(pl.order.begin(), pl.order.end(), [&](uint32_t a, uint32_t b) {
    return pl.groups[a].members.size() * pl.groups[a].n > pl.groups[b].members.size() * pl.groups[b].n;
  });
  for (size_t k = 0; k < pl.order.size(); k++) pl.groups[pl.order[k]].run_order = (uint32_t)k;
  return pl;
}

// Device form: whether the blocks of a group's members already lie where one device batch reads them - at ONE constant
// stride in member order, block k at offsets[members[0]] + k * stride.  `exact` != 0 (evals / coeffs): that stride must be
// exactly `exact` = 5 n; exact == 0 (variable form): any constant stride of at least min_stride, the group's largest
// num_vars - a lone member takes min_stride.  Offsets and the stride are in field elements.
inline bool constant_stride(const uint64_t* offsets, const uint32_t* members, size_t count, uint64_t exact, uint64_t min_stride,
                            uint64_t* stride_out) {
  uint64_t stride = exact ? exact : min_stride;
  if (count > 1) {
    const uint64_t a = offsets[members[0]], b = offsets[members[1]];
    if (b <= a) return false;
    stride = b - a;
    if (exact ? stride != exact : stride < min_stride) return false;
    for (size_t k = 2; k < count; k++)
      if (offsets[members[k]] < offsets[members[k - 1]] || offsets[members[k]] - offsets[members[k - 1]] != stride) return false;
  }
  *stride_out = stride;
  return true;
}

// ---- k_move_rows_at (notes_kernels.hpp): where lane t of tile x of move k reads and writes, in 16-byte units -----------
// Move k reads `len16` units at from + 2 * src (src: an offset in field elements of 32 bytes, 2 units each) and writes
// them to row k of `to`, whose rows are row16 units apart - the group's row length; a member of the variable form with
// fewer variables than the group's largest moves its own len16 <= row16 and no more, so nothing outside its block is read.
// kNotesTile lanes per tile; a lane whose t is at or past the move's len16 moves nothing.
struct MoveAt {
  uint64_t src;    // field elements from the caller's base
  uint64_t len16;  // 16-byte units to move
};
constexpr uint32_t kNotesTile = 256;
CAP_HD uint64_t notes_lane(uint32_t tile, uint32_t lane) { return (uint64_t)tile * kNotesTile + lane; }
CAP_HD uint64_t notes_src16(uint64_t src, uint64_t t) { return src * 2 + t; }
CAP_HD uint64_t notes_dst16(uint64_t k, uint64_t row16, uint64_t t) { return k * row16 + t; }
inline uint32_t notes_tiles(uint64_t row16) { return (uint32_t)((row16 + kNotesTile - 1) / kNotesTile); }

}  // namespace np
}  // namespace cap
