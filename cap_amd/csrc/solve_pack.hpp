// Packing several witnesses into one workgroup of the witness solver (k_solve_vars_packed<W>, solve_kernels.hpp): how a
// lane finds its work, and how many witnesses W a workgroup takes.  The decode is host + device; the choice of W is host
// code without HIP, like solve_plan.hpp.  tests/cpp/solve_pack_check.cpp emulates a packed workgroup with this same code.
//
// A workgroup b of a launch at W completes the witnesses of its W SLOTS: slot s holds entry b W + s of the launch's
// witness list, or nothing when that is at or beyond `count`.  Inside level l, of r rows, the lanes stride over r W ITEMS:
//   item i  =  row level_off[l] + i / W  for slot i % W          (i < r W)
// so W adjacent lanes read one row record, one set of selectors and ids and one row constant, and branch on one kind.
// An empty slot's items do nothing, but their lanes reach the level's barrier like the others.
//
// THE CHOICE OF W.  A launch of one witness always runs the unpacked kernel.  Setting 1, 2, 4, 8, 16: that W, whatever
// the count (a last workgroup with empty slots included).  Setting 0 (the default): the largest power of two <= 16 with
//   W * median_level_width <= threads per workgroup       (fixed when the key takes its schedule)
//   W <= the largest power of two not above count         (per launch)
// The median is the lower median of the levels' row counts: half the barriers of a walk then see every lane of the
// packed workgroup busy at most once.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CAP_SPK_HD __host__ __device__ __forceinline__
#else
#define CAP_SPK_HD inline
#endif

namespace cap {
namespace spk {

constexpr int kMaxPack = 16;

struct Item {
  uint32_t k;     // index into the plan's rows
  uint32_t slot;  // witness slot of the workgroup, below W
};
// items of a level of `rows` rows (rows <= n <= 2^26: no overflow)
CAP_SPK_HD uint32_t level_items(uint32_t rows, uint32_t W) { return rows * W; }
CAP_SPK_HD Item item_decode(uint32_t level_begin, uint32_t i, uint32_t W) { return Item{level_begin + i / W, i % W}; }
// entry of the launch's witness list that slot `slot` of workgroup `block` holds; at or beyond count: the slot is empty
CAP_SPK_HD uint32_t slot_entry(uint32_t block, uint32_t slot, uint32_t W) { return block * W + slot; }
// the witness behind an entry: the list's, or - no list - the entry itself
CAP_SPK_HD uint32_t entry_witness(const uint32_t* which, uint32_t entry) { return which ? which[entry] : entry; }
CAP_SPK_HD uint32_t blocks_for(uint32_t count, uint32_t W) { return (count + W - 1) / W; }

inline bool valid_setting(int w) { return w == 0 || w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }

// lower median of the levels' row counts; 0 for a plan without levels
inline uint32_t median_level_width(const uint32_t* level_off, size_t levels) {
  if (!levels) return 0;
  // (levels are few - hundreds: a selection by counting smaller-or-equal widths would not pay)
  uint32_t* w = new uint32_t[levels];
  for (size_t l = 0; l < levels; l++) w[l] = level_off[l + 1] - level_off[l];
  for (size_t i = 1; i < levels; i++) {  // insertion sort
    const uint32_t x = w[i];
    size_t j = i;
    for (; j > 0 && w[j - 1] > x; j--) w[j] = w[j - 1];
    w[j] = x;
  }
  const uint32_t m = w[(levels - 1) / 2];
  delete[] w;
  return m;
}

// the plan's term of the automatic rule
inline int auto_pack(uint32_t median_width, int threads) {
  int W = kMaxPack;
  while (W > 1 && (uint64_t)W * median_width > (uint64_t)threads) W /= 2;
  return W;
}
// the largest power of two <= kMaxPack that is not above count (count >= 1)
inline int count_cap(uint32_t count) {
  int W = 1;
  while (W * 2 <= kMaxPack && (uint32_t)(W * 2) <= count) W *= 2;
  return W;
}
// W of one launch: `setting` as capgpu_plonk_set_solve_pack took it, `plan_auto` = auto_pack of the key's schedule
inline int pack_for(int setting, int plan_auto, uint32_t count) {
  if (count <= 1) return 1;
  if (setting > 0) return setting;
  const int cap = count_cap(count);
  return plan_auto < cap ? plan_auto : cap;
}

}  // namespace spk
}  // namespace cap
