// The kernel of the device form of capgpu_plonk_prove_notes_dev (notes_plan.hpp has the plan): k_move_rows_at is
// k_move_rows (compact_kernels.hpp) with a 64-bit SOURCE OFFSET per move instead of a slot number.  A group whose members'
// blocks do not lie at one constant stride in the caller's buffer is gathered into library staging by one launch: move k
// reads the block of the group's k-th member where the caller put it and writes row k of `to`.  `from` is the caller's
// buffer and is never written; `to` is Context::stage_b, so the two do not meet.  No workgroup waits for another: no
// atomics, no LDS, no field arithmetic - an HBM copy, 16 bytes per lane.
#pragma once
#include <hip/hip_runtime.h>

#include "notes_plan.hpp"

namespace cap {
namespace np {

// grid (row tiles, moves): a tile is kNotesTile x 16 bytes of a row; workgroup (x, y) copies tile x of the rows of moves
// y, y + gridDim.y, .. < count.  row16: 16-byte units between the rows of `to`; a lane at or past its move's len16 does
// nothing, so nothing is read outside the member's block and nothing written outside row k.
__global__ __launch_bounds__(kNotesTile) void k_move_rows_at(const uint4* __restrict__ from, uint4* __restrict__ to,
                                                             uint64_t row16, const MoveAt* __restrict__ moves, uint32_t count) {
  const uint64_t t = notes_lane(blockIdx.x, threadIdx.x);
  if (t >= row16) return;
#pragma unroll 4
  for (uint32_t k = blockIdx.y; k < count; k += gridDim.y) {
    const MoveAt mv = moves[k];
    if (t < mv.len16) to[notes_dst16(k, row16, t)] = from[notes_src16(mv.src, t)];
  }
}

}  // namespace np
}  // namespace cap
