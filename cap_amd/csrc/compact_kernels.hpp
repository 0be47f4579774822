// The kernel of batch compaction (compact.hpp has the plan): k_move_rows copies whole witness rows - the five wire columns
// of one proof, 5 n field elements - from slot moves[k].src of `from` to slot moves[k].dst of `to`, all moves of a call in
// one launch.  In place (from == to: library staging, gathered columns) the plan's sources lie at or above P' and its
// destinations below, so no move reads what another writes; out of place (`from` the caller's device buffer, which is
// never written, `to` library staging) the two do not meet at all.  Either way no workgroup waits for another: no atomics,
// no LDS, no field arithmetic - an HBM copy, 16 bytes per lane and access as k_gather_vars moves its cells.
#pragma once
#include <hip/hip_runtime.h>

#include "plonk_kernels.hpp"

namespace cap {
namespace pk {

// grid (row tiles, moves): a tile is kThreads x 16 bytes of a row; workgroup (x, y) copies tile x of the rows of moves y,
// y + gridDim.y, .. < count.  row16: 16-byte elements per row; a lane past the row's end does nothing, so nothing is read
// or written outside the two rows of a move.  The table holds (src, dst) as (x, y).
__global__ __launch_bounds__(kThreads) void k_move_rows(const uint4* __restrict__ from, uint4* __restrict__ to, size_t row16,
                                                        const uint2* __restrict__ moves, uint32_t count) {
  const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= row16) return;
#pragma unroll 4
  for (uint32_t k = blockIdx.y; k < count; k += gridDim.y) {
    const uint2 mv = moves[k];
    to[(size_t)mv.y * row16 + t] = from[(size_t)mv.x * row16 + t];
  }
}

}  // namespace pk
}  // namespace cap
