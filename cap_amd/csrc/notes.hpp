// notes.hip: the gather of capgpu_plonk_prove_notes_dev.  `count` moves on stream s: move k copies d_moves[k].len16 units
// of 16 bytes from (const char*)from + 32 * d_moves[k].src to row k of `to`, rows row16 units apart (notes_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "notes_plan.hpp"

namespace cap {
void notes_move_rows(hipStream_t s, const void* from, void* to, uint64_t row16, const np::MoveAt* d_moves, uint32_t count);
}  // namespace cap
