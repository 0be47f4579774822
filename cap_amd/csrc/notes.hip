// The launch of k_move_rows_at (notes_kernels.hpp), in a translation unit of its own: the device code of the prover's
// other units is what it was before capgpu_plonk_prove_notes_dev existed.  plonk.hip builds the move table and calls this.
#include "notes_kernels.hpp"

#include "launch.hpp"
#include "notes.hpp"

namespace cap {

void notes_move_rows(hipStream_t s, const void* from, void* to, uint64_t row16, const np::MoveAt* d_moves, uint32_t count) {
  if (!count || !row16) return;
  launch("k_move_rows_at", np::k_move_rows_at, dim3(np::notes_tiles(row16), std::min<uint32_t>(count, 65535)),
         dim3(np::kNotesTile), 0, s, (const uint4*)from, (uint4*)to, row16, d_moves, count);
}

}  // namespace cap
