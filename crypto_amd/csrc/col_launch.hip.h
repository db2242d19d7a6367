// crypto_amd/csrc/col_launch.hip.h — the launch side of the column sums every batch verifier shares (col_sums.hip.h: the routines and the block frame; k_cols.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace colk {
// COL_RUN  rows per lane of a k_*_col_sums kernel.  UNMEASURED.  A lane pays at most 2 log2(n) products for its start power, then two per row
//          plus the conversions of its operands: at 16 the start costs at most 2 x 17 products against ~64.  A block covers 256 x 16 rows of one column.
constexpr size_t COL_RUN = 16;
// blocks of a sums kernel per column for a chunk of `count` rows, and the words of its partial sums for ncols columns
size_t col_blocks(size_t count);
size_t col_part_words(size_t count, size_t ncols);
// One lane per column k < ncols: the chunk's block sums part[(k * nparts + b) * 10 ..] onto the running sum (run_sums[10 k ..], internal form; first: it starts
// from zero), in block order; the running sum goes back, and out_words[8 k ..] = the canonical words of the sum as it stands after this chunk — of minus the
// sum for the columns in [neg_lo, neg_hi).
void launch_col_finish(hipStream_t s, const uint32_t *part, size_t nparts, size_t ncols, bool first, size_t neg_lo, size_t neg_hi, uint32_t *run_sums, uint32_t *out_words);
}  // namespace colk
