// crypto_amd/csrc/k_cols.hip — translation unit of the column sums' second pass, one kernel for every batch verifier (col_sums.hip.h, col_launch.hip.h).
#include "col_sums.hip.h"
#include "col_launch.hip.h"
namespace colk {
// one lane per column: the chunk's block sums onto the running sum (run_sums[k * NL ..], internal form; first: it starts from zero), in block order; the running
// sum goes back, and out_words[8 k ..] = the canonical words of -c_k (neg_lo <= k < neg_hi) or c_k as they stand after this chunk.
__global__ void __launch_bounds__(64) k_col_finish(const uint32_t *__restrict__ part, size_t nparts, size_t ncols, int first, size_t neg_lo, size_t neg_hi,
                                                   uint32_t *__restrict__ run_sums, uint32_t *__restrict__ out_words) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ncols) return;
    Fr start, c, o;
    if (first) fr_zero(start); else for (int l = 0; l < NL; l++) start.l[l] = run_sums[k * NL + l];
    col_finish(start, nparts, [&](size_t b, Fr &v) { for (int l = 0; l < NL; l++) v.l[l] = part[(k * nparts + b) * NL + l]; }, c);
    for (int l = 0; l < NL; l++) run_sums[k * NL + l] = c.l[l];
    if (k >= neg_lo && k < neg_hi) neg_product(o, c); else o = c;
    st_words(out_words, k, o);
}
size_t col_blocks(size_t count) { return (count + 256 * COL_RUN - 1) / (256 * COL_RUN); }
size_t col_part_words(size_t count, size_t ncols) { return col_blocks(count) * ncols * NL; }
void launch_col_finish(hipStream_t s, const uint32_t *part, size_t nparts, size_t ncols, bool first, size_t neg_lo, size_t neg_hi, uint32_t *run_sums, uint32_t *out_words) {
    hipLaunchKernelGGL(k_col_finish, dim3((unsigned)((ncols + 63) / 64)), dim3(64), 0, s, part, nparts, ncols, first ? 1 : 0, neg_lo, neg_hi, run_sums, out_words);
}
}  // namespace colk
