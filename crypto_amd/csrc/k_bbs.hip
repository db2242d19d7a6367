// crypto_amd/csrc/k_bbs.hip — translation unit of the BBS+ scalar kernels (bbs_kernels.hip.h).
#include "bbs_kernels.hip.h"
#include "bbs_launch.hip.h"
namespace bbsk {
static_assert(BBS_COL_RUN == colk::COL_RUN, "one run length for every column-sum kernel");
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
void launch_bbs_rows(hipStream_t s, const uint32_t *s_words, const uint32_t *msgs, const uint32_t *t_words, int mont, size_t rows, size_t n, size_t fixed,
                     uint32_t *out_rows) {
    hipLaunchKernelGGL(k_bbs_rows, dim3(blocks_for(rows * n)), dim3(256), 0, s, s_words, msgs, t_words, mont, rows, n, fixed, out_rows);
}
void launch_bbs_columns(hipStream_t s, const uint32_t *e, const uint32_t *s_words, const uint32_t *msgs, const uint32_t rho_words[8], int mont, size_t rows, size_t n, size_t fixed,
                        size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *wts, uint32_t *we, uint32_t *c_words) {
    RhoWords w; for (int k = 0; k < 8; k++) w.w[k] = rho_words[k];
    const size_t nb = colk::col_blocks(rows);
    hipLaunchKernelGGL(k_bbs_col_sums, dim3((unsigned)n, (unsigned)nb), dim3(256), 0, s, e, s_words, msgs, w, mont, rows, n, fixed, i0, colk::COL_RUN, part, wts, we);
    colk::launch_col_finish(s, part, nb, n, first, 0, n, run_sums, c_words);      // every column leaves as -c_k
}
}  // namespace bbsk
