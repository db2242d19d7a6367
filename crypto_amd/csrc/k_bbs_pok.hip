// crypto_amd/csrc/k_bbs_pok.hip — translation unit of the kernels of BBS+ proofs of knowledge in bulk (bbs_pok_kernels.hip.h).
#include "bbs_pok_kernels.hip.h"
#include "col_launch.hip.h"
#include "bbs_pok_launch.hip.h"
namespace bbspk {
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
static inline PokIn dev_in(const PokDev &d) { return PokIn{d.chal, d.fixed, d.vals, d.rev, d.L, d.mont != 0}; }
void launch_pok_rows(hipStream_t s, const PokDev &in, size_t rows, uint32_t *out_rows, uint32_t *own) {
    const size_t n = in.L + 2;
    hipLaunchKernelGGL(k_bbs_pok_rows, dim3(blocks_for(rows * n)), dim3(256), 0, s, dev_in(in), rows, n, out_rows);
    hipLaunchKernelGGL(k_bbs_pok_own, dim3(blocks_for(rows * POK_OWN)), dim3(256), 0, s, dev_in(in), rows, own);
}
void launch_pok_stage(hipStream_t s, const uint32_t *points, const uint32_t h0[24], size_t rows, uint32_t *own_pts, uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    PointWords h; for (int k = 0; k < 24; k++) h.w[k] = h0[k];
    hipLaunchKernelGGL(k_bbs_pok_stage, dim3(blocks_for(rows * 9)), dim3(256), 0, s, points, h, rows, own_pts, pa, pb, skip);
}
void launch_pok_verdict(hipStream_t s, const uint32_t *seg, const uint8_t *seg_inf, const uint32_t *b, const uint8_t *b_inf, const uint8_t *pairing, const uint8_t *a_inf, size_t rows,
                        uint8_t *status) {
    hipLaunchKernelGGL(k_bbs_pok_verdict, dim3(blocks_for(rows)), dim3(256), 0, s, seg, seg_inf, b, b_inf, pairing, a_inf, rows, status);
}
void launch_pok_columns(hipStream_t s, const PokDev &in, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *w5,
                        uint32_t *tp, uint32_t *tn, uint32_t *c_words) {
    colk::RhoWords w; for (int k = 0; k < 8; k++) w.w[k] = rho_words[k];
    const size_t n = in.L + 2, nb = colk::col_blocks(rows);
    hipLaunchKernelGGL(k_bbs_pok_col_sums, dim3((unsigned)n, (unsigned)nb), dim3(256), 0, s, dev_in(in), w, rows, i0, colk::COL_RUN, part, w5, tp, tn);
    colk::launch_col_finish(s, part, nb, n, first, 0, 0, run_sums, c_words);
}
}  // namespace bbspk
