// crypto_amd/csrc/k_smc.hip — translation unit of the kernels of range proofs over weak-BB signatures in bulk (smc_kernels.hip.h).
#include "smc_kernels.hip.h"
#include "col_launch.hip.h"
#include "smc_launch.hip.h"
namespace smck {
static_assert(SMC_MAX_L == MAX_L && SMC_STMT_CONSTS == (size_t)STMT_CONSTS, "one shape of the statement");
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
static inline ProofIn dev_in(const ProofDev &d) { return ProofIn{d.chal, d.zr, d.z, d.stmt, d.sides, d.l, d.mont != 0}; }
void launch_smc_own(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *own) {
    hipLaunchKernelGGL(k_smc_own, dim3(blocks_for(rows * eq_count(in.sides, in.l))), dim3(256), 0, s, dev_in(in), rows, own);
}
void launch_smc_stage(hipStream_t s, const uint32_t *commitments, const uint32_t *side_points, const uint32_t *digit_points, const uint32_t *shared, int sides, int l, size_t rows,
                      uint32_t *bases, uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    SharedPoints sp;
    for (int q = 0; q < 3; q++) for (int k = 0; k < 2 * FQW; k++) sp.w[q][k] = shared[q * 2 * FQW + k];
    hipLaunchKernelGGL(k_smc_stage, dim3(blocks_for(rows * eq_count(sides, l) * 6)), dim3(256), 0, s, commitments, side_points, digit_points, sp, sides, l, rows, bases, pa, pb, skip);
}
void launch_smc_verdict(hipStream_t s, const uint8_t *seg_inf, const uint8_t *pairing, const uint8_t *skip, int sides, int l, bool merged, size_t rows, uint8_t *status,
                        int32_t *detail) {
    hipLaunchKernelGGL(k_smc_verdict, dim3(blocks_for(rows)), dim3(256), 0, s, seg_inf, pairing, skip, sides, l, merged, rows, status, detail);
}
void launch_smc_merge_weights(hipStream_t s, const uint32_t *random, int sides, int l, int mont, size_t rows, uint32_t *tw) {
    hipLaunchKernelGGL(k_smc_merge_weights, dim3(blocks_for(rows * digit_count(sides, l))), dim3(256), 0, s, random, sides, l, mont != 0, rows, tw);
}
void launch_smc_merged_sides(hipStream_t s, const uint32_t *sums, const uint8_t *inf, size_t rows, uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    hipLaunchKernelGGL(k_smc_merged_sides, dim3(blocks_for(2 * rows)), dim3(256), 0, s, sums, inf, rows, pa, pb, skip);
}
size_t smc_part_words(size_t rows, int sides, int l) { return colk::col_part_words(rows * eq_count(sides, l), 3); }
void launch_smc_columns(hipStream_t s, const uint32_t *own, const uint32_t rho_words[8], int sides, int l, int mont, size_t rows, size_t i0, bool first, uint32_t *part,
                        uint32_t *run_sums, uint32_t *w_side, uint32_t *w_digit, uint32_t *tp, uint32_t *tn, uint32_t *c_words) {
    colk::RhoWords w; for (int k = 0; k < 8; k++) w.w[k] = rho_words[k];
    const size_t nb = colk::col_blocks(rows * eq_count(sides, l));
    hipLaunchKernelGGL(k_smc_col_sums, dim3(3, (unsigned)nb), dim3(256), 0, s, own, w, sides, l, mont != 0, rows, i0 * eq_count(sides, l), i0 * digit_count(sides, l), colk::COL_RUN,
                       part, w_side, w_digit, tp, tn);
    colk::launch_col_finish(s, part, nb, 3, first, 0, 0, run_sums, c_words);
}
}  // namespace smck
