// crypto_amd/csrc/k_acc_gt.hip — translation unit of the kernels of the accumulator proofs with a GT commitment in bulk (acc_gt_kernels.hip.h).
#include "acc_gt_kernels.hip.h"
#include "col_launch.hip.h"
#include "acc_gt_launch.hip.h"
namespace accgt {
static_assert(KIND_MEMBERSHIP == MEMBERSHIP && KIND_NON_MEMBERSHIP == NON_MEMBERSHIP, "one numbering of the proof kinds");
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
static inline ProofIn dev_in(const ProofDev &d) { return ProofIn{d.chal, d.resp, d.kind, d.mont != 0}; }
KindShape kind_shape(int kind) { const Shape s = shape_of(kind); return KindShape{s.pts, s.resp, s.own, s.segs, s.checks, s.g1cols, s.pcols}; }
void kind_seg_ends(int kind, unsigned ends[8]) { for (int g = 0; g < shape_of(kind).segs; g++) ends[g] = seg_end(kind, (unsigned)g); }
void launch_acc_gt_own(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *own) {
    hipLaunchKernelGGL(k_acc_gt_own, dim3(blocks_for(rows * shape_of(in.kind).own)), dim3(256), 0, s, dev_in(in), rows, own);
}
void launch_acc_gt_stage(hipStream_t s, const uint32_t *points, const uint32_t *shared, int kind, size_t rows, uint32_t *bases) {
    SharedPoints sp;
    for (int q = 0; q < N_SHARED; q++) for (int k = 0; k < 2 * FQW; k++) sp.w[q][k] = shared[q * 2 * FQW + k];
    hipLaunchKernelGGL(k_acc_gt_stage, dim3(blocks_for(rows * shape_of(kind).own)), dim3(256), 0, s, points, sp, kind, rows, bases);
}
void launch_acc_gt_sides(hipStream_t s, const uint32_t *sums, const uint8_t *inf, int kind, size_t rows, uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    hipLaunchKernelGGL(k_acc_gt_sides, dim3(blocks_for(2 * rows)), dim3(256), 0, s, sums, inf, kind, rows, pa, pb, skip);
}
void launch_acc_gt_verdict(hipStream_t s, const uint8_t *seg_inf, const uint32_t *gt, const uint32_t *r_e, int kind, size_t rows, uint8_t *status) {
    hipLaunchKernelGGL(k_acc_gt_verdict, dim3(blocks_for(rows)), dim3(256), 0, s, seg_inf, gt, r_e, kind, rows, status);
}
size_t acc_gt_part_words(size_t rows, int kind) { return colk::col_part_words(rows, (size_t)cols_of(kind)); }
void launch_acc_gt_columns(hipStream_t s, const ProofDev &in, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *wts,
                           uint32_t *wp, uint32_t *wq, uint32_t *tp, uint32_t *c_words) {
    colk::RhoWords w; for (int k = 0; k < 8; k++) w.w[k] = rho_words[k];
    const size_t n = (size_t)cols_of(in.kind), nb = colk::col_blocks(rows);
    if (in.kind == MEMBERSHIP) hipLaunchKernelGGL(k_acc_gt_col_sums<MEMBERSHIP>, dim3((unsigned)n, (unsigned)nb), dim3(256), 0, s, dev_in(in), w, rows, i0, colk::COL_RUN, part, wts, wp, wq, tp);
    else hipLaunchKernelGGL(k_acc_gt_col_sums<NON_MEMBERSHIP>, dim3((unsigned)n, (unsigned)nb), dim3(256), 0, s, dev_in(in), w, rows, i0, colk::COL_RUN, part, wts, wp, wq, tp);
    // the columns of the two sides (Z, V [, K] and Z) enter p and q negated
    colk::launch_col_finish(s, part, nb, n, first, (size_t)shape_of(in.kind).g1cols, n, run_sums, c_words);
}
}  // namespace accgt
