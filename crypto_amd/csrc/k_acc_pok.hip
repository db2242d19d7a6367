// crypto_amd/csrc/k_acc_pok.hip — translation unit of the kernels of accumulator proofs in bulk (acc_pok_kernels.hip.h).
#include "acc_pok_kernels.hip.h"
#include "col_launch.hip.h"
#include "acc_pok_launch.hip.h"
namespace accpk {
static_assert(KIND_MEMBERSHIP == MEMBERSHIP && KIND_NON_MEMBERSHIP == NON_MEMBERSHIP, "one numbering of the proof kinds");
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
static inline ProofIn dev_in(const ProofDev &d) { return ProofIn{d.chal, d.resp, d.kind, d.mont != 0}; }
KindShape kind_shape(int kind) { const Shape s = shape_of(kind); return KindShape{s.pts, s.resp, s.own, s.segs, s.shared}; }
void launch_acc_pok_own(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *own) {
    hipLaunchKernelGGL(k_acc_pok_own, dim3(blocks_for(rows * shape_of(in.kind).own)), dim3(256), 0, s, dev_in(in), rows, own);
}
void launch_acc_pok_stage(hipStream_t s, const uint32_t *points, const uint32_t *shared, int kind, size_t rows, uint32_t *own_pts, uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    const Shape sh = shape_of(kind);
    SharedPoints sp;
    for (int q = 0; q < MAX_SHARED; q++) for (int k = 0; k < 2 * FQW; k++) sp.w[q][k] = q < sh.shared ? shared[q * 2 * FQW + k] : 0;
    hipLaunchKernelGGL(k_acc_pok_stage, dim3(blocks_for(rows * (sh.own + 2))), dim3(256), 0, s, points, sp, kind, rows, own_pts, pa, pb, skip);
}
void launch_acc_pok_verdict(hipStream_t s, const uint8_t *seg_inf, const uint8_t *pairing, const uint8_t *skip, int kind, size_t rows, uint8_t *status) {
    hipLaunchKernelGGL(k_acc_pok_verdict, dim3(blocks_for(rows)), dim3(256), 0, s, seg_inf, pairing, skip, kind, rows, status);
}
size_t acc_pok_part_words(size_t rows, int kind) { return colk::col_part_words(rows, (size_t)shape_of(kind).shared); }
void launch_acc_pok_columns(hipStream_t s, const ProofDev &in, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *wts,
                            uint32_t *tp, uint32_t *tn, uint32_t *c_words) {
    colk::RhoWords w; for (int k = 0; k < 8; k++) w.w[k] = rho_words[k];
    const size_t n = (size_t)shape_of(in.kind).shared, nb = colk::col_blocks(rows);
    if (in.kind == MEMBERSHIP) hipLaunchKernelGGL(k_acc_pok_col_sums<MEMBERSHIP>, dim3((unsigned)n, (unsigned)nb), dim3(256), 0, s, dev_in(in), w, rows, i0, colk::COL_RUN, part, wts, tp, tn);
    else hipLaunchKernelGGL(k_acc_pok_col_sums<NON_MEMBERSHIP>, dim3((unsigned)n, (unsigned)nb), dim3(256), 0, s, dev_in(in), w, rows, i0, colk::COL_RUN, part, wts, tp, tn);
    // the P of a non-membership proof (column 1) enters its check as -s_d P
    colk::launch_col_finish(s, part, nb, n, first, in.kind == MEMBERSHIP ? 0 : 1, in.kind == MEMBERSHIP ? 0 : 2, run_sums, c_words);
}
}  // namespace accpk
