// crypto_amd/csrc/k_bbs23.hip — translation unit of the kernels of BBS (2023) proofs of knowledge in bulk (bbs23_kernels.hip.h).
#include "bbs23_kernels.hip.h"
#include "col_launch.hip.h"
#include "bbs23_launch.hip.h"
namespace bbs23k {
static_assert(KIND_CDL == CDL && KIND_IETF == IETF, "one numbering of the proof kinds");
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
static inline ProofIn dev_in(const ProofDev &d) { return ProofIn{d.chal, d.resp, d.vals, d.rev, d.L, (unsigned)shape_of(d.kind).resp, d.mont != 0}; }
KindShape kind_shape(int kind) { const Shape s = shape_of(kind); return KindShape{s.pts, s.resp, s.own, s.segs}; }
void launch_bbs23_rows(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *out_rows, uint32_t *own) {
    const size_t n = in.L + 1, n_own = (size_t)shape_of(in.kind).own;
    hipLaunchKernelGGL(k_bbs23_rows, dim3(blocks_for(rows * n)), dim3(256), 0, s, dev_in(in), rows, n, out_rows);
    if (in.kind == CDL) hipLaunchKernelGGL(k_bbs23_own<CDL>, dim3(blocks_for(rows * n_own)), dim3(256), 0, s, dev_in(in), rows, own);
    else hipLaunchKernelGGL(k_bbs23_own<IETF>, dim3(blocks_for(rows * n_own)), dim3(256), 0, s, dev_in(in), rows, own);
}
void launch_bbs23_stage(hipStream_t s, const uint32_t *points, int kind, size_t rows, uint32_t *own_pts, uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    const unsigned nb = blocks_for(rows * (size_t)(shape_of(kind).own + 2));
    if (kind == CDL) hipLaunchKernelGGL(k_bbs23_stage<CDL>, dim3(nb), dim3(256), 0, s, points, rows, own_pts, pa, pb, skip);
    else hipLaunchKernelGGL(k_bbs23_stage<IETF>, dim3(nb), dim3(256), 0, s, points, rows, own_pts, pa, pb, skip);
}
void launch_bbs23_verdict(hipStream_t s, const uint32_t *seg, const uint8_t *seg_inf, const uint32_t *b, const uint8_t *b_inf, const uint8_t *pairing, const uint8_t *a_inf, int kind,
                          size_t rows, uint8_t *status) {
    if (kind == CDL) hipLaunchKernelGGL(k_bbs23_verdict<CDL>, dim3(blocks_for(rows)), dim3(256), 0, s, seg, seg_inf, b, b_inf, pairing, a_inf, rows, status);
    else hipLaunchKernelGGL(k_bbs23_verdict<IETF>, dim3(blocks_for(rows)), dim3(256), 0, s, seg, seg_inf, b, b_inf, pairing, a_inf, rows, status);
}
void launch_bbs23_columns(hipStream_t s, const ProofDev &in, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *wts,
                          uint32_t *tp, uint32_t *tn, uint32_t *c_words) {
    colk::RhoWords w; for (int k = 0; k < 8; k++) w.w[k] = rho_words[k];
    const size_t n = in.L + 1, nb = colk::col_blocks(rows);
    if (in.kind == CDL) hipLaunchKernelGGL(k_bbs23_col_sums<CDL>, dim3((unsigned)n, (unsigned)nb), dim3(256), 0, s, dev_in(in), w, rows, i0, colk::COL_RUN, part, wts, tp, tn);
    else hipLaunchKernelGGL(k_bbs23_col_sums<IETF>, dim3((unsigned)n, (unsigned)nb), dim3(256), 0, s, dev_in(in), w, rows, i0, colk::COL_RUN, part, wts, tp, tn);
    colk::launch_col_finish(s, part, nb, n, first, 0, 0, run_sums, c_words);
}
}  // namespace bbs23k
