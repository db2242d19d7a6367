// crypto_amd/csrc/k_bpp.hip — translation unit of the kernels of Bulletproofs++ range proofs in bulk (bpp_kernels.hip.h).
#include "bpp_kernels.hip.h"
#include "col_launch.hip.h"
#include "bpp_launch.hip.h"
namespace bppk {
static inline unsigned blocks_for(size_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }
static inline Shape shape_of(const ProofDev &d) { return make_shape(d.base, d.num_bits, d.m); }
ShapeInfo bpp_shape(uint32_t base, uint32_t num_bits, uint32_t m) {
    if (!shape_ok(base, num_bits, m)) return ShapeInfo{0, 0, 0, 0, 0};
    const Shape s = make_shape(base, num_bits, m);
    return ShapeInfo{1, (size_t)s.NG, (size_t)s.K, (size_t)s.own, (size_t)(SHARED0 + s.NG)};
}
size_t bpp_rec_words(size_t rows) { return rows * (size_t)REC_N * NL; }
void launch_bpp_consts(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *rec, size_t own_stride, uint32_t *own, uint8_t *bad) {
    hipLaunchKernelGGL(k_bpp_consts, dim3(blocks_for(rows, 64)), dim3(64), 0, s, shape_of(in), in.chal, in.l_n, in.mont != 0, rows, RecDev{rec, rows}, (int)own_stride, own, bad);
}
void launch_bpp_shared(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *rec, uint32_t *out_rows) {
    const Shape sh = shape_of(in);
    hipLaunchKernelGGL(k_bpp_shared, dim3(blocks_for(rows * (size_t)(SHARED0 + sh.NG))), dim3(256), 0, s, sh, rows, RecDev{rec, rows}, out_rows);
}
void launch_bpp_stage(hipStream_t s, const ProofDev &in, const uint32_t *values, const uint32_t *round_points, const uint32_t *wnla_points, const uint32_t *p, const uint8_t *p_inf,
                      size_t rows, uint32_t *bases) {
    const Shape sh = shape_of(in);
    hipLaunchKernelGGL(k_bpp_stage, dim3(blocks_for(rows * (size_t)(sh.own + 1))), dim3(256), 0, s, sh, values, round_points, wnla_points, p, p_inf, rows, bases);
}
void launch_bpp_verdict(hipStream_t s, const uint8_t *seg_inf, const uint8_t *bad, size_t rows, uint8_t *status) {
    hipLaunchKernelGGL(k_bpp_verdict, dim3(blocks_for(rows)), dim3(256), 0, s, seg_inf, bad, rows, status);
}
size_t bpp_part_words(size_t rows, size_t shared) { return colk::col_part_words(rows, shared); }
void launch_bpp_columns(hipStream_t s, const ProofDev &in, const uint32_t *rows_sc, const uint32_t *own, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part,
                        uint32_t *run_sums, uint32_t *wts, uint32_t *c_words) {
    const Shape sh = shape_of(in);
    colk::RhoWords w; for (int k = 0; k < 8; k++) w.w[k] = rho_words[k];
    const size_t nb = colk::col_blocks(rows), cols = (size_t)(SHARED0 + sh.NG);
    hipLaunchKernelGGL(k_bpp_col_sums, dim3((unsigned)cols, (unsigned)nb), dim3(256), 0, s, sh, rows_sc, own, w, in.mont != 0, rows, i0, colk::COL_RUN, part, wts);
    colk::launch_col_finish(s, part, nb, cols, first, 0, 0, run_sums, c_words);
}
}  // namespace bppk
