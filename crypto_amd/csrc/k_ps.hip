// crypto_amd/csrc/k_ps.hip — translation unit of the PS (Coconut) scalar kernels (ps_kernels.hip.h).
#include "ps_kernels.hip.h"
#include "ps_launch.hip.h"
namespace psk {
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
void launch_ps_sign_rows(hipStream_t s, const uint32_t *sk, const uint32_t *r, const uint32_t *msgs, int mont, size_t rows, size_t L, uint32_t *out) {
    hipLaunchKernelGGL(k_ps_sign_rows, dim3(blocks_for(rows)), dim3(256), 0, s, sk, r, msgs, mont, rows, L, out);
}
void launch_ps_pok_rows(hipStream_t s, const PokDev &in, size_t rows, uint32_t *out_rows) {
    const PokIn k{in.resp, in.vals, in.rev, in.L, in.mont != 0};
    hipLaunchKernelGGL(k_ps_pok_rows, dim3(blocks_for(2 * rows * (in.L + 2))), dim3(256), 0, s, k, rows, out_rows);
}
void launch_ps_col_scalars(hipStream_t s, const uint32_t *msgs, const uint32_t rho_words[8], int mont, size_t rows, size_t L, size_t i0, size_t cstride, uint32_t *cols) {
    colk::RhoWords w; for (int k = 0; k < 8; k++) w.w[k] = rho_words[k];
    const size_t nb = (rows + 256 * PS_COL_RUN - 1) / (256 * PS_COL_RUN);
    hipLaunchKernelGGL(k_ps_col_scalars, dim3((unsigned)(L + 2), (unsigned)nb), dim3(256), 0, s, msgs, w, mont, rows, L, i0, PS_COL_RUN, cstride, cols);
}
void launch_ps_verdict(hipStream_t s, const uint32_t *got, const uint8_t *got_inf, const uint32_t *t, const uint32_t *sig, const uint8_t *pairing, size_t rows, uint8_t *status) {
    hipLaunchKernelGGL(k_ps_verdict, dim3(blocks_for(rows)), dim3(256), 0, s, got, got_inf, t, sig, pairing, rows, status);
}
}  // namespace psk
