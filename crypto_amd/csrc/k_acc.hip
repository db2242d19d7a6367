// crypto_amd/csrc/k_acc.hip — translation unit of the accumulator witness-update kernels (acc_kernels.hip.h).
#include "acc_kernels.hip.h"
#include "acc_launch.hip.h"
namespace acck {
static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
AccShape acc_shape(size_t m, size_t n_add, size_t n_rem, int forced_split) {
    const size_t n = n_add > n_rem ? n_add : n_rem;
    size_t K = 1;
    if (forced_split > 0) K = (size_t)forced_split;
    else if (m < ACC_FILL_LANES) {
        const size_t want = (ACC_FILL_LANES + m - 1) / m, most = n / ACC_MIN_CHUNK;      // chunks never shorter than ACC_MIN_CHUNK
        K = want < most ? want : most;
    }
    if (K < 1) K = 1;
    if (K > ACC_MAX_SPLIT) K = ACC_MAX_SPLIT;
    size_t per = (m + ACC_SHARE_LANES - 1) / ACC_SHARE_LANES;
    if (per > 32) per = 32;
    return AccShape{(uint32_t)K, (m + per - 1) / per};
}
size_t acc_table_entries(size_t n_add, size_t n_rem) { return 2 * n_add + 2 * n_rem + 1; }
size_t acc_part_bytes(size_t m, AccShape sh) { return sh.K > 1 ? align256((size_t)4 * NL * 4 * sh.K * m) : 0; }
size_t acc_scratch_bytes(size_t m) { return align256((size_t)4 * NL * 4 * m); }
void launch_acc_prep(hipStream_t s, const uint32_t *table_words, size_t entries, uint32_t *tab, int mont) {
    hipLaunchKernelGGL(k_acc_prep, dim3(blocks_for(entries)), dim3(256), 0, s, table_words, entries, tab, mont);
}
void launch_acc_factors(hipStream_t s, const uint32_t *tab, size_t n_add, size_t n_rem, const uint32_t *elems, int mont, size_t m, AccShape sh,
                        uint32_t *part, uint32_t *scratch, uint32_t *fg) {
    if (sh.K == 1) { hipLaunchKernelGGL(k_acc_eval, dim3(blocks_for(sh.G)), dim3(256), 0, s, tab, n_add, n_rem, elems, mont, m, 1u, sh.G, part, scratch, fg); return; }
    hipLaunchKernelGGL(k_acc_eval, dim3(blocks_for(m), sh.K), dim3(256), 0, s, tab, n_add, n_rem, elems, mont, m, sh.K, m, part, scratch, fg);
    hipLaunchKernelGGL(k_acc_combine, dim3(blocks_for(sh.G)), dim3(256), 0, s, tab, n_add, n_rem, part, m, sh.K, sh.G, scratch, fg);
}
void launch_acc_omega_eval(hipStream_t s, const uint32_t *tab, size_t n_add, size_t n_rem, const uint32_t *pts, size_t N, AccShape sh, uint32_t *part, uint32_t *ev) {
    hipLaunchKernelGGL(k_acc_omega_eval, dim3(blocks_for(N), sh.K), dim3(256), 0, s, tab, n_add, n_rem, pts, N, sh.K, part, ev);
    if (sh.K > 1) hipLaunchKernelGGL(k_acc_omega_combine, dim3(blocks_for(N)), dim3(256), 0, s, tab, n_add, n_rem, part, N, sh.K, ev);
}
void launch_acc_omega_coeffs(hipStream_t s, const uint32_t *ev, int logn, const uint32_t ninv_words[8], size_t len, uint32_t *coeff, uint8_t *nz) {
    Words8 w; for (int k = 0; k < 8; k++) w.w[k] = ninv_words[k];
    hipLaunchKernelGGL(k_acc_omega_coeffs, dim3(blocks_for((size_t)1 << logn)), dim3(256), 0, s, ev, logn, w, len, coeff, nz);
}
void launch_acc_pub_factors(hipStream_t s, const uint32_t *lists, size_t n_add, size_t n_rem, const uint32_t *elems, int mont, size_t m, AccShape sh,
                            uint32_t *part, uint32_t *scratch, uint32_t *fs, uint8_t *ok) {
    if (sh.K == 1) { hipLaunchKernelGGL(k_acc_pub_factors, dim3(blocks_for(sh.G)), dim3(256), 0, s, lists, n_add, n_rem, elems, mont, m, 1u, sh.G, part, scratch, fs, ok); return; }
    hipLaunchKernelGGL(k_acc_pub_factors, dim3(blocks_for(m), sh.K), dim3(256), 0, s, lists, n_add, n_rem, elems, mont, m, sh.K, m, part, scratch, fs, ok);
    hipLaunchKernelGGL(k_acc_pub_combine, dim3(blocks_for(sh.G)), dim3(256), 0, s, part, m, sh.K, sh.G, scratch, fs, ok);
}
void launch_acc_pub_rows(hipStream_t s, const uint32_t *elems, int mont, const uint32_t *s_words, size_t rows, size_t n, uint32_t *out_rows) {
    const size_t lanes = rows * ((n + ACC_ROW_RUN - 1) / ACC_ROW_RUN);
    hipLaunchKernelGGL(k_acc_pub_rows, dim3(blocks_for(lanes)), dim3(256), 0, s, elems, mont, s_words, rows, n, ACC_ROW_RUN, out_rows);
}
size_t acc_d_part_bytes(size_t m, uint32_t K) { return K > 1 ? align256((size_t)NL * 4 * K * m) : 0; }
size_t acc_d_run_bytes(size_t m) { return align256((size_t)NL * 4 * m); }
void launch_acc_d(hipStream_t s, const uint32_t *tab, size_t n, const uint32_t *elems, int mont, size_t m, int U, uint32_t K, const uint32_t *d_in, bool first, bool last,
                  uint32_t *part, uint32_t *run, uint32_t *d_words, uint8_t *nz) {
    const DOut o{d_in, run, d_words, nz, m, mont, first ? 1 : 0, last ? 1 : 0};
    const size_t G = acc_d_lanes(m, U);
    if (U == 4) hipLaunchKernelGGL(k_acc_d<4>, dim3(blocks_for(G), K), dim3(256), 0, s, tab, n, elems, m, K, G, part, o);
    else hipLaunchKernelGGL(k_acc_d<1>, dim3(blocks_for(G), K), dim3(256), 0, s, tab, n, elems, m, K, G, part, o);
    if (K > 1) hipLaunchKernelGGL(k_acc_d_combine, dim3(blocks_for(m)), dim3(256), 0, s, part, m, K, o);
}
void launch_acc_issue_scalars(hipStream_t s, const uint32_t *d_words, const uint32_t *t_words, const uint32_t fv_words[8], int mont, size_t m, uint32_t *sc, uint8_t *zero) {
    Words8 w; for (int k = 0; k < 8; k++) w.w[k] = d_words ? fv_words[k] : 0;
    hipLaunchKernelGGL(k_acc_issue_scalars, dim3(blocks_for(m)), dim3(256), 0, s, d_words, t_words, w, mont, d_words ? 1 : 0, m, sc, zero);
}
}  // namespace acck
