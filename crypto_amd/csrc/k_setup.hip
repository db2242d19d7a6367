// crypto_amd/csrc/k_setup.hip — translation unit of the key-generation kernels (setup_kernels.hip.h).
#include "setup_kernels.hip.h"
#include "setup_launch.hip.h"
namespace setupk {
static inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
// lanes of k_lagrange: one Fermat inversion (~430 products) per lane against ~4 products per element, so a lane takes 32 elements up to
// D = 2^21 (65536 lanes at most), more beyond
static size_t lagrange_lanes(size_t D) { const size_t K = D <= ((size_t)1 << 21) ? 32 : D >> 16; return (D + K - 1) / K; }
void launch_lagrange(hipStream_t s, const uint32_t *pw, const uint32_t *consts, size_t D, uint32_t *u) {
    const size_t G = lagrange_lanes(D);
    hipLaunchKernelGGL(k_lagrange, grid_for(G), dim3(256), 0, s, pw, consts, D, G, u);
}
void launch_im_init(hipStream_t s, const uint32_t *u, size_t D, size_t m, size_t num_inputs, size_t nv, uint32_t *a, uint32_t *b, uint32_t *c) {
    hipLaunchKernelGGL(k_im_init, grid_for(nv), dim3(256), 0, s, u, D, m, num_inputs, nv, a, b, c);
}
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t scan_tiles(size_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
size_t col_sum_scratch_bytes(size_t nnz, size_t nv) {
    const size_t p = 2 * ((nnz + FOLD_CHUNK - 1) / FOLD_CHUNK);
    return align256(nnz * 4) + align256(nnz * NL * 4) + align256((nv + 1) * 4) + align256(scan_tiles(nv + 1) * 4) + 2 * (align256(p * 4) + align256(p * NL * 4));
}
void launch_col_sum(hipStream_t s, const uint64_t *rowptr, size_t rows, const uint32_t *cols, const uint32_t *vals, size_t vstride, size_t nnz,
                    const uint32_t *u, size_t D, uint32_t *out, size_t nv, void *scratch) {
    if (nnz == 0) return;
    const size_t p = 2 * ((nnz + FOLD_CHUNK - 1) / FOLD_CHUNK);
    uint8_t *q = (uint8_t *)scratch;
    uint32_t *keys = (uint32_t *)q; q += align256(nnz * 4);
    uint32_t *vv = (uint32_t *)q; q += align256(nnz * NL * 4);
    uint32_t *cnt = (uint32_t *)q; q += align256((nv + 1) * 4);
    const size_t nt = scan_tiles(nv + 1);
    uint32_t *tiles = (uint32_t *)q; q += align256(nt * 4);
    uint32_t *pk[2], *pv[2];
    for (int k = 0; k < 2; k++) { pk[k] = (uint32_t *)q; q += align256(p * 4); pv[k] = (uint32_t *)q; q += align256(p * NL * 4); }
    (void)hipMemsetAsync(cnt, 0, (nv + 1) * 4, s);
    hipLaunchKernelGGL(k_col_count, grid_for(nnz), dim3(256), 0, s, cols, nnz, cnt);
    hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)nt), dim3(SCAN_B), 0, s, cnt, nv + 1, tiles);
    hipLaunchKernelGGL(k_scan_excl, dim3(1), dim3(SCAN_T), 0, s, tiles, nt);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nt), dim3(SCAN_B), 0, s, cnt, nv + 1, tiles);
    hipLaunchKernelGGL(k_col_scatter, grid_for(nnz), dim3(256), 0, s, rowptr, rows, cols, vals, vstride, nnz, u, D, cnt, keys, vv);
    // passes of k_fold until one chunk covers what is left: nnz -> 2 nnz / FOLD_CHUNK -> ...
    const uint32_t *ck = keys, *cv = vv;
    size_t n = nnz;
    for (int lvl = 0;; lvl++) {
        const size_t nch = (n + FOLD_CHUNK - 1) / FOLD_CHUNK;
        const bool fin = nch == 1;
        uint32_t *ok = pk[lvl & 1], *ov = pv[lvl & 1];
        hipLaunchKernelGGL(k_fold, grid_for(nch), dim3(256), 0, s, ck, cv, n, FOLD_CHUNK, (int)fin, out, nv, ok, ov);
        if (fin) break;
        ck = ok; cv = ov; n = 2 * nch;
    }
}
void launch_soa_to_words(hipStream_t s, const uint32_t *src, size_t n, int mont, uint32_t *words) {
    if (n) hipLaunchKernelGGL(k_soa_to_words, grid_for(n), dim3(256), 0, s, src, n, mont, words);
}
void launch_key_scalars(hipStream_t s, const uint32_t *a, const uint32_t *b, const uint32_t *c, size_t nv, size_t n_abc, const uint32_t *consts,
                        uint32_t *a_w, uint32_t *b_w, uint32_t *abc_w, uint32_t *l_w) {
    hipLaunchKernelGGL(k_key_scalars, grid_for(nv), dim3(256), 0, s, a, b, c, nv, n_abc, consts, a_w, b_w, abc_w, l_w);
}
}  // namespace setupk
