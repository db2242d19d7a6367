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
void launch_acc_prep(hipStream_t s, const uint32_t *table_words, size_t entries, uint32_t *tab) {
    hipLaunchKernelGGL(k_acc_prep, dim3(blocks_for(entries)), dim3(256), 0, s, table_words, entries, tab);
}
void launch_acc_factors(hipStream_t s, const uint32_t *tab, size_t n_add, size_t n_rem, const uint32_t *elems, int mont, size_t m, AccShape sh,
                        uint32_t *part, uint32_t *scratch, uint32_t *fg) {
    if (sh.K == 1) { hipLaunchKernelGGL(k_acc_eval, dim3(blocks_for(sh.G)), dim3(256), 0, s, tab, n_add, n_rem, elems, mont, m, 1u, sh.G, part, scratch, fg); return; }
    hipLaunchKernelGGL(k_acc_eval, dim3(blocks_for(m), sh.K), dim3(256), 0, s, tab, n_add, n_rem, elems, mont, m, sh.K, m, part, scratch, fg);
    hipLaunchKernelGGL(k_acc_combine, dim3(blocks_for(sh.G)), dim3(256), 0, s, tab, n_add, n_rem, part, m, sh.K, sh.G, scratch, fg);
}
}  // namespace acck
