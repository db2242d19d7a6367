// crypto_amd/csrc/k_serde.hip — the point decoding / validation kernels (serde_kernels.hip.h) and their launchers (serde_launch.hip.h)
#include "serde_kernels.hip.h"
#include "serde_launch.hip.h"

namespace serde {
static dim3 blocks_for(size_t lo, size_t hi) { return dim3((unsigned)((hi - lo + SERDE_BLOCK - 1) / SERDE_BLOCK)); }
void launch_deserialize(hipStream_t s, int nfp, bool compressed, bool validate, const uint32_t *raw, size_t lo, size_t hi, uint32_t *xy, uint8_t *is_inf, uint32_t *first_bad) {
    if (hi <= lo) return;
    const dim3 g = blocks_for(lo, hi), b(SERDE_BLOCK);
    const int v = validate ? 1 : 0;
    if (nfp == 1) {
        if (compressed) hipLaunchKernelGGL((k_deserialize<Fp, true>), g, b, 0, s, raw, lo, hi, v, xy, is_inf, first_bad);
        else hipLaunchKernelGGL((k_deserialize<Fp, false>), g, b, 0, s, raw, lo, hi, v, xy, is_inf, first_bad);
    } else {
        if (compressed) hipLaunchKernelGGL((k_deserialize<Fp2, true>), g, b, 0, s, raw, lo, hi, v, xy, is_inf, first_bad);
        else hipLaunchKernelGGL((k_deserialize<Fp2, false>), g, b, 0, s, raw, lo, hi, v, xy, is_inf, first_bad);
    }
}
void launch_validate_words(hipStream_t s, int nfp, const uint32_t *xy, const uint8_t *is_inf, size_t lo, size_t hi, uint8_t *ok) {
    if (hi <= lo) return;
    if (nfp == 1) hipLaunchKernelGGL((k_validate_words<Fp>), blocks_for(lo, hi), dim3(SERDE_BLOCK), 0, s, xy, is_inf, lo, hi, ok);
    else hipLaunchKernelGGL((k_validate_words<Fp2>), blocks_for(lo, hi), dim3(SERDE_BLOCK), 0, s, xy, is_inf, lo, hi, ok);
}
}  // namespace serde
