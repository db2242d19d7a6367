// crypto_amd/csrc/k_g2_many.hip — G2 kernels of the many-row small MSM (many_kernels.hip.h)
#include "many_kernels.hip.h"
namespace msm {
template void launch_many_tree<G2>(hipStream_t, const uint32_t *, const uint8_t *, const uint32_t *, size_t, size_t, size_t, uint32_t *, uint8_t *, uint32_t *, uint32_t *, uint8_t *, uint32_t *);
template void launch_many_fold<G2>(hipStream_t, const uint32_t *, const uint8_t *, size_t, uint32_t *, uint8_t *);
}  // namespace msm
