// crypto_amd/csrc/k_g1_seg.hip — G1 kernels of the segmented small MSM (seg_kernels.hip.h)
#include "seg_kernels.hip.h"
namespace msm {
template void launch_seg_tree<G1>(hipStream_t, const uint32_t *, const uint8_t *, const uint32_t *, const void *, size_t, uint32_t *, uint8_t *, uint32_t *, uint32_t *, uint8_t *, bool, uint32_t *);
template void launch_seg_fold<G1>(hipStream_t, const uint32_t *, const uint8_t *, size_t, uint32_t *, uint8_t *);
}  // namespace msm
