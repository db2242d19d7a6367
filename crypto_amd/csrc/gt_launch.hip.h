// crypto_amd/csrc/gt_launch.hip.h — launchers of the batched GT kernels (k_gt.hip, gt_kernels.hip.h) for the host units
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace gtk {
// groups of six lanes per 64-lane wave for n elements: up to ten, fewer while the chip would hold less than GT_MIN_WAVES waves
int groups_per_wave(size_t n);
// out_f12 (m x 144 u32, ABI) = the Miller output of each of m segments from its 68 per-step products in k_line_products' layout
// (partial[(s * m + j) * 12 NL + word], the internal 29-bit form)
void launch_miller_tail(hipStream_t s, const uint32_t *partial, size_t m, uint32_t *out_f12);
// final exponentiation of n ABI elements.  out_gt / is_zero may be NULL; want != NULL: ok[i] = 1 iff element i is not zero and its GT value
// equals want (144 u32)
void launch_final_exp(hipStream_t s, const uint32_t *in_f12, size_t n, uint32_t *out_gt, uint8_t *is_zero, const uint32_t *want, uint8_t *ok);
}  // namespace gtk
