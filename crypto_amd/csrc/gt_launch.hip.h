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

// ---- powers, products of powers, membership (k_gt_pow.hip).  G = groups per wave (0: groups_per_wave of the launch's group count) ----
// bases per group of a product of powers over n bases (provisional rule, see its definition)
int bases_per_group(size_t n);
// words of the table workspace launch_gt_pow needs for n bases
size_t pow_table_words(size_t n);
// n bases (ABI, 144 u32 each), exponent of base b at exps + b exp_words (8, or 0: one exponent for all), k bases per group (1 .. 8):
// out element i = prod_j in[i k + j]^(e[i k + j]), ceil(n / k) of them, in the ABI form (144 u32) or the internal one (168 u32: gt_kernels.hip.h)
void launch_gt_pow(hipStream_t s, const uint32_t *in, const uint32_t *exps, int exp_words, size_t n, int G, int k, uint32_t *tab, uint32_t *out, bool out_abi);
// one level of a product: out element i = in[8 i] ... in[8 i + 7]; returns the number of outputs, ceil(n_in / 8)
size_t launch_gt_fold(hipStream_t s, const uint32_t *in, bool in_abi, size_t n_in, int G, uint32_t *out, bool out_abi);
// ok[i] = element i (ABI) lies in GT
void launch_gt_in_subgroup(hipStream_t s, const uint32_t *in, size_t n, int G, uint8_t *ok);
}  // namespace gtk
