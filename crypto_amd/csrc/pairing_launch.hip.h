// crypto_amd/csrc/pairing_launch.hip.h — launchers of the Miller-loop kernels (k_pairing.hip, pairing_kernels.hip.h) for the host units,
// and the sizes the host allocates their buffers by.  `mode` is dgpu_set_miller_pipeline's word (Shared::ml_mode), read once by the caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mlk {
constexpr int N_LINES = 68;       // line steps of the loop: 63 doublings + 5 additions
constexpr int FPW = 14;           // u32 per Fp in the internal form (fp29.hip.h NL)
constexpr int LW = 6 * FPW;       // u32 per sparse line (3 Fp2)
constexpr int F12W = 12 * FPW;    // u32 per dense Fp12
constexpr int MAX_SLICES = 64;    // partials one tree block folds
constexpr int STATE_W = 3 * 4 * FPW;      // u32 per pair of a cut chain's state: R on every lane of the quad (the sixteen-lane forms need half)
constexpr int PXY_W = 2 * FPW;            // u32 per pair of px, py beside unevaluated lines

// line steps of the bits b_hi .. b_lo of |x|
int chain_steps(int b_hi, int b_lo);

// K9, evaluated at P: lines[(s * LW + k) * stride + i].  lanes per pair: 1, 2 or 4
void launch_lines_eval(hipStream_t s, const uint32_t *p_abi, const uint32_t *q_abi, const uint8_t *skip, size_t n, uint32_t *lines, size_t stride, int lanes);
// K9, the evaluation left to the product kernel (px, py go to pxy by the launch that starts the chain): sixteen lanes per pair while the chip has
// room for them (mode bit 2; bit 3: a wave per role), four otherwise.  Bits b_hi .. b_lo, lines from s_first on; R travels through `state`
// (STATE_W words per pair) between the launches of a cut chain.  p_abi == nullptr: the coefficients alone
void launch_lines_uneval(hipStream_t s, int mode, const uint32_t *p_abi, const uint32_t *q_abi, const uint8_t *skip, size_t n, uint32_t *lines, size_t stride, int b_hi, int b_lo, int s_first, uint32_t *state, uint32_t *pxy);
// (P, ell_coeffs) -> evaluated lines; pxy != nullptr: the pairs' neutral px, py for a product kernel that evaluates; shared: one coefficient set for every pair
void launch_lines_from_prepared(hipStream_t s, const uint32_t *p_abi, const uint32_t *coeffs, const uint8_t *skip, size_t n, uint32_t *lines, size_t stride, uint32_t *pxy = nullptr, bool shared = false);
// Q -> ell_coeffs in the ABI form: the whole chain on a lane pair, or from the unevaluated lines a line kernel left
void launch_g2_prepare(hipStream_t s, const uint32_t *q_abi, const uint8_t *is_inf, size_t n, uint32_t *out, uint8_t *out_inf);
void launch_prepared_from_lines(hipStream_t s, const uint32_t *lines, const uint32_t *q_abi, const uint8_t *is_inf, size_t n, uint32_t *out, uint8_t *out_inf);
// K10 for the steps s0 .. s0 + ns - 1 of nseg segments (seg_off == nullptr, nseg == 1: one loop over all n pairs): partial[((g * N_LINES + s) * nsl + j) * F12W].
// allow3: three waves per product while the launch leaves the chip nearly empty (mode bit 4)
void launch_line_products(hipStream_t s, int mode, const uint32_t *lines, size_t n, int slice_len, int nsl, uint32_t *partial, const uint32_t *seg_off, int nseg, int s0, int ns, const uint32_t *pxy, bool allow3);
// K11, one level: `blocks` = (segment, step, group) (mode bit 1: the 18-role form)
void launch_product_tree(hipStream_t s, int mode, unsigned blocks, const uint32_t *partial, int nsl, int ngroups, uint32_t *next, uint32_t *out_abi, const uint32_t *seg_off, int slice_len, int s0, int ns);
// affine ABI points on the device -> px, py in the internal form: pxy[(c * FPW + k) * stride + i]
void launch_pxy_from_abi(hipStream_t s, const uint32_t *p_abi, size_t n, uint32_t *pxy, size_t stride);
}  // namespace mlk
