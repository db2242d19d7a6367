// crypto_amd/csrc/k_pairing.hip — the Miller-loop kernels (pairing_kernels.hip.h) and their launchers (pairing_launch.hip.h): every launch geometry and every choice between two kernels of one job, once
#include "pairing_kernels.hip.h"
#include "pairing_launch.hip.h"
#include <atomic>

namespace mlk {
constexpr size_t ML_HEX_MAX = 4096;           // 16 lanes x 4096 pairs = 1024 waves: one per SIMD
constexpr size_t LP3_MAX_BLOCKS = 512;        // two blocks of three waves per CU

int chain_steps(int b_hi, int b_lo) { return ml_steps(b_hi, b_lo); }

void launch_lines_eval(hipStream_t s, const uint32_t *p_abi, const uint32_t *q_abi, const uint8_t *skip, size_t n, uint32_t *lines, size_t stride, int lanes) {
    const dim3 grid((unsigned)((lanes * n + 63) / 64)), block(64);
    if (lanes == 1) hipLaunchKernelGGL(k_miller_lines, grid, block, 0, s, p_abi, q_abi, skip, n, lines, stride);
    else if (lanes == 2) hipLaunchKernelGGL(k_miller_lines_pair, grid, block, 0, s, p_abi, q_abi, skip, n, lines, stride);
    else hipLaunchKernelGGL(k_miller_lines_quad<true>, grid, block, 0, s, p_abi, q_abi, skip, n, lines, stride);
}
void launch_lines_uneval(hipStream_t s, int mode, const uint32_t *p_abi, const uint32_t *q_abi, const uint8_t *skip, size_t n, uint32_t *lines, size_t stride, int b_hi, int b_lo, int s_first, uint32_t *state, uint32_t *pxy) {
    if ((mode & 8) && (mode & 4) && n <= ML_HEX_MAX)
        hipLaunchKernelGGL(k_miller_lines_ws, dim3((unsigned)((n + WS_PAIRS - 1) / WS_PAIRS)), dim3(256), 0, s, p_abi, q_abi, skip, n, lines, stride, b_hi, b_lo, s_first, state, pxy);
    else if ((mode & 4) && n <= ML_HEX_MAX)
        hipLaunchKernelGGL(k_miller_lines_hex, dim3((unsigned)((16 * n + 63) / 64)), dim3(64), 0, s, p_abi, q_abi, skip, n, lines, stride, b_hi, b_lo, s_first, state, pxy);
    else
        hipLaunchKernelGGL(k_miller_lines_quad<false>, dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, s, p_abi, q_abi, skip, n, lines, stride, b_hi, b_lo, s_first, state, pxy);
}
void launch_lines_from_prepared(hipStream_t s, const uint32_t *p_abi, const uint32_t *coeffs, const uint8_t *skip, size_t n, uint32_t *lines, size_t stride, uint32_t *pxy, bool shared) {
    hipLaunchKernelGGL(k_lines_from_prepared, dim3((unsigned)((n * N_LINES + 255) / 256)), dim3(256), 0, s, p_abi, coeffs, skip, n, lines, stride, pxy, shared);
}
void launch_g2_prepare(hipStream_t s, const uint32_t *q_abi, const uint8_t *is_inf, size_t n, uint32_t *out, uint8_t *out_inf) {
    hipLaunchKernelGGL(k_g2_prepare, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, s, q_abi, is_inf, n, out, out_inf);
}
void launch_prepared_from_lines(hipStream_t s, const uint32_t *lines, const uint32_t *q_abi, const uint8_t *is_inf, size_t n, uint32_t *out, uint8_t *out_inf) {
    hipLaunchKernelGGL(k_prepared_from_lines, dim3((unsigned)((n * N_LINES * 6 + 255) / 256)), dim3(256), 0, s, lines, q_abi, is_inf, n, out, out_inf);
}
void launch_line_products(hipStream_t s, int mode, const uint32_t *lines, size_t n, int slice_len, int nsl, uint32_t *partial, const uint32_t *seg_off, int nseg, int s0, int ns, const uint32_t *pxy, bool allow3) {
    const size_t chains = (size_t)ns * nsl * nseg, blocks3 = (chains + 31) / 32;
    if (allow3 && blocks3 <= (LP3_MAX_BLOCKS << ((mode >> 28) & 3)) && (mode & 16))
        hipLaunchKernelGGL(k_line_products3, dim3((unsigned)blocks3), dim3(192), 0, s, lines, n, slice_len, nsl, partial, s0, ns, pxy, seg_off, nseg);
    else
        hipLaunchKernelGGL(k_line_products, dim3((unsigned)((2 * chains + 63) / 64)), dim3(64), 0, s, lines, n, slice_len, nsl, partial, seg_off, nseg, s0, ns, pxy);
}
void launch_product_tree(hipStream_t s, int mode, unsigned blocks, const uint32_t *partial, int nsl, int ngroups, uint32_t *next, uint32_t *out_abi, const uint32_t *seg_off, int slice_len, int s0, int ns) {
    if (mode & 2) {
        static std::atomic<uint32_t> done{0};
        { int dev = 0; (void)hipGetDevice(&dev); const uint32_t bit = 1u << (dev & 31);
          if (!(done.load() & bit)) { (void)hipFuncSetAttribute((const void *)k_product_tree18, hipFuncAttributeMaxDynamicSharedMemorySize, (int)T18_LDS); done.fetch_or(bit); } }
        hipLaunchKernelGGL(k_product_tree18, dim3(blocks), dim3(T18_THREADS), T18_LDS, s, partial, nsl, ngroups, next, out_abi, seg_off, slice_len, s0, ns);
    } else
        hipLaunchKernelGGL(k_product_tree, dim3(blocks), dim3(192), 0, s, partial, nsl, ngroups, next, out_abi, seg_off, slice_len, s0, ns);
}
void launch_pxy_from_abi(hipStream_t s, const uint32_t *p_abi, size_t n, uint32_t *pxy, size_t stride) {
    hipLaunchKernelGGL(k_pxy_from_abi, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, s, p_abi, n, pxy, stride);
}
}  // namespace mlk
