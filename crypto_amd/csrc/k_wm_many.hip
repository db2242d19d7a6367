// crypto_amd/csrc/k_wm_many.hip — translation unit of the block witness map (wm_block_kernels.hip.h) and its launcher.
#include <atomic>
#include "wm_block_kernels.hip.h"
#include "qap_launch.hip.h"
namespace ntt {
static_assert(WM_BLOCK_MAX_LOG == PIPE_TILE_LOG, "the block kernel takes exactly the domains run_passes sends to one pass per stage, and the first piped one");
void launch_wm_block(hipStream_t s, const WmCircuit &c, const WmTables &tb, const WmJob &j) {
    const uint32_t T = j.rows_per_block << j.logn;                                  // elements per array and block
    const size_t lds_bytes = (size_t)3 * NL * T * 4;
    // (the attribute belongs to the function ON THE CURRENT DEVICE: a process that drives several GPUs sets it once per device)
    { static std::atomic<uint32_t> done{0}; int dev = 0; (void)hipGetDevice(&dev); const uint32_t bit = 1u << (dev & 31);
      if (!(done.load() & bit)) { (void)hipFuncSetAttribute((const void *)k_wm_block, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * NL * (4 << WM_BLOCK_MAX_LOG)); done.fetch_or(bit); } }
    // one radix-4 unit per lane over the three arrays, whole waves, at least two of them
    uint32_t threads = (3 * (T >> 2) + 63) & ~63u;
    if (threads < 128) threads = 128;
    if (threads > (uint32_t)WM_BLOCK_THREADS) threads = WM_BLOCK_THREADS;
    const uint32_t blocks = (j.nrows + j.rows_per_block - 1) / j.rows_per_block;
    hipLaunchKernelGGL(k_wm_block, dim3(blocks), dim3(threads), lds_bytes, s, c, tb, j);
}
}  // namespace ntt
