// crypto_amd/csrc/k_saver.hip — translation unit of the SAVER kernels (saver_kernels.hip.h): the GT power table in k_gt_pow.hip's layout (one product
// per group of six lanes, G groups per 64-lane wave, a wave per block), the discrete-log lookup and the row verdict (one lane per value / per row).
#include "gt_lanes.hip.h"
#include "gt_launch.hip.h"
#include "saver_kernels.hip.h"
#include "saver_launch.hip.h"

namespace {
using namespace bls29;

// group i of n = K cnt: column i / cnt, k = i % cnt + 1.  Reads entries <= half, writes entries > half: no group reads what another writes.
__global__ void __launch_bounds__(64) k_gt_table_extend(uint32_t *tab, size_t n, int G, uint32_t E, uint32_t half, uint32_t cnt) {
    GT_GROUP_PROLOGUE
    (void)q;
    const size_t j = i / cnt, k = i % cnt + 1;
    uint32_t *col = tab + j * E * (size_t)GT_ABIW;
    saverk::table_extend_group(x, col + (size_t)(half - 1) * GT_ABIW, col + (k - 1) * GT_ABIW, col + (half + k - 1) * GT_ABIW);
}
}  // namespace

namespace saverk {
void launch_gt_table_extend(hipStream_t s, uint32_t *tab, size_t K, uint32_t E, uint32_t half, uint32_t cnt) {
    const size_t n = K * cnt;
    if (!n) return;
    const int G = gtk::groups_per_wave(n);
    hipLaunchKernelGGL(k_gt_table_extend, dim3((unsigned)((n + G - 1) / G)), dim3(64), 0, s, tab, n, G, E, half, cnt);
}
void launch_gt_dlog_lookup(hipStream_t s, const uint32_t *p, size_t rows, size_t K, const DkDev &dk, bool at_index, uint16_t *chunks, uint8_t *miss) {
    if (!rows || !K) return;
    const DkIndex ix{dk.tab, dk.fps, dk.ms, dk.one, dk.E, dk.mask};
    hipLaunchKernelGGL(k_gt_dlog_lookup, dim3((unsigned)((rows * K + 63) / 64)), dim3(64), 0, s, p, rows, K, ix, at_index ? 1 : 0, chunks, miss);
}
void launch_saver_row_verdict(hipStream_t s, const uint8_t *miss, size_t rows, size_t K, uint16_t *chunks, const uint8_t *extra, bool invert, uint8_t *status) {
    if (!rows) return;
    hipLaunchKernelGGL(k_saver_row_verdict, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s, miss, rows, K, chunks, extra, invert ? 1 : 0, status);
}
}  // namespace saverk
