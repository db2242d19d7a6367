// crypto_amd/csrc/gt_lanes.hip.h — the device side of gt_kernels.hip.h's lane groups, shared by the kernel units k_gt.hip and k_gt_pow.hip:
// a group is six lanes of ONE 64-lane wave (a wave per block), its exchange slots are LDS.
#pragma once
#include "gt_kernels.hip.h"

namespace bls29 {
constexpr int GT_MAX_GROUPS = 10;                 // 60 of a wave's 64 lanes
constexpr size_t GT_MIN_WAVES = 2048;             // two waves per SIMD before a wave takes more than one group

// the group of lanes [base, base + 6) of this wave, its slots in LDS
struct GtLanesDev {
    Fp2 *sh; int e, base;
    __device__ int lane() const { return e; }
    __device__ Fp2 *slot(int j) { return sh + j * GT_LANES; }
    __device__ void sync() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
    __device__ bool all(bool v) { const uint64_t m = __ballot(v); return ((m >> base) & 0x3fu) == 0x3fu; }
    __device__ bool wave_all(bool v) { return __ballot(!v) == 0; }        // over every lane of the wave that is still running
};

// lane layout of a launch with G groups per wave: lane t < 6 G is lane t % 6 of group t / 6
#define GT_GROUP_PROLOGUE                                                                                  \
    __shared__ Fp2 sh[GT_MAX_GROUPS * GT_SLOTS * GT_LANES];                                               \
    const int t = threadIdx.x;                                                                            \
    if (t >= GT_LANES * G) return;                                                                        \
    const int g = t / GT_LANES, e = t % GT_LANES;                                                         \
    const size_t i = (size_t)blockIdx.x * G + g;                                                          \
    if (i >= n) return;                                                                                   \
    GtLanesDev x{sh + g * GT_SLOTS * GT_LANES, e, g * GT_LANES};                                          \
    const int q = gt_tower_of(e);
}  // namespace bls29
