// crypto_amd/csrc/k_gt.hip — the batched GT kernels: Miller-loop tails and final exponentiations, one element per group of six lanes
// (gt_kernels.hip.h), a 64-lane wave per block.  Groups exchange coefficients through LDS inside their wave only.
#include "gt_lanes.hip.h"
#include "gt_launch.hip.h"

namespace {
using namespace bls29;
constexpr int F12W = 12 * NL;

__global__ void __launch_bounds__(64) k_miller_tail(const uint32_t *__restrict__ partial, size_t n, int G, uint32_t *__restrict__ out) {
    GT_GROUP_PROLOGUE
    auto load = [&](int s, Fp2 &v) {
        const uint32_t *src = partial + ((size_t)s * n + i) * F12W + 2 * q * NL;
#pragma unroll
        for (int k = 0; k < NL; k++) { v.c0.l[k] = src[k]; v.c1.l[k] = src[NL + k]; }
        gt_shrink(v, v);                                                  // (the sparse products leave values up to 200 p)
    };
    Fp2 f; gt_miller_tail(x, f, load);
    uint32_t *dst = out + i * 144 + q * 24;
    fp_to_abi(dst, f.c0); fp_to_abi(dst + 12, f.c1);
}

__global__ void __launch_bounds__(64) k_final_exp(const uint32_t *__restrict__ in, size_t n, int G, uint32_t *__restrict__ out, uint8_t *__restrict__ is_zero,
                                                  const uint32_t *__restrict__ want, uint8_t *__restrict__ ok) {
    GT_GROUP_PROLOGUE
    const uint32_t *src = in + i * 144 + q * 24;
    uint32_t w[24], any = 0;
#pragma unroll
    for (int k = 0; k < 24; k++) { w[k] = src[k]; any |= w[k]; }
    const bool zero = x.all(any == 0);                                    // arkworks: None (hostf::final_exponentiation: all words zero)
    Fp2 f, r; fp_from_abi(f.c0, w); fp_from_abi(f.c1, w + 12);
    gt_final_exp(x, r, f);
    fp_to_abi(w, r.c0); fp_to_abi(w + 12, r.c1);
    if (zero) for (int k = 0; k < 24; k++) w[k] = 0;
    if (out) { uint32_t *dst = out + i * 144 + q * 24; for (int k = 0; k < 24; k++) dst[k] = w[k]; }
    if (is_zero && e == 0) is_zero[i] = zero ? 1 : 0;
    if (want) {
        uint32_t diff = 0;
        for (int k = 0; k < 24; k++) diff |= w[k] ^ want[q * 24 + k];
        const bool eq = x.all(diff == 0);
        if (e == 0) ok[i] = (eq && !zero) ? 1 : 0;
    }
}
}  // namespace

namespace gtk {
int groups_per_wave(size_t n) {
    size_t g = n / GT_MIN_WAVES;
    return (int)(g < 1 ? 1 : (g > (size_t)GT_MAX_GROUPS ? GT_MAX_GROUPS : g));
}
static dim3 blocks(size_t n, int G) { return dim3((unsigned)((n + G - 1) / G)); }
void launch_miller_tail(hipStream_t s, const uint32_t *partial, size_t m, uint32_t *out_f12) {
    if (!m) return;
    const int G = groups_per_wave(m);
    hipLaunchKernelGGL(k_miller_tail, blocks(m, G), dim3(64), 0, s, partial, m, G, out_f12);
}
void launch_final_exp(hipStream_t s, const uint32_t *in_f12, size_t n, uint32_t *out_gt, uint8_t *is_zero, const uint32_t *want, uint8_t *ok) {
    if (!n) return;
    const int G = groups_per_wave(n);
    hipLaunchKernelGGL(k_final_exp, blocks(n, G), dim3(64), 0, s, in_f12, n, G, out_gt, is_zero, want, ok);
}
}  // namespace gtk
