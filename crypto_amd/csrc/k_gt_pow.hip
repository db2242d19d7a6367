// crypto_amd/csrc/k_gt_pow.hip — GT powers, products of powers and membership tests over many elements: one element (or k bases) per group of
// six lanes, G groups per 64-lane wave, a wave per block — the lane functions of gt_kernels.hip.h, the layout of k_gt.hip.
//
// k_gt_pow is ONE kernel with a wave-uniform branch between the windowed cyclotomic path and the generic one (a ballot over the wave, see
// gt_pow_group); the other layout — a lean cyclotomic kernel that flags its waves, a generic one behind it — was not needed: the branch costs no
// registers beyond what the cyclotomic path takes (DESIGN.md §10 has the resource table).
#include "gt_lanes.hip.h"
#include "gt_launch.hip.h"

namespace {
using namespace bls29;

// nb bases, k per group: group i writes prod_j in[i k + j]^(e[i k + j]) to element i of out (ABI form if out_abi, else internal).
// tab: GT_TAB GT_ELW words per base, rounded up to whole groups.
__global__ void __launch_bounds__(64) k_gt_pow(const uint32_t *__restrict__ in, const uint32_t *__restrict__ exps, int ew, size_t nb, int G, int k,
                                               uint32_t *tab, uint32_t *__restrict__ out, int out_abi) {
    __shared__ uint64_t cms[GT_MAX_K * 64];
    const size_t n = (nb + k - 1) / k;
    GT_GROUP_PROLOGUE
    (void)q;
    gt_pow_group(x, in, exps, ew, nb, i * k, k, tab + i * k * GT_TAB * GT_ELW, cms + t, 64, false, out + i * (out_abi ? GT_ABIW : GT_ELW), out_abi != 0);
}

// one level of a product: group i multiplies inputs [8 i, 8 i + 8) of n_in
__global__ void __launch_bounds__(64) k_gt_fold(const uint32_t *__restrict__ in, int in_abi, size_t n_in, int G, uint32_t *__restrict__ out, int out_abi) {
    const size_t n = (n_in + GT_FOLD - 1) / GT_FOLD;
    GT_GROUP_PROLOGUE
    (void)q;
    gt_fold_group(x, in, in_abi != 0, n_in, i * GT_FOLD, out + i * (out_abi ? GT_ABIW : GT_ELW), out_abi != 0);
}

__global__ void __launch_bounds__(64) k_gt_in_subgroup(const uint32_t *__restrict__ in, size_t n, int G, uint8_t *__restrict__ ok) {
    GT_GROUP_PROLOGUE
    (void)q;
    Fp2 f; gt_get_abi(f, in + i * GT_ABIW, e);
    const bool v = gt_in_gt(x, f);
    if (e == 0) ok[i] = v ? 1 : 0;
}
}  // namespace

namespace gtk {
static dim3 blocks(size_t n, int G) { return dim3((unsigned)((n + G - 1) / G)); }
static int groups(size_t n, int G) { return (G >= 1 && G <= GT_MAX_GROUPS) ? G : groups_per_wave(n); }
// PROVISIONAL (no sweep has run yet): bases per group of a product of powers: one while the bases alone fill the chip with GT_MIN_WAVES waves,
// then as many as still leave that many groups, up to GT_MAX_K (the four squarings of a window are shared by a group's bases)
int bases_per_group(size_t n) {
    const size_t k = n / GT_MIN_WAVES;
    return (int)(k < 1 ? 1 : (k > (size_t)GT_MAX_K ? GT_MAX_K : k));
}
size_t pow_table_words(size_t n) { return (n + GT_MAX_K) * GT_TAB * GT_ELW; }
void launch_gt_pow(hipStream_t s, const uint32_t *in, const uint32_t *exps, int exp_words, size_t n, int G, int k, uint32_t *tab, uint32_t *out, bool out_abi) {
    if (!n) return;
    if (k < 1 || k > GT_MAX_K) k = 1;
    const size_t ng = (n + k - 1) / k;
    G = groups(ng, G);
    hipLaunchKernelGGL(k_gt_pow, blocks(ng, G), dim3(64), 0, s, in, exps, exp_words, n, G, k, tab, out, out_abi ? 1 : 0);
}
size_t launch_gt_fold(hipStream_t s, const uint32_t *in, bool in_abi, size_t n_in, int G, uint32_t *out, bool out_abi) {
    if (!n_in) return 0;
    const size_t ng = (n_in + GT_FOLD - 1) / GT_FOLD;
    G = groups(ng, G);
    hipLaunchKernelGGL(k_gt_fold, blocks(ng, G), dim3(64), 0, s, in, in_abi ? 1 : 0, n_in, G, out, out_abi ? 1 : 0);
    return ng;
}
void launch_gt_in_subgroup(hipStream_t s, const uint32_t *in, size_t n, int G, uint8_t *ok) {
    if (!n) return;
    G = groups(n, G);
    hipLaunchKernelGGL(k_gt_in_subgroup, blocks(n, G), dim3(64), 0, s, in, n, G, ok);
}
}  // namespace gtk
