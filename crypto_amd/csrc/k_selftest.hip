// crypto_amd/csrc/k_selftest.hip — translation unit of the device self-tests: linked into the development twin only (libdock_gpu_dev.so).
// One kernel per op is some sixty kernels of fully inlined field code, so the Makefile compiles this file twelve times, -DST_PART=k instantiating
// the k-th share of the ops (k_selftest.o is part 0, which also holds the dispatch; k_selftest_p<k>.o the others): the parts build side by side.
// Parts 8 and up hold the six-lane GT ops (selftest_gt_kernels.hip.h), launched as the shipping GT kernels are, with G groups per wave.
#ifndef ST_PART
#define ST_PART 0
#endif
#include "selftest_gt_kernels.hip.h"
#include "selftest_launch.hip.h"

#define ST_OPS_0(X) X(ST_FP_ROUNDTRIP) X(ST_FP_MUL) X(ST_FP_SQR) X(ST_FP_MUL2) X(ST_FP_MUL_SUB) X(ST_FP_MUL12) X(ST_FP_CANON) X(ST_FP_ISZERO) X(ST_FP_INV) X(ST_FP_SUBMUL)
#define ST_OPS_1(X) X(ST_FS_ROUNDTRIP) X(ST_FS_MUL) X(ST_FS_SQR) X(ST_FS_MUL2) X(ST_FS_MUL_SUB) X(ST_FS_NEG) X(ST_FS_BAL) X(ST_FS_BAL_WIDE) X(ST_FS_ISZERO) X(ST_FS_VIA_FP) X(ST_FS_SUBMUL) \
    X(ST_FP2_MUL) X(ST_FP2_SQR) X(ST_FS2_MUL) X(ST_FS2_SQR) X(ST_FP2_INV) X(ST_FR_ROUNDTRIP) X(ST_FR_MUL) X(ST_FR_BUTTERFLIES) X(ST_FR_CANON) X(ST_FR_INV)
#define ST_OPS_2(X) X(ST_FP2H_MUL) X(ST_FP2H_SQR) X(ST_FP2H_MUL_SUB) X(ST_FP2H_SQR_M) X(ST_FP2H_MUL_XI_N) X(ST_FP2H_INV) X(ST_FS2H_MUL) X(ST_FS2H_MUL_TWO) X(ST_FS2H_SQR) X(ST_FS2H_MUL_SUB)
#define ST_OPS_3(X) X(ST_G1_MADD) X(ST_G1_TREE) X(ST_G1_DBL) X(ST_G1S_MADD) X(ST_G1S_TREE) X(ST_G1S_DBL) X(ST_G1S_TREE_ROUNDS) X(ST_G1S_DBL_ROUNDS)
#define ST_OPS_4(X) X(ST_G2H_TO_AFFINE) X(ST_LINE_DBL) X(ST_LINE_ADD) X(ST_GT_DIGITS)
#define ST_OPS_5(X) X(ST_F12_MUL_BY_014)
#define ST_OPS_6(X) X(ST_G1_MADD_2L) X(ST_G1_DBL_2L) X(ST_G2_MADD_4L) X(ST_G2_DBL_4L) X(ST_G1_PHI) X(ST_G1_TO_AFFINE)
#define ST_OPS_7(X) X(ST_F12_MUL) X(ST_F12_MUL_ROLES)
#define ST_OPS_8(X) X(ST_GT_ROUNDTRIP) X(ST_GT_CONJ) X(ST_GT_NEG) X(ST_GT_MUL) X(ST_GT_SQR_BY_MUL) X(ST_GT_CYC_SQR) X(ST_GT_FROB1) X(ST_GT_FROB2) X(ST_GT_SHRINK) X(ST_GT_TAIL_STEP)
#define ST_OPS_9(X) X(ST_GT_INV) X(ST_GT_EXP_BY_X)
#define ST_OPS_10(X) X(ST_GT_FINAL_EXP)
#define ST_OPS_11(X) X(ST_GT_MEMBERSHIP)
#define ST_CAT_(a, b) a##b
#define ST_CAT(a, b) ST_CAT_(a, b)
#define ST_PART_OPS ST_CAT(ST_OPS_, ST_PART)

namespace selftest {
// this part's ops; false: not one of them
bool ST_CAT(launch_selftest_part, ST_PART)(hipStream_t s, int op, int stress, const uint32_t *in, size_t n, uint32_t *out) {
#if ST_PART >= 8
    const int reps = stress & 0xff, G = stress >> 8;       // (selftest_arith_shape has let through G = 1, 3 and 10 only)
    if (G < 1 || G > bls29::GT_MAX_GROUPS) return false;
#endif
    switch (op) {
#if ST_PART >= 8
#define X(ID) case ID: hipLaunchKernelGGL((k_selftest_gt<ID>), dim3((unsigned)((n + G - 1) / G)), dim3(64), 0, s, in, n, G, out, reps); return true;
#else
#define X(ID) case ID: hipLaunchKernelGGL((k_selftest_arith<ID>), dim3((unsigned)((n * StOp<ID>::LANES + 63) / 64)), dim3(64), 0, s, in, n, out, stress); return true;
#endif
        ST_PART_OPS(X)
#undef X
        default: return false;
    }
}

#if ST_PART == 0
#define ST_DECL(k) bool launch_selftest_part##k(hipStream_t s, int op, int stress, const uint32_t *in, size_t n, uint32_t *out);
ST_DECL(1) ST_DECL(2) ST_DECL(3) ST_DECL(4) ST_DECL(5) ST_DECL(6) ST_DECL(7) ST_DECL(8) ST_DECL(9) ST_DECL(10) ST_DECL(11)
#undef ST_DECL

void launch_selftest_fp_mul(hipStream_t s, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out) {
    hipLaunchKernelGGL(k_selftest_fp_mul, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, a, b, n, out);
}
void launch_selftest_g1_sum(hipStream_t s, const uint32_t *pts, const uint8_t *neg, size_t n, uint32_t *out, uint8_t *out_inf) {
    hipLaunchKernelGGL(k_selftest_g1_sum, dim3(1), dim3(64), 0, s, pts, neg, n, out, out_inf);
}
// the six-lane GT ops take stress = reps | G << 8 with G = 1, 3 or 10 groups per wave; every other op a plain count
static bool stress_ok(int lanes, int stress) {
    if (lanes != bls29::GT_LANES) return stress >= 0 && stress <= 64;
    const int G = stress >> 8;
    return stress >= 0 && (stress & 0xff) <= 64 && (G == 1 || G == 3 || G == 10);
}
bool selftest_arith_shape(int op, int stress, size_t *in_words, size_t *out_words) {
    switch (op) {
#define X(ID) case ID: if (!stress_ok(StOp<ID>::LANES, stress)) return false; *in_words = StOp<ID>::IN64; *out_words = StOp<ID>::OUT64; return true;
        ST_OPS_0(X) ST_OPS_1(X) ST_OPS_2(X) ST_OPS_3(X) ST_OPS_4(X) ST_OPS_5(X) ST_OPS_6(X) ST_OPS_7(X) ST_OPS_8(X) ST_OPS_9(X) ST_OPS_10(X) ST_OPS_11(X)
#undef X
        case ST_FR_BATCH_INV:
            if (stress < 1 || stress > ST_MAX_SHARE) return false;
            *in_words = *out_words = 4 * (size_t)stress; return true;
        default: return false;
    }
}
bool launch_selftest_arith(hipStream_t s, int op, int stress, const uint32_t *in, size_t n, uint32_t *out) {
    if (op == ST_FR_BATCH_INV) { hipLaunchKernelGGL(k_selftest_fr_batch_inv, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, in, n, out, stress); return true; }
    return launch_selftest_part0(s, op, stress, in, n, out) || launch_selftest_part1(s, op, stress, in, n, out) || launch_selftest_part2(s, op, stress, in, n, out)
        || launch_selftest_part3(s, op, stress, in, n, out) || launch_selftest_part4(s, op, stress, in, n, out) || launch_selftest_part5(s, op, stress, in, n, out)
        || launch_selftest_part6(s, op, stress, in, n, out) || launch_selftest_part7(s, op, stress, in, n, out) || launch_selftest_part8(s, op, stress, in, n, out)
        || launch_selftest_part9(s, op, stress, in, n, out) || launch_selftest_part10(s, op, stress, in, n, out) || launch_selftest_part11(s, op, stress, in, n, out);
}
#endif
}  // namespace selftest
