// crypto_amd/csrc/selftest_launch.hip.h — host-callable launchers of the device self-tests (k_selftest.hip; development twin only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace selftest {
void launch_selftest_fp_mul(hipStream_t s, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out);
void launch_selftest_g1_sum(hipStream_t s, const uint32_t *pts, const uint8_t *neg, size_t n, uint32_t *out, uint8_t *out_inf);
// the row shape of op (u64 words in / out per row) for this stress; false: no such op, or a stress the op does not take
bool selftest_arith_shape(int op, int stress, size_t *in_words, size_t *out_words);
// n rows of the shape above through op's kernel (selftest_kernels.hip.h); false: no such op
bool launch_selftest_arith(hipStream_t s, int op, int stress, const uint32_t *in, size_t n, uint32_t *out);
}  // namespace selftest
