// crypto_amd/csrc/setup_launch.hip.h — host-callable launchers of the key-generation kernels (k_setup.hip, setup_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace setupk {
constexpr size_t FOLD_CHUNK = 64;       // entries per lane of a k_fold pass: each pass shrinks the list 32-fold
// u_i (SoA, stride D) from pw = w^i (SoA) and consts = {t, Z(t)/D} (canonical words on the device)
void launch_lagrange(hipStream_t s, const uint32_t *pw, const uint32_t *consts, size_t D, uint32_t *u);
void launch_im_init(hipStream_t s, const uint32_t *u, size_t D, size_t m, size_t num_inputs, size_t nv, uint32_t *a, uint32_t *b, uint32_t *c);
// out (SoA, stride nv) += column sums of u_i * coeff over a resident CSR matrix of `rows` rows and nnz entries (vals: SoA, stride vstride).
// scratch: the transpose (keys + values, nnz entries, then two partial lists), cnt: nv + 1 words (zeroed here).  Size: col_sum_scratch_bytes.
size_t col_sum_scratch_bytes(size_t nnz, size_t nv);
void launch_col_sum(hipStream_t s, const uint64_t *rowptr, size_t rows, const uint32_t *cols, const uint32_t *vals, size_t vstride, size_t nnz,
                    const uint32_t *u, size_t D, uint32_t *out, size_t nv, void *scratch);
void launch_soa_to_words(hipStream_t s, const uint32_t *src, size_t n, int mont, uint32_t *words);
void launch_key_scalars(hipStream_t s, const uint32_t *a, const uint32_t *b, const uint32_t *c, size_t nv, size_t n_abc, const uint32_t *consts,
                        uint32_t *a_w, uint32_t *b_w, uint32_t *abc_w, uint32_t *l_w);
}  // namespace setupk
