// crypto_amd/csrc/serde_launch.hip.h — host-callable launchers of the point decoding / validation kernels (serde_kernels.hip.h, built in
// k_serde.hip); the driver (dock_serde_dev.hip) only sees these declarations.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace serde {
// points [lo, hi) of raw (records of 48 / 96 / 192 bytes, 4-byte aligned) -> xy (ABI words, 12 / 24 u64 per point) + is_inf for accepted points;
// *first_bad := min(*first_bad, i) for every refused i.  nfp: 1 = G1, 2 = G2.
void launch_deserialize(hipStream_t s, int nfp, bool compressed, bool validate, const uint32_t *raw, size_t lo, size_t hi, uint32_t *xy, uint8_t *is_inf, uint32_t *first_bad);
// ok[i] for the affine ABI words of points [lo, hi) (is_inf may be null)
void launch_validate_words(hipStream_t s, int nfp, const uint32_t *xy, const uint8_t *is_inf, size_t lo, size_t hi, uint8_t *ok);
}  // namespace serde
