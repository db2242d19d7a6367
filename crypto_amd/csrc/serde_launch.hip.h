// crypto_amd/csrc/serde_launch.hip.h — host-callable launchers of the point decoding / validation / encoding kernels (serde_kernels.hip.h, built in
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
// the ABI words of points [lo, hi) (is_inf may be null) -> their encoded records in out (48 / 96 NFP bytes per point)
void launch_serialize_words(hipStream_t s, int nfp, bool compressed, const uint32_t *xy, const uint8_t *is_inf, size_t lo, size_t hi, uint32_t *out);
// resident base records [lo, hi) of recs (the MSM form: 128 / 256 bytes each) -> enc = 0: ABI words into xy and / or flags into is_inf (either may be
// null); enc = 1 / 2: the compressed / uncompressed encoding into out
void launch_read_records(hipStream_t s, int nfp, int enc, const uint32_t *recs, size_t lo, size_t hi, uint32_t *xy, uint8_t *is_inf, uint32_t *out);
}  // namespace serde
