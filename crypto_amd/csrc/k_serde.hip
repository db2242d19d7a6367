// crypto_amd/csrc/k_serde.hip — the point decoding / validation / encoding kernels (serde_kernels.hip.h) and their launchers (serde_launch.hip.h)
#include "serde_kernels.hip.h"
#include "serde_launch.hip.h"
#include "msm_kernels.hip.h"

// the record layout serde::record_to_abi reads is the one k_prep_bases writes
static_assert(msm::G1::MSM::AFF_STRIDE == serde::Rec<bls29::Fp>::WORDS && msm::G1::MSM::FLAGW == serde::Rec<bls29::Fp>::FLAGW && msm::G1::MSM::FW == serde::Rec<bls29::Fp>::SLOT, "G1 record layout");
static_assert(msm::G2::MSM::AFF_STRIDE == serde::Rec<bls29::Fp2>::WORDS && msm::G2::MSM::FLAGW == serde::Rec<bls29::Fp2>::FLAGW && msm::PS == serde::Rec<bls29::Fp2>::SLOT, "G2 record layout");

namespace serde {
static dim3 blocks_for(size_t lo, size_t hi) { return dim3((unsigned)((hi - lo + SERDE_BLOCK - 1) / SERDE_BLOCK)); }
void launch_deserialize(hipStream_t s, int nfp, bool compressed, bool validate, const uint32_t *raw, size_t lo, size_t hi, uint32_t *xy, uint8_t *is_inf, uint32_t *first_bad) {
    if (hi <= lo) return;
    const dim3 g = blocks_for(lo, hi), b(SERDE_BLOCK);
    const int v = validate ? 1 : 0;
    if (nfp == 1) {
        if (compressed) hipLaunchKernelGGL((k_deserialize<Fp, true>), g, b, 0, s, raw, lo, hi, v, xy, is_inf, first_bad);
        else hipLaunchKernelGGL((k_deserialize<Fp, false>), g, b, 0, s, raw, lo, hi, v, xy, is_inf, first_bad);
    } else {
        if (compressed) hipLaunchKernelGGL((k_deserialize<Fp2, true>), g, b, 0, s, raw, lo, hi, v, xy, is_inf, first_bad);
        else hipLaunchKernelGGL((k_deserialize<Fp2, false>), g, b, 0, s, raw, lo, hi, v, xy, is_inf, first_bad);
    }
}
void launch_validate_words(hipStream_t s, int nfp, const uint32_t *xy, const uint8_t *is_inf, size_t lo, size_t hi, uint8_t *ok) {
    if (hi <= lo) return;
    if (nfp == 1) hipLaunchKernelGGL((k_validate_words<Fp>), blocks_for(lo, hi), dim3(SERDE_BLOCK), 0, s, xy, is_inf, lo, hi, ok);
    else hipLaunchKernelGGL((k_validate_words<Fp2>), blocks_for(lo, hi), dim3(SERDE_BLOCK), 0, s, xy, is_inf, lo, hi, ok);
}
void launch_serialize_words(hipStream_t s, int nfp, bool compressed, const uint32_t *xy, const uint8_t *is_inf, size_t lo, size_t hi, uint32_t *out) {
    if (hi <= lo) return;
    const dim3 g = blocks_for(lo, hi), b(SERDE_BLOCK);
    if (nfp == 1) {
        if (compressed) hipLaunchKernelGGL((k_serialize_words<Fp, true>), g, b, 0, s, xy, is_inf, lo, hi, out);
        else hipLaunchKernelGGL((k_serialize_words<Fp, false>), g, b, 0, s, xy, is_inf, lo, hi, out);
    } else {
        if (compressed) hipLaunchKernelGGL((k_serialize_words<Fp2, true>), g, b, 0, s, xy, is_inf, lo, hi, out);
        else hipLaunchKernelGGL((k_serialize_words<Fp2, false>), g, b, 0, s, xy, is_inf, lo, hi, out);
    }
}
void launch_read_records(hipStream_t s, int nfp, int enc, const uint32_t *recs, size_t lo, size_t hi, uint32_t *xy, uint8_t *is_inf, uint32_t *out) {
    if (hi <= lo) return;
    const dim3 g = blocks_for(lo, hi), b(SERDE_BLOCK);
    if (nfp == 1) {
        if (enc == 0) hipLaunchKernelGGL((k_read_records<Fp, 0>), g, b, 0, s, recs, lo, hi, xy, is_inf, out);
        else if (enc == 1) hipLaunchKernelGGL((k_read_records<Fp, 1>), g, b, 0, s, recs, lo, hi, xy, is_inf, out);
        else hipLaunchKernelGGL((k_read_records<Fp, 2>), g, b, 0, s, recs, lo, hi, xy, is_inf, out);
    } else {
        if (enc == 0) hipLaunchKernelGGL((k_read_records<Fp2, 0>), g, b, 0, s, recs, lo, hi, xy, is_inf, out);
        else if (enc == 1) hipLaunchKernelGGL((k_read_records<Fp2, 1>), g, b, 0, s, recs, lo, hi, xy, is_inf, out);
        else hipLaunchKernelGGL((k_read_records<Fp2, 2>), g, b, 0, s, recs, lo, hi, xy, is_inf, out);
    }
}
}  // namespace serde
