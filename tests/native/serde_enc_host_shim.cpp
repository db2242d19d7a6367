// tests/native/serde_enc_host_shim.cpp — host build (g++) of the DEVICE point encoding routines (crypto_amd/csrc/serde_kernels.hip.h: encode_point,
// record_to_abi) with the FP29_CHECK worst-case bound tracker.  Test-only: tests/test_serde_encode_device_code_on_host.py compares their bytes with
// dgpu_g1_serialize / dgpu_g2_serialize without a GPU; an assertion that fires inside means a lazy-limb overflow is possible for some input.
#define FP29_CHECK 1
#include "../../crypto_amd/csrc/serde_kernels.hip.h"
#include <string.h>
using namespace serde;

namespace {
// a base record as k_prep_bases writes it (msm_kernels.hip.h store_coords_from_abi for G1S / G2S): fs_from_abi of every component, the flag word
template <class F> void make_record(const uint32_t *w, bool inf, uint32_t *rec) {
    constexpr int K = Curve<F>::NFP;
    memset(rec, 0, Rec<F>::WORDS * 4);
    for (int j = 0; j < 2 * K; j++) {
        Fs f; fs_from_abi(f, w + 12 * j);
        for (int i = 0; i < SN; i++) rec[j * Rec<F>::SLOT + i] = (uint32_t)f.l[i];
    }
    uint32_t any = 0;
    for (int k = 0; k < 24 * K; k++) any |= w[k];
    rec[Rec<F>::FLAGW] = (inf || any == 0) ? 1u : 0u;
}
template <class F> void encode_one(const uint32_t *w, bool inf, int compressed, uint32_t *rec) {
    if (compressed) encode_point<F, true>(w, inf, rec); else encode_point<F, false>(w, inf, rec);
}
}  // namespace

extern "C" {
// n points of ABI words (12 / 24 u64 each; is_inf may be null) -> the bytes of dgpu_g*_serialize (48 / 96 NFP bytes per point)
void shim_encode(int nfp, const uint64_t *xy, const uint8_t *is_inf, size_t n, int compressed, uint8_t *out) {
    const size_t sz = (compressed ? 48 : 96) * nfp;
    for (size_t i = 0; i < n; i++) {
        uint32_t w[48], rec[48]; memcpy(w, xy + i * 12 * nfp, 96 * nfp);
        const bool inf = is_inf && is_inf[i];
        if (nfp == 1) encode_one<Fp>(w, inf, compressed, rec); else encode_one<Fp2>(w, inf, compressed, rec);
        memcpy(out + i * sz, rec, sz);
    }
}
// the same points through a base record: the words and flags record_to_abi reads back, and (out != null) the bytes of k_read_records
void shim_record(int nfp, const uint64_t *xy, const uint8_t *is_inf, size_t n, int compressed, uint64_t *xy_back, uint8_t *inf_back, uint8_t *out) {
    const size_t sz = (compressed ? 48 : 96) * nfp;
    for (size_t i = 0; i < n; i++) {
        uint32_t w[48], rec[64], back[48], enc[48]; uint8_t inf = 0;
        memcpy(w, xy + i * 12 * nfp, 96 * nfp);
        const bool fl = is_inf && is_inf[i];
        if (nfp == 1) { make_record<Fp>(w, fl, rec); record_to_abi<Fp>(rec, back, &inf); }
        else { make_record<Fp2>(w, fl, rec); record_to_abi<Fp2>(rec, back, &inf); }
        memcpy(xy_back + i * 12 * nfp, back, 96 * nfp); inf_back[i] = inf;
        if (out) {
            if (nfp == 1) encode_one<Fp>(back, inf != 0, compressed, enc); else encode_one<Fp2>(back, inf != 0, compressed, enc);
            memcpy(out + i * sz, enc, sz);
        }
    }
}
}
