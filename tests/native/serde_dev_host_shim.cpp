// tests/native/serde_dev_host_shim.cpp — host build (g++) of the DEVICE point decoding / validation routines (crypto_amd/csrc/serde_kernels.hip.h)
// with the FP29_CHECK worst-case bound tracker.  Test-only: tests/test_serde_device_code_on_host.py compares them with the big-integer model and the
// host deserialisers without a GPU; an assertion that fires inside means a lazy-limb overflow is possible for some input.
#define FP29_CHECK 1
#include "../../crypto_amd/csrc/serde_kernels.hip.h"
#include <string.h>
using namespace serde;
extern "C" {
// n records of `sz` bytes (sz = 48 / 96 for G1, 96 / 192 for G2); per point ok[i], and for accepted points xy (ABI words) and is_inf
void shim_decode(int nfp, const uint8_t *in, size_t n, int mode, uint64_t *xy, uint8_t *is_inf, uint8_t *ok) {
    const bool comp = mode & 1, validate = !(mode & 2);
    const size_t sz = (comp ? 48 : 96) * nfp;
    for (size_t i = 0; i < n; i++) {
        uint32_t rec[48], out[48]; memcpy(rec, in + i * sz, sz);
        uint8_t inf = 0; bool r;
        if (nfp == 1) r = comp ? decode_point<Fp, true>(rec, validate, out, &inf) : decode_point<Fp, false>(rec, validate, out, &inf);
        else r = comp ? decode_point<Fp2, true>(rec, validate, out, &inf) : decode_point<Fp2, false>(rec, validate, out, &inf);
        ok[i] = r;
        if (r) { memcpy(xy + i * 12 * nfp, out, 96 * nfp); is_inf[i] = inf; }
    }
}
void shim_validate(int nfp, const uint64_t *xy, const uint8_t *is_inf, size_t n, uint8_t *ok) {
    for (size_t i = 0; i < n; i++) {
        uint32_t w[48]; memcpy(w, xy + i * 12 * nfp, 96 * nfp);
        const bool inf = is_inf && is_inf[i];
        ok[i] = nfp == 1 ? words_valid<Fp>(w, inf) : words_valid<Fp2>(w, inf);
    }
}
// Fq / Fq2 square roots alone (ABI words in and out): 1 and the root, or 0
int shim_fq_sqrt(const uint32_t *a, uint32_t *out) { Fp x, y; fp_from_abi(x, a); const bool r = fq_sqrt_dev(y, x); fp_to_abi(out, y); return r; }
int shim_fq2_sqrt(const uint32_t *a, uint32_t *out) { Fp2 x, y; fp_from_abi(x.c0, a); fp_from_abi(x.c1, a + 12); const bool r = fq2_sqrt_dev(y, x); fp_to_abi(out, y.c0); fp_to_abi(out + 12, y.c1); return r; }
}
