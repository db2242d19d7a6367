// tests/native/digit_codes_host_shim.cpp — the three copies of the signed radix-2^c recoding (crypto_amd/csrc/digit_codes.hip.h digit_codes_one with 2-byte and
// 4-byte codes; crypto_amd/csrc/ps_digits.hip.h ps_digits with the width at run time and with the constant shifts of the three fixed shapes) compiled for the
// host as they are, one call per scalar where the kernels run one lane per scalar.  Built by tests/test_digit_codes_device_code_on_host.py with the HIP
// headers on the include path (the vector types and the empty host meanings of __device__ / __forceinline__ come from there); the one device function
// the code names, atomicOr, is the plain read-modify-write below.
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p = old | v; return old; }
#include "../../crypto_amd/csrc/digit_codes.hip.h"
#include "../../crypto_amd/csrc/ps_digits.hip.h"

// k_digit_codes over entries [0, n_pad): entry i < n is scalar i (skip[i]: its base is the identity), the others are padding
template <class CODE>
static void codes(const uint32_t *scalars, size_t n, size_t n_pad, const uint8_t *skip, int c, int W, CODE *dig, uint32_t *bad) {
    for (size_t i = 0; i < n_pad; i++) msm::digit_codes_one<CODE>(scalars, i, n, i >= n || skip[i] != 0, n_pad, c, W, dig, bad);
}

// the digits of scalars [0, n) as the sort's kernels receive them: out[(w * n + i) * 3 + {0, 1, 2}] = |d| - 1, negative, non-zero; calls[i] = windows reported
template <int CC, int CW>
static void walk(const uint32_t *scalars, size_t n, const uint8_t *live, int c, int W, uint32_t *out, uint32_t *calls) {
    msm::PsParams q = {};
    q.scalars = scalars; q.n = n; q.c = c; q.W = W;
    for (size_t i = 0; i < n; i++) {
        uint32_t k = 0;
        msm::ps_digits<CC, CW>(q, i, live[i] != 0, [&](int w, uint32_t m1, uint32_t neg, bool nz) {
            uint32_t *o = out + ((size_t)w * n + i) * 3;
            o[0] = m1; o[1] = neg; o[2] = nz ? 1u : 0u;
            k++;
        });
        calls[i] = k;
    }
}

extern "C" {
void shim_codes16(const uint32_t *scalars, size_t n, size_t n_pad, const uint8_t *skip, int c, int W, uint16_t *dig, uint32_t *bad) { codes<uint16_t>(scalars, n, n_pad, skip, c, W, dig, bad); }
void shim_codes32(const uint32_t *scalars, size_t n, size_t n_pad, const uint8_t *skip, int c, int W, uint32_t *dig, uint32_t *bad) { codes<uint32_t>(scalars, n, n_pad, skip, c, W, dig, bad); }
// shape 0: the width at run time; 20, 17, 16: the fixed shapes <20, 13>, <17, 16>, <16, 16> (c and W are ignored by them).  Returns 0, or -1 for no such shape.
int shim_ps_digits(int shape, const uint32_t *scalars, size_t n, const uint8_t *live, int c, int W, uint32_t *out, uint32_t *calls) {
    if (shape == 0) walk<0, 0>(scalars, n, live, c, W, out, calls);
    else if (shape == 20) walk<20, 13>(scalars, n, live, c, W, out, calls);
    else if (shape == 17) walk<17, 16>(scalars, n, live, c, W, out, calls);
    else if (shape == 16) walk<16, 16>(scalars, n, live, c, W, out, calls);
    else return -1;
    return 0;
}
int shim_ps_part_log(uint32_t NB) { return msm::ps_part_log(NB); }
// the two rules of launch_psort (the write-combining placement, P3's dynamic LDS with the limit it is launched under) and plain_geometry's condition on them
int shim_ps_use_wc(size_t n, int W, uint32_t P) { return msm::ps_use_wc(n, W, P) ? 1 : 0; }
size_t shim_ps_scatter_lds_bytes(uint32_t P, int W) { return msm::ps_scatter_lds_bytes(P, W); }
size_t shim_ps_scatter_lds_max(void) { return msm::PS_SCATTER_LDS_MAX; }
int shim_plain_psort_fits(int W, uint32_t NB) { return msm::plain_psort_fits(W, NB) ? 1 : 0; }
}
