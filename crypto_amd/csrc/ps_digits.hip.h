// crypto_amd/csrc/ps_digits.hip.h — the signed radix-2^c recoding as the partition sort walks it (psort_kernels.hip.h k_ps_count1 / k_ps_scatter1): one callback per
// window instead of a stored code.  A header of its own, free of wave intrinsics, so that the host can compile it next to digit_codes.hip.h
// (tests/native/digit_codes_host_shim.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sort_launch.hip.h"

namespace msm {
// the W signed digits of scalar i (same recoding as k_digit_codes): f(w, |d| - 1, neg, nonzero) for EVERY window, uniformly over the wave
// (`live` = this lane has a scalar at all).  CC, CW: window width and count known at compile time (the shapes of the per-key tables: every shift
// is a constant and the window loop is unrolled: ~7 instructions per digit instead of ~35 for the word selects of the general form); CC = 0: q.c, q.W.
template <int CC, int CW, class F> __device__ __forceinline__ void ps_digits(const PsParams &q, size_t i, bool live, F f) {
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if (live) { const uint4 *p = reinterpret_cast<const uint4 *>(q.scalars + i * 8); a = p[0]; b = p[1]; }
    uint32_t s[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w & 0x7fffffffu};       // Fr::MODULUS_BIT_SIZE = 255
    uint32_t carry = 0;
    if constexpr (CC != 0) {
        constexpr uint32_t B = 1u << (CC - 1);
#pragma unroll
        for (int w = 0; w < CW; w++) {
            const int bitpos = w * CC;
            uint32_t raw = 0;
            if (bitpos < 256) {
                const int wd = bitpos >> 5, sh = bitpos & 31;
                const uint32_t lo = s[wd], hi = wd + 1 < 8 ? s[wd + 1] : 0u;
                raw = (sh ? ((lo >> sh) | (hi << (32 - sh))) : lo) & ((1u << CC) - 1u);
            }
            const uint32_t v = raw + carry;
            const uint32_t neg = v > B ? 1u : 0u;
            const uint32_t mag = neg ? (2u * B - v) : v;
            carry = neg;
            f(w, mag - 1, neg, live && mag != 0);
        }
    } else {
        const uint32_t B = 1u << (q.c - 1);
        for (int w = 0; w < q.W; w++) {
            const int bitpos = w * q.c;
            uint32_t raw = 0;
            if (bitpos < 256) {
                const int wd = bitpos >> 5, sh = bitpos & 31;
                uint64_t v = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) { if (k == wd) v |= s[k]; if (k == wd + 1) v |= (uint64_t)s[k] << 32; }
                raw = (uint32_t)(v >> sh) & ((1u << q.c) - 1u);
            }
            const uint32_t v = raw + carry;
            const uint32_t neg = v > B ? 1u : 0u;
            const uint32_t mag = neg ? (2u * B - v) : v;
            carry = neg;
            f(w, mag - 1, neg, live && mag != 0);
        }
    }
}
}  // namespace msm
