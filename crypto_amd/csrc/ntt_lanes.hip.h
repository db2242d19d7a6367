// crypto_amd/csrc/ntt_lanes.hip.h — what ONE lane does in the NTT / witness-map kernels: element loads, the sparse row of k_csr_eval, the radix-2
// butterfly, the radix-4 unit (two stages on four elements) and the (a b - c) / Z step.  __host__ __device__ and free of HIP builtins, so the pass
// kernels of ntt_kernels.hip.h (one pass over an array in HBM) and the block kernel of wm_block_kernels.hip.h (a whole witness map inside one
// block's LDS) run the SAME bodies, and tests/native/wm_block_host_shim.cpp runs them on the host under -DFP29_CHECK.
#pragma once
#include <stddef.h>
#include "fr29.hip.h"

namespace ntt {
using namespace fr29;

constexpr int PIPE_TILE_LOG = 10;      // 1024 elements = 40 KB of LDS, 256 lanes (one radix-4 unit each), four blocks per CU

FRD void ld(Fr &r, const uint32_t *__restrict__ buf, size_t D, size_t i) {
#pragma unroll
    for (int l = 0; l < NL; l++) r.l[l] = buf[(size_t)l * D + i];
}
FRD void st(uint32_t *__restrict__ buf, size_t D, size_t i, const Fr &a) {
#pragma unroll
    for (int l = 0; l < NL; l++) buf[(size_t)l * D + i] = a.l[l];
}
FRD uint32_t bitrev(uint32_t x, int logn) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x) >> (32 - logn);
#else
    uint32_t r = 0;
    for (int b = 0; b < logn; b++) r |= ((x >> b) & 1u) << (logn - 1 - b);
    return r;
#endif
}
// Per-stage twiddle tables.  A stage whose twiddle exponents are j << sigma reads T_sigma[j] = w^(j << sigma), H >> sigma entries stored
// contiguously (limb-major, stride H >> sigma) behind the full table T_0: consecutive butterflies read consecutive words.  Indexing T_0
// with the stride 2^sigma made every lane of a wave touch its own cache line (0.6 of the 2.4 ms of the seven transforms at D = 2^20).
// Word offset of T_sigma inside the buffer: NL * (2H - 2 (H >> sigma)); the whole buffer holds < 2H elements.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline size_t tw_stage_offset(size_t H, int sigma) { return (size_t)NL * (2 * H - 2 * (H >> sigma)); }
// one scalar of the caller's words (8 x u32 = 32 contiguous bytes: one cache line per gather), converted on the fly
FRD void ld_words(Fr &r, const uint32_t *__restrict__ words, size_t i, bool mont) {
    uint32_t w[8];
#if defined(__HIPCC__)
    const uint4 *p = reinterpret_cast<const uint4 *>(words + i * 8);
    uint4 a = p[0], b = p[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
#else
    for (int k = 0; k < 8; k++) w[k] = words[i * 8 + k];
#endif
    fr_from_words(r, w, mont);
}
FRD void st_words(uint32_t *__restrict__ words, size_t i, const uint32_t w[8]) {
#if defined(__HIPCC__)
    uint4 *q = reinterpret_cast<uint4 *>(words + i * 8);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]); q[1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
    for (int k = 0; k < 8; k++) words[i * 8 + k] = w[k];
#endif
}
// element i of a sparse matrix times z, padded to the domain: sum_k vals[k] * z[cols[k]] over row i (i < rows); z[i - rows] for the next `extra`
// elements (matrix A only: a_{m+j} = z_j); zero beyond.
FRD void csr_row(Fr &acc, const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ cols, const uint32_t *__restrict__ vals_soa, size_t nnz,
                 const uint32_t *__restrict__ z_words, bool z_mont, size_t rows, size_t extra, size_t i) {
    fr_zero(acc);
    if (i < rows) {
        for (uint64_t k = rowptr[i]; k < rowptr[i + 1]; k++) {
            Fr c, zz, t; ld(c, vals_soa, nnz, k); ld_words(zz, z_words, cols[k], z_mont);
            fr_mul(t, zz, c); fr_add(acc, acc, t); fr_norm(acc, acc);
        }
        // a long row leaves a sum of (row length) products of < 2 r each: one product with the Montgomery one brings it back under 2 r, so
        // that what the inverse transform accumulates is bounded by the domain size alone (fr_sub's M = 2^34 case)
        if (rowptr[i + 1] - rowptr[i] > 8) { Fr one; fr_one(one); fr_mul(acc, acc, one); }
    } else if (i < rows + extra) ld_words(acc, z_words, i - rows, z_mont);
}
template <bool DIF> FRD void butterfly(Fr &x, Fr &y, const Fr &w) {
    Fr u, v;
    if (DIF) {
        fr_add(u, x, y); fr_norm(u, u);
        fr_sub<FR_BIG>(v, x, y); fr_norm(v, v); fr_mul(v, v, w);     // y: an unreduced partial sum (up to 2^32 r)
    } else {
        Fr yw; fr_mul(yw, y, w);
        fr_add(u, x, yw); fr_norm(u, u);
        fr_sub(v, x, yw); fr_norm(v, v);
    }
    x = u; y = v;
}
// The radix-4 unit: two stages on four elements, no carry pass in between (limbs are 29 bits in 32-bit words, a sum of two normalised values or a
// difference formed with the 2^30-limbed multiple of r stays below 2^31 and may enter a product or one more addition as it is).
//   DIF pair of stages, distances ha = 2^(S-1-st), hb = ha / 2:      m00, m01 = m00 + hb, m10 = m00 + ha, m11
//        A: (m00, m10) twiddle jm, (m01, m11) twiddle jm + hb;  B: (m00, m01) and (m10, m11) share one twiddle
FRD void r4_dif(Fr &x00, Fr &x01, Fr &x10, Fr &x11, const Fr &wa0, const Fr &wa1, const Fr &wb) {
    Fr t;
    // A
    fr_sub<FR_BIG>(t, x00, x10); fr_add(x00, x00, x10); fr_norm(t, t); fr_mul(x10, t, wa0);
    fr_sub<FR_BIG>(t, x01, x11); fr_add(x01, x01, x11); fr_norm(t, t); fr_mul(x11, t, wa1);
    // B (x00, x01 carry limbs < 2^30 + 16: dominated by the subtraction constant, and their sum fits a word)
    fr_sub<FR_BIG>(t, x00, x01); fr_add(x00, x00, x01); fr_norm(x00, x00); fr_norm(t, t); fr_mul(x01, t, wb);
    fr_sub<FR_BIG>(t, x10, x11); fr_add(x10, x10, x11); fr_norm(x10, x10); fr_norm(t, t); fr_mul(x11, t, wb);
}
//   DIT pair of stages (st, st+1), distances ha = 2^st, hb = 2 ha:   m00, m01 = m00 + ha, m10 = m00 + hb, m11
//        A: (m00, m01) and (m10, m11) share one twiddle;  B: (m00, m10) twiddle jm, (m01, m11) twiddle jm + ha
FRD void r4_dit(Fr &x00, Fr &x01, Fr &x10, Fr &x11, const Fr &wa, const Fr &wb0, const Fr &wb1) {
    Fr t;
    // A: no carry pass; sums < 2^30 + 16, differences < 2^31 per limb
    fr_mul(t, x01, wa); fr_sub<512, 30>(x01, x00, t); fr_add(x00, x00, t);
    fr_mul(t, x11, wa); fr_sub<512, 30>(x11, x10, t); fr_add(x10, x10, t);
    // B
    fr_mul(t, x10, wb0); fr_sub<512, 30>(x10, x00, t); fr_add(x00, x00, t); fr_norm(x00, x00); fr_norm(x10, x10);
    fr_mul(t, x11, wb1); fr_sub<512, 30>(x11, x01, t); fr_add(x01, x01, t); fr_norm(x01, x01); fr_norm(x11, x11);
}
// t = (x y - z) * zinv; z is an un-reduced transform output
FRD void pointwise_lane(Fr &t, const Fr &x, const Fr &y, const Fr &z, const Fr &zi) {
    fr_mul(t, x, y); fr_sub<FR_BIG>(t, t, z); fr_norm(t, t); fr_mul(t, t, zi);
}

}  // namespace ntt
