// crypto_amd/csrc/selftest_gt_kernels.hip.h — the six-lane GT group arithmetic one function at a time (development twin only: k_selftest.hip).
//
// The wrappers follow selftest_kernels.hip.h (its StOp<ID>, its ST_* numbers): each calls ONE function of gt_kernels.hip.h, included unchanged.  Their
// bodies are templates over the lane type X: k_selftest_gt<ID> instantiates them with GtLanesDev behind GT_GROUP_PROLOGUE — the body shape of k_final_exp,
// k_gt_in_subgroup and k_gt_fold: G groups per 64-lane wave, slots at sh + g GT_SLOTS GT_LANES, the lanes past 6 G and the groups past n leaving early —
// and tests/native/gt_dev_host_shim.cpp instantiates them with its HostLanes (six threads) under the FP29_CHECK bound tracker (shim_selftest_gt).
// For these ops `stress` = reps | G << 8: reps = how often the output is fed back (the value bounds must close), G = groups per wave (1, 3 or 10).
//
// Rows (u64 words): an element in the ABI form is 72 words, lane e loading and storing coefficient e through gt_get_abi / gt_put_abi; an element as RAW
// limbs (what k_miller_tail loads from `partial`) is 6 x 14 words, coefficient q (tower order) at word 14 q: the 14 u32 limbs of c0, then those of c1.
#pragma once
#include "selftest_kernels.hip.h"
#if defined(__HIPCC__)
#include "gt_lanes.hip.h"
#else
#include "gt_kernels.hip.h"
#endif

namespace selftest {

constexpr int ST_GT_RAW = GT_LANES * NL;         // u64 words of an element as raw limbs (= those of the internal form, GT_ELW / 2)
constexpr int ST_GT_SHRUNK = 26;                 // u64 words a lane of ST_GT_SHRINK stores: 28 raw limbs, 12 canonical words

// six lanes per row, IN / OUT u64 words per row; the body sees the group as x
#define ST_GT_OP(ID, IN, OUT) \
    template <> struct StOp<ID> { static constexpr int LANES = GT_LANES, IN64 = IN, OUT64 = OUT; static constexpr bool HOST = true; \
                                  template <class X> static FD void run(X &x, const uint32_t *in, uint32_t *out, int reps); }; \
    template <class X> FD void StOp<ID>::run(X &x, const uint32_t *in, uint32_t *out, int reps)

// raw limbs as k_miller_tail loads them: gt_shrink's input contract (limbs 0..12 <= 2^29 + 7, the top limb < 2^16)
FD void st_ld_raw(Fp &r, const uint32_t *w) {
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = w[i];
    CHK(for (int i = 0; i < NL - 1; i++) r.ub[i] = (1ull << LB) + 7; r.ub[NL - 1] = (1ull << 16) - 1; r.vb = 5041.0; chk_actual(r);)
}
FD void st_ld_raw(Fp2 &r, const uint32_t *w) { st_ld_raw(r.c0, w); st_ld_raw(r.c1, w + NL); }

ST_GT_OP(ST_GT_ROUNDTRIP, 72, 72 + ST_GT_RAW) {          // ABI -> internal form (the row's scratch element, words 72..) -> ABI
    (void)reps; const int e = x.lane(); uint32_t *scr = out + GT_ABIW + e * GT_TABW;
    Fp2 a, b; gt_get_abi(a, in, e); gt_put(scr, a); gt_get(b, scr); gt_put_abi(out, e, b);
}
ST_GT_OP(ST_GT_CONJ, 72, 72) { (void)reps; const int e = x.lane(); Fp2 a, r; gt_get_abi(a, in, e); gt_conj(r, a, e); gt_put_abi(out, e, r); }
ST_GT_OP(ST_GT_NEG, 72, 72) { (void)reps; const int e = x.lane(); Fp2 a, r; gt_get_abi(a, in, e); gt_neg(r, a); gt_put_abi(out, e, r); }
ST_GT_OP(ST_GT_MUL, 144, 72) {                           // a b, then b again reps - 1 times
    const int e = x.lane(); Fp2 a, b, r; gt_get_abi(a, in, e); gt_get_abi(b, in + GT_ABIW, e);
    gt_mul(x, r, a, b);
#pragma unroll 1
    for (int i = 1; i < reps; i++) gt_mul(x, r, r, b);
    gt_put_abi(out, e, r);
}
ST_GT_OP(ST_GT_SQR_BY_MUL, 72, 72) { (void)reps; const int e = x.lane(); Fp2 f; gt_get_abi(f, in, e); gt_mul(x, f, f, f); gt_put_abi(out, e, f); }      // the tail's aliased call
ST_GT_OP(ST_GT_CYC_SQR, 72, 72) {                        // cyclotomic inputs only
    const int e = x.lane(); Fp2 r; gt_get_abi(r, in, e);
#pragma unroll 1
    for (int i = 0; i < reps; i++) gt_cyc_sqr(x, r, r);
    gt_put_abi(out, e, r);
}
ST_GT_OP(ST_GT_FROB1, 72, 72) { (void)reps; const int e = x.lane(); Fp2 a, r; gt_get_abi(a, in, e); gt_frob1(r, a, e); gt_put_abi(out, e, r); }
ST_GT_OP(ST_GT_FROB2, 72, 72) { (void)reps; const int e = x.lane(); Fp2 a, r; gt_get_abi(a, in, e); gt_frob2(r, a, e); gt_put_abi(out, e, r); }
ST_GT_OP(ST_GT_INV, 72, 72) { (void)reps; const int e = x.lane(); Fp2 a, r; gt_get_abi(a, in, e); gt_inv(x, r, a); gt_put_abi(out, e, r); }
ST_GT_OP(ST_GT_EXP_BY_X, 72, 72) { (void)reps; const int e = x.lane(); Fp2 a, r; gt_get_abi(a, in, e); gt_exp_by_x(x, r, a); gt_put_abi(out, e, r); }     // cyclotomic inputs only
ST_GT_OP(ST_GT_FINAL_EXP, 72, 73) {                      // as k_final_exp: a zero input gives zero words; word 72 = the zero flag
    (void)reps; const int e = x.lane(); const uint32_t *src = in + gt_tower_of(e) * 24;
    uint32_t any = 0;
    for (int k = 0; k < 24; k++) any |= src[k];
    const bool zero = x.all(any == 0);
    Fp2 f, r; gt_get_abi(f, in, e); gt_final_exp(x, r, f);
    gt_put_abi(out, e, r);
    if (zero) st_zero(out + gt_tower_of(e) * 24, 24);
    if (e == 0) { out[GT_ABIW] = zero ? 1u : 0u; out[GT_ABIW + 1] = 0; }
}
ST_GT_OP(ST_GT_MEMBERSHIP, 72, 1) {                      // bit 0: gt_in_cyclotomic, bit 1: gt_in_gt
    (void)reps; const int e = x.lane(); Fp2 f; gt_get_abi(f, in, e);
    const bool cyc = gt_in_cyclotomic(x, f), gt = gt_in_gt(x, f);
    if (e == 0) { out[0] = (cyc ? 1u : 0u) | (gt ? 2u : 0u); out[1] = 0; }
}
ST_GT_OP(ST_GT_SHRINK, ST_GT_RAW, GT_LANES * ST_GT_SHRUNK) {    // lane e shrinks the row's e-th input: its 28 raw limbs out, then its canonical words
    (void)reps; const int e = x.lane(); uint32_t *o = out + e * 2 * ST_GT_SHRUNK;
    Fp2 a, r; st_ld_raw(a, in + e * GT_TABW); gt_shrink(r, a);
    for (int i = 0; i < NL; i++) { o[i] = r.c0.l[i]; o[NL + i] = r.c1.l[i]; }
    st_st(o + GT_TABW, r);
}
ST_GT_OP(ST_GT_TAIL_STEP, 2 * ST_GT_RAW, 72) {           // k_miller_tail's load path and step: f, l raw, both shrunk; f = f f, f = f l, reps times
    const int e = x.lane(), q = gt_tower_of(e);
    Fp2 f, l; st_ld_raw(f, in + q * GT_TABW); gt_shrink(f, f); st_ld_raw(l, in + GT_ELW + q * GT_TABW); gt_shrink(l, l);
#pragma unroll 1
    for (int i = 0; i < reps; i++) { gt_mul(x, f, f, f); gt_mul(x, f, f, l); }
    gt_put_abi(out, e, f);
}
// one lane per row: the 65 signed digits of a 256-bit exponent, a byte each
ST_OP(ST_GT_DIGITS, 1, 4, 9) {
    (void)stress; uint32_t ex[8]; int8_t d[65];
    for (int i = 0; i < 8; i++) ex[i] = in[i];
    gt_signed_digits(ex, d);
    st_zero(out, 18);
    for (int w = 0; w <= 64; w++) out[w >> 2] |= (uint32_t)(uint8_t)d[w] << (8 * (w & 3));
}

#if defined(__HIPCC__)
// one instantiation per op, launched as the shipping GT kernels are: a wave per block, (n + G - 1) / G blocks
template <int OP> __global__ void __launch_bounds__(64) k_selftest_gt(const uint32_t *__restrict__ in, size_t n, int G, uint32_t *__restrict__ out, int reps) {
    using O = StOp<OP>;
    GT_GROUP_PROLOGUE
    (void)q;
    O::run(x, in + i * (size_t)(2 * O::IN64), out + i * (size_t)(2 * O::OUT64), reps);
}
#endif

}  // namespace selftest
