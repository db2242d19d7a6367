// crypto_amd/csrc/selftest_kernels.hip.h — the device arithmetic one operation at a time (development twin only: k_selftest.hip).
//
// Every op is a wrapper StOp<ID> around ONE function of the product headers (fp29 / fp30s / fp2_29 / fs2_pair / fp2_pair / fr29 / fp_safegcd /
// fp_inv / ec29 / ec29_two_lane / pairing29, included unchanged): load a row of ABI words, run the function, store through the op's canonicalising
// store.  k_selftest_arith<ID> is one kernel per op (no switch: the register allocation and inlining around the function under test stay what a
// kernel of its own gets), 64 lanes per block, one row per lane — or per lane pair / quad for the lane-shared forms, so that the two pairs of a
// quad hold different rows and an exchange that crosses the pair shows.
//
// The wrappers that need no lane exchange are host/device functions: tests/native/fp29_host_shim.cpp runs the SAME bodies under the FP29_CHECK bound
// tracker (shim_selftest_arith), which is what decides the operand classes (`stress`) an op may be given.  tests/test_gpu_device_arith.py holds the
// operand tables and the big-integer expectations, and mirrors the ST_* numbers below.
//
// Families: Fp, Fs, Fp2 / Fs2 (one lane and lane pairs), Fr, the group law over all four fields (one lane, two and four lanes), the Fp12 products and the
// one-lane line steps of pairing29.hip.h (ST_LINE_*), and — numbered here, wrapped in selftest_gt_kernels.hip.h — the six-lane GT group arithmetic of
// gt_kernels.hip.h / gt_lanes.hip.h (ST_GT_*: six lanes per row behind GT_GROUP_PROLOGUE, k_selftest_gt<ID>, stress = reps | G << 8).
//
// Row layout (u64 words in the ABI of include/dock_gpu.h; the wrappers see them as u32 pairs):
//   Fp / Fs element: 6 words (value * 2^384 mod p), Fp2 / Fs2: 12 (c0, c1), Fr: 4 (canonical or * 2^256, per op), Fp12: 72
//   chain rows: word 0 = count | sign bits << 32, then ST_MAXP affine points (x, y); point outputs are X, Y, ZZ, ZZZ — all-zero = identity
//   stress = k: an operand is added to itself k - 1 times, un-normalised, before the operation (a lazy-class operand)
#pragma once
#include "fp29.hip.h"
#include "fp2_29.hip.h"
#include "ec29.hip.h"
#include "fp30s.hip.h"
#include "fs2_pair.hip.h"
#include "pairing29.hip.h"
#include "fr29.hip.h"
#include "fp_safegcd.hip.h"
#if defined(__HIPCC__)
#include "fp_inv.hip.h"
#include "ec29_two_lane.hip.h"
#endif

namespace selftest {
using namespace bls29;

constexpr int ST_MAXP = 24;          // points per chain / tree row
constexpr int ST_MAX_SHARE = 16;     // elements per lane of the batched inversion

enum : int {
    // fp29.hip.h
    ST_FP_ROUNDTRIP = 0, ST_FP_MUL, ST_FP_SQR, ST_FP_MUL2, ST_FP_MUL_SUB, ST_FP_MUL12, ST_FP_CANON, ST_FP_ISZERO, ST_FP_INV, ST_FP_SUBMUL,
    // fp30s.hip.h
    ST_FS_ROUNDTRIP = 16, ST_FS_MUL, ST_FS_SQR, ST_FS_MUL2, ST_FS_MUL_SUB, ST_FS_NEG, ST_FS_BAL, ST_FS_BAL_WIDE, ST_FS_ISZERO, ST_FS_VIA_FP, ST_FS_SUBMUL,
    // fp2_29.hip.h / fs2_pair.hip.h, one lane per element
    ST_FP2_MUL = 32, ST_FP2_SQR, ST_FS2_MUL, ST_FS2_SQR, ST_FP2_INV,
    // fp2_pair.hip.h / fs2_pair.hip.h, a lane pair per element
    ST_FP2H_MUL = 40, ST_FP2H_SQR, ST_FP2H_MUL_SUB, ST_FP2H_SQR_M, ST_FP2H_MUL_XI_N, ST_FP2H_INV, ST_FS2H_MUL, ST_FS2H_MUL_TWO, ST_FS2H_SQR, ST_FS2H_MUL_SUB,
    // fr29.hip.h
    ST_FR_ROUNDTRIP = 56, ST_FR_MUL, ST_FR_BUTTERFLIES, ST_FR_CANON, ST_FR_INV, ST_FR_BATCH_INV,
    // ec29.hip.h: mixed-addition chains, addition trees, doubling chains
    ST_G1_MADD = 64, ST_G1_TREE, ST_G1_DBL,
    ST_G1S_MADD = 68, ST_G1S_TREE, ST_G1S_DBL, ST_G1S_TREE_ROUNDS, ST_G1S_DBL_ROUNDS,
    ST_G2_MADD = 74, ST_G2_TREE, ST_G2_DBL,
    ST_G2S_MADD = 78, ST_G2S_MADD_EARLY, ST_G2S_TREE, ST_G2S_DBL, ST_G2S_TREE_ROUNDS, ST_G2S_DBL_ROUNDS,
    // ec29_two_lane.hip.h (two lanes per G1 point, four per G2 point), xyzz_phi, fp_inv.hip.h's xyzz_to_affine
    ST_G1_MADD_2L = 88, ST_G1_DBL_2L, ST_G2_MADD_4L, ST_G2_DBL_4L, ST_G1_PHI, ST_G1_TO_AFFINE, ST_G2H_TO_AFFINE = 95,
    // pairing29.hip.h
    ST_F12_MUL = 100, ST_F12_MUL_ROLES, ST_F12_MUL_BY_014, ST_LINE_DBL = 104, ST_LINE_ADD,
    // gt_kernels.hip.h / gt_lanes.hip.h (the wrappers are in selftest_gt_kernels.hip.h): six lanes per row, but for the digits
    ST_GT_ROUNDTRIP = 110, ST_GT_CONJ, ST_GT_NEG, ST_GT_MUL, ST_GT_SQR_BY_MUL, ST_GT_CYC_SQR, ST_GT_FROB1, ST_GT_FROB2, ST_GT_INV, ST_GT_EXP_BY_X, ST_GT_FINAL_EXP,
    ST_GT_MEMBERSHIP, ST_GT_SHRINK, ST_GT_TAIL_STEP, ST_GT_DIGITS,
    ST_OP_END
};

// ---- loads / stores by field type (u32 words per element: SW<F>::N) ----
template <class F> struct SW;
template <> struct SW<Fp> { static constexpr int N = 12; };
template <> struct SW<Fs> { static constexpr int N = 12; };
template <> struct SW<Fp2> { static constexpr int N = 24; };
template <> struct SW<Fs2> { static constexpr int N = 24; };
FD void st_ld(Fp &r, const uint32_t *w) { fp_from_abi(r, w); }
FD void st_ld(Fs &r, const uint32_t *w) { fs_from_abi(r, w); }
FD void st_ld(Fp2 &r, const uint32_t *w) { fp_from_abi(r.c0, w); fp_from_abi(r.c1, w + 12); }
FD void st_ld(Fs2 &r, const uint32_t *w) { fs_from_abi(r.c0, w); fs_from_abi(r.c1, w + 12); }
FD void st_st(uint32_t *w, const Fp &a) { fp_to_abi(w, a); }
FD void st_st(uint32_t *w, const Fs &a) { fs_to_abi(w, a); }
FD void st_st(uint32_t *w, const Fp2 &a) { fp_to_abi(w, a.c0); fp_to_abi(w + 12, a.c1); }
FD void st_st(uint32_t *w, const Fs2 &a) { fs_to_abi(w, a.c0); fs_to_abi(w + 12, a.c1); }
// k x as k - 1 unreduced additions
template <class F> FD void st_lazy(F &t, const F &x, int k) { t = x; for (int i = 1; i < k; i++) fadd(t, t, x); }
FD void st_zero(uint32_t *w, int n) { for (int i = 0; i < n; i++) w[i] = 0; }

template <int OP> struct StOp;
// LANES lanes per row, IN / OUT u64 words per row; HOST: the body also builds for the host (the bound-tracker run)
#define ST_OP(ID, L, IN, OUT) \
    template <> struct StOp<ID> { static constexpr int LANES = L, IN64 = IN, OUT64 = OUT; static constexpr bool HOST = true; static FD void run(const uint32_t *in, uint32_t *out, int stress); }; \
    FD void StOp<ID>::run(const uint32_t *in, uint32_t *out, int stress)
#define ST_DEV_OP(ID, L, IN, OUT) \
    template <> struct StOp<ID> { static constexpr int LANES = L, IN64 = IN, OUT64 = OUT; static constexpr bool HOST = false; static __device__ __forceinline__ void run(const uint32_t *in, uint32_t *out, int stress); }; \
    __device__ __forceinline__ void StOp<ID>::run(const uint32_t *in, uint32_t *out, int stress)

// ---- Fp ----
ST_OP(ST_FP_ROUNDTRIP, 1, 6, 6) { (void)stress; Fp x; fp_from_abi(x, in); fp_to_abi(out, x); }
ST_OP(ST_FP_MUL, 1, 12, 6) { (void)stress; Fp x, y, r; fp_from_abi(x, in); fp_from_abi(y, in + 12); fp_mul(r, x, y); fp_to_abi(out, r); }
ST_OP(ST_FP_SQR, 1, 6, 6) { (void)stress; Fp x, r; fp_from_abi(x, in); fp_sqr(r, x); fp_to_abi(out, r); }
ST_OP(ST_FP_MUL2, 1, 24, 6) {       // a b + c d
    (void)stress; Fp a, b, c, d, r; fp_from_abi(a, in); fp_from_abi(b, in + 12); fp_from_abi(c, in + 24); fp_from_abi(d, in + 36);
    fp_mul2(r, a, b, c, d); fp_to_abi(out, r);
}
ST_OP(ST_FP_MUL_SUB, 1, 24, 6) {    // a b - c d
    (void)stress; Fp a, b, c, d, r; fp_from_abi(a, in); fp_from_abi(b, in + 12); fp_from_abi(c, in + 24); fp_from_abi(d, in + 36);
    fmul_sub<4>(r, a, b, c, d); fp_to_abi(out, r);
}
ST_OP(ST_FP_MUL12, 1, 6, 6) {       // 12 (k a): the scaled carry pass on a lazily added, carry-passed operand
    Fp x, t, r; fp_from_abi(x, in); st_lazy(t, x, stress); fp_norm(t, t);
    fp_mul12_norm(r, t); fp_norm(r, r); fp_to_abi(out, r);
}
ST_OP(ST_FP_CANON, 1, 6, 7) {       // the 14 canonical limbs of k a (Montgomery form), un-normalised on the way in
    Fp x, t, c; fp_from_abi(x, in); st_lazy(t, x, stress); fp_canon(c, t);
    for (int i = 0; i < NL; i++) out[i] = c.l[i];
}
ST_OP(ST_FP_ISZERO, 1, 12, 1) {     // bit 0: fp_maybe_zero(a - b), bit 1: fp_is_zero_exact(a - b)
    (void)stress; Fp x, y, t; fp_from_abi(x, in); fp_from_abi(y, in + 12); fp_sub<4>(t, x, y); fp_norm(t, t);
    out[0] = (fp_maybe_zero(t) ? 1u : 0u) | (fp_is_zero_exact(t) ? 2u : 0u); out[1] = 0;
}
ST_OP(ST_FP_INV, 1, 6, 6) {         // 1 / (k a) by division steps
    Fp x, t, r; fp_from_abi(x, in); st_lazy(t, x, stress);
#if defined(__HIP_DEVICE_COMPILE__)
    fp_inv_device(r, t);
#else
    fp_inv_safegcd(r, t);
#endif
    fp_to_abi(out, r);
}
ST_OP(ST_FP_SUBMUL, 1, 18, 6) {     // (a - b) c with lazy subtractions and carry passes around the product
    (void)stress; Fp x, y, z, t, u; fp_from_abi(x, in); fp_from_abi(y, in + 12); fp_from_abi(z, in + 24);
    fp_sub<4>(t, x, y); fp_norm(t, t); fp_mul(t, t, z);
    fp_sub<16>(u, t, x); fp_norm(u, u); fp_add(u, u, x); fp_norm(u, u);
    fp_to_abi(out, u);
}

// ---- Fs ----
ST_OP(ST_FS_ROUNDTRIP, 1, 6, 6) { (void)stress; Fs x; fs_from_abi(x, in); fs_to_abi(out, x); }
ST_OP(ST_FS_MUL, 1, 12, 6) { (void)stress; Fs x, y, r; fs_from_abi(x, in); fs_from_abi(y, in + 12); fs_mul(r, x, y); fs_to_abi(out, r); }
ST_OP(ST_FS_SQR, 1, 6, 6) { (void)stress; Fs x, r; fs_from_abi(x, in); fs_sqr(r, x); fs_to_abi(out, r); }
ST_OP(ST_FS_MUL2, 1, 24, 6) {       // a b + c d
    (void)stress; Fs a, b, c, d, r; fs_from_abi(a, in); fs_from_abi(b, in + 12); fs_from_abi(c, in + 24); fs_from_abi(d, in + 36);
    fs_mul2(r, a, b, c, d); fs_to_abi(out, r);
}
ST_OP(ST_FS_MUL_SUB, 1, 24, 6) {    // a b - c d
    (void)stress; Fs a, b, c, d, r; fs_from_abi(a, in); fs_from_abi(b, in + 12); fs_from_abi(c, in + 24); fs_from_abi(d, in + 36);
    fmul_sub<0>(r, a, b, c, d); fs_to_abi(out, r);
}
ST_OP(ST_FS_NEG, 1, 12, 12) {       // (-a, b odd ? -a : a)
    (void)stress; Fs x, n, c; fs_from_abi(x, in); fs_neg(n, x); fs_cond_neg(c, x, (in[12] & 1u) != 0);
    fs_to_abi(out, n); fs_to_abi(out + 12, c);
}
ST_OP(ST_FS_BAL, 1, 12, 6) {        // k a - k b, one carry pass
    Fs x, y, s, t; fs_from_abi(x, in); fs_from_abi(y, in + 12); st_lazy(s, x, stress); st_lazy(t, y, stress);
    fs_sub(s, s, t); fs_bal(s, s); fs_to_abi(out, s);
}
ST_OP(ST_FS_BAL_WIDE, 1, 18, 6) {   // a - b - c (digits of up to 31 bits), the wide carry pass
    (void)stress; Fs x, y, z, t; fs_from_abi(x, in); fs_from_abi(y, in + 12); fs_from_abi(z, in + 24);
    fs_sub(t, x, y); fs_sub(t, t, z); fs_bal_wide(t, t); fs_to_abi(out, t);
}
ST_OP(ST_FS_ISZERO, 1, 12, 1) {
    (void)stress; Fs x, y, t; fs_from_abi(x, in); fs_from_abi(y, in + 12); fs_sub(t, x, y); fs_bal(t, t);
    out[0] = (fs_maybe_zero(t) ? 1u : 0u) | (fs_is_zero_exact(t) ? 2u : 0u); out[1] = 0;
}
ST_OP(ST_FS_VIA_FP, 1, 6, 12) {     // Fs -> Fp (out) -> Fs (out): the conversions around the inversion
    (void)stress; Fs x, y; Fp f; fs_from_abi(x, in); fp_from_fs(f, x); fp_to_abi(out, f); fs_from_fp(y, f); fs_to_abi(out + 12, y);
}
ST_OP(ST_FS_SUBMUL, 1, 18, 6) {     // (a - b) c - 3 a + 3 a: lazy subtractions, both carry passes, negations
    (void)stress; Fs x, y, z, t, u, v; fs_from_abi(x, in); fs_from_abi(y, in + 12); fs_from_abi(z, in + 24);
    fs_sub(t, x, y); fs_bal(t, t); fs_mul(t, t, z);
    fs_add(u, x, x); fs_add(u, u, x); fs_sub(v, t, u); fs_bal_wide(v, v); fs_neg(v, v); fs_neg(v, v); fs_bal(u, u); fs_add(v, v, u); fs_bal(v, v);
    fs_to_abi(out, v);
}

// ---- Fp2 / Fs2, one lane ----
template <class F2> FD void st_f2_mul(const uint32_t *in, uint32_t *out) { F2 x, y, r; st_ld(x, in); st_ld(y, in + 24); fmul(r, x, y); st_st(out, r); }
template <class F2> FD void st_f2_sqr(const uint32_t *in, uint32_t *out) { F2 x, r; st_ld(x, in); fsqr(r, x); st_st(out, r); }
ST_OP(ST_FP2_MUL, 1, 24, 12) { (void)stress; st_f2_mul<Fp2>(in, out); }
ST_OP(ST_FP2_SQR, 1, 12, 12) { (void)stress; st_f2_sqr<Fp2>(in, out); }
ST_OP(ST_FS2_MUL, 1, 24, 12) { (void)stress; st_f2_mul<Fs2>(in, out); }
ST_OP(ST_FS2_SQR, 1, 12, 12) { (void)stress; st_f2_sqr<Fs2>(in, out); }

// ---- Fr ----
ST_OP(ST_FR_ROUNDTRIP, 1, 4, 4) { fr29::Fr x; fr29::fr_from_words(x, in, stress != 0); fr29::fr_to_words(out, x, stress != 0); }       // stress: the Montgomery flag
ST_OP(ST_FR_MUL, 1, 8, 4) {
    const bool mont = stress != 0; fr29::Fr x, y, r; fr29::fr_from_words(x, in, mont); fr29::fr_from_words(y, in + 8, mont); fr29::fr_mul(r, x, y); fr29::fr_to_words(out, r, mont);
}
ST_OP(ST_FR_BUTTERFLIES, 1, 12, 8) {        // (x, y) -> (x + w y, x - w y), `stress` times, lazily
    fr29::Fr x, y, tw, t, u, v; fr29::fr_from_words(x, in, false); fr29::fr_from_words(y, in + 8, false); fr29::fr_from_words(tw, in + 16, false);
    for (int i = 0; i < stress; i++) { fr29::fr_mul(t, y, tw); fr29::fr_add(u, x, t); fr29::fr_sub(v, x, t); fr29::fr_norm(x, u); fr29::fr_norm(y, v); }
    fr29::fr_to_words(out, x, false); fr29::fr_to_words(out + 8, y, false);
}
ST_OP(ST_FR_CANON, 1, 4, 5) {               // the 10 canonical limbs of k a (Montgomery form)
    fr29::Fr x, t, c; fr29::fr_from_words(x, in, false); t = x; for (int i = 1; i < stress; i++) fr29::fr_add(t, t, x);
    fr29::fr_canon<24>(c, t);
    for (int i = 0; i < fr29::NL; i++) out[i] = c.l[i];
}
ST_OP(ST_FR_INV, 1, 4, 4) {                 // 1 / (k a), k a un-normalised
    fr29::Fr x, t, r; fr29::fr_from_words(x, in, false); t = x; for (int i = 1; i < stress; i++) fr29::fr_add(t, t, x);
    fr29::fr_inv(r, t); fr29::fr_to_words(out, r, false);
}
// Montgomery's trick with each lane taking a strided share (lane g: elements g, g + G, g + 2 G, ... as k_lagrange does); `share` elements per lane,
// the rows are the flat array of G * share elements.  Every element non-zero.
FD void st_fr_batch_inv_lane(const uint32_t *in, uint32_t *out, size_t g, size_t G, int share) {
    auto x = [&](size_t k, fr29::Fr &v) { fr29::fr_from_words(v, in + 8 * (g + k * G), false); };
    auto lo = [&](size_t k, fr29::Fr &v) { fr29::fr_from_words(v, out + 8 * (g + k * G), false); };
    auto so = [&](size_t k, const fr29::Fr &v) { fr29::fr_to_words(out + 8 * (g + k * G), v, false); };
    fr29::fr_batch_inv((size_t)share, x, lo, so);
}

// ---- group law (ec29.hip.h) ----
template <class F> FD void st_ld_aff(Aff<F> &p, const uint32_t *w) { st_ld(p.x, w); st_ld(p.y, w + SW<F>::N); }
template <class F> FD void st_st_xyzz(uint32_t *out, const Xyzz<F> &a, bool inf) {
    constexpr int N = SW<F>::N;
    if (inf) { st_zero(out, 4 * N); return; }
    st_st(out, a.x); st_st(out + N, a.y); st_st(out + 2 * N, a.zz); st_st(out + 3 * N, a.zzz);
}
template <class F> FD void st_id(Xyzz<F> &a) { fzero(a.x); fzero(a.y); fzero(a.zz); fzero(a.zzz); }
FD int st_count(const uint32_t *in) { const int n = (int)(in[0] & 0xffu); return n > ST_MAXP ? ST_MAXP : n; }
// sum of (+/-) points by mixed additions, from the identity
template <class F, bool EARLY> FD void st_madd_chain(const uint32_t *in, uint32_t *out) {
    const int n = st_count(in); const uint32_t neg = in[1];
    Xyzz<F> acc; bool inf = true; st_id(acc);
    for (int i = 0; i < n; i++) {
        Aff<F> p; st_ld_aff(p, in + 2 + 2 * SW<F>::N * i);
        if (EARLY) xyzz_madd_early(acc, inf, p, ((neg >> i) & 1u) != 0); else xyzz_madd(acc, inf, p, ((neg >> i) & 1u) != 0);
    }
    st_st_xyzz(out, acc, inf);
}
// a balanced tree over the row's points by the general addition, kept as a binary counter (slot l holds the sum of 2^l consecutive points, so five
// slots serve ST_MAXP points and the lane's private memory stays small); ROUNDS: merges into even slots take the round-by-round form, the others
// xyzz_add, so each form must accept the other's outputs.  Every leaf enters as (x, y, 1, 1) through a mixed addition onto the identity.
template <class F, bool ROUNDS> FD void st_add_tree(const uint32_t *in, uint32_t *out) {
    static_assert(ST_MAXP < 32, "five slots");
    const int n = st_count(in);
    Xyzz<F> v[5], cur; bool f[5], cf; uint32_t full = 0; QuadSerial q4;
    auto merge = [&](int l) {        // v[l] += cur; cur = v[l]
        if (ROUNDS && !(l & 1)) xyzz_add_rounds(v[l], f[l], cur, cf, q4); else xyzz_add(v[l], f[l], cur, cf);
        cur = v[l]; cf = f[l];
    };
    for (int i = 0; i < n; i++) {
        Aff<F> p; st_ld_aff(p, in + 2 + 2 * SW<F>::N * i);
        cf = true; st_id(cur); xyzz_madd(cur, cf, p, false);
        int l = 0;
        for (; (full >> l) & 1u; l++) { merge(l); full &= ~(1u << l); }
        v[l] = cur; f[l] = cf; full |= 1u << l;
    }
    cf = true; st_id(cur);
    for (int l = 0; l < 5; l++) if ((full >> l) & 1u) merge(l);
    st_st_xyzz(out, cur, cf);
}
// 2^k P through xyzz_dbl_affine and k - 1 doublings (ROUNDS: odd steps in the round-by-round form); k = the row's count, at least 1
template <class F, bool ROUNDS> FD void st_dbl_chain(const uint32_t *in, uint32_t *out) {
    const int k = (int)(in[0] & 0xffu);
    Aff<F> p; st_ld_aff(p, in + 2);
    Xyzz<F> acc; xyzz_dbl_affine(acc, p); QuadSerial q4;
    for (int i = 1; i < k; i++) { Xyzz<F> d; if (ROUNDS && (i & 1)) xyzz_dbl_rounds(d, acc, q4); else xyzz_dbl(d, acc); acc = d; }
    st_st_xyzz(out, acc, false);
}
#define ST_CHAIN_IN(F) (1 + ST_MAXP * SW<F>::N)
#define ST_PT_OUT(F) (2 * SW<F>::N)
ST_OP(ST_G1_MADD, 1, ST_CHAIN_IN(Fp), ST_PT_OUT(Fp)) { (void)stress; st_madd_chain<Fp, false>(in, out); }
ST_OP(ST_G1_TREE, 1, ST_CHAIN_IN(Fp), ST_PT_OUT(Fp)) { (void)stress; st_add_tree<Fp, false>(in, out); }
ST_OP(ST_G1_DBL, 1, ST_CHAIN_IN(Fp), ST_PT_OUT(Fp)) { (void)stress; st_dbl_chain<Fp, false>(in, out); }
ST_OP(ST_G1S_MADD, 1, ST_CHAIN_IN(Fs), ST_PT_OUT(Fs)) { (void)stress; st_madd_chain<Fs, false>(in, out); }
ST_OP(ST_G1S_TREE, 1, ST_CHAIN_IN(Fs), ST_PT_OUT(Fs)) { (void)stress; st_add_tree<Fs, false>(in, out); }
ST_OP(ST_G1S_DBL, 1, ST_CHAIN_IN(Fs), ST_PT_OUT(Fs)) { (void)stress; st_dbl_chain<Fs, false>(in, out); }
ST_OP(ST_G1S_TREE_ROUNDS, 1, ST_CHAIN_IN(Fs), ST_PT_OUT(Fs)) { (void)stress; st_add_tree<Fs, true>(in, out); }
ST_OP(ST_G1S_DBL_ROUNDS, 1, ST_CHAIN_IN(Fs), ST_PT_OUT(Fs)) { (void)stress; st_dbl_chain<Fs, true>(in, out); }
// G2 with one lane per point: host build only (the bound-tracker run of tests/test_gpu_device_arith.py).  Their device kernels are left out: the
// first GPU run of them did not return within its time limit and the cause is not known; on the device G2 is covered through
// the lane-pair and four-lane forms below.
#if !defined(__HIPCC__)
ST_OP(ST_G2_MADD, 1, ST_CHAIN_IN(Fp2), ST_PT_OUT(Fp2)) { (void)stress; st_madd_chain<Fp2, false>(in, out); }
ST_OP(ST_G2_TREE, 1, ST_CHAIN_IN(Fp2), ST_PT_OUT(Fp2)) { (void)stress; st_add_tree<Fp2, false>(in, out); }
ST_OP(ST_G2_DBL, 1, ST_CHAIN_IN(Fp2), ST_PT_OUT(Fp2)) { (void)stress; st_dbl_chain<Fp2, false>(in, out); }
ST_OP(ST_G2S_MADD, 1, ST_CHAIN_IN(Fs2), ST_PT_OUT(Fs2)) { (void)stress; st_madd_chain<Fs2, false>(in, out); }
ST_OP(ST_G2S_MADD_EARLY, 1, ST_CHAIN_IN(Fs2), ST_PT_OUT(Fs2)) { (void)stress; st_madd_chain<Fs2, true>(in, out); }
ST_OP(ST_G2S_TREE, 1, ST_CHAIN_IN(Fs2), ST_PT_OUT(Fs2)) { (void)stress; st_add_tree<Fs2, false>(in, out); }
ST_OP(ST_G2S_DBL, 1, ST_CHAIN_IN(Fs2), ST_PT_OUT(Fs2)) { (void)stress; st_dbl_chain<Fs2, false>(in, out); }
ST_OP(ST_G2S_TREE_ROUNDS, 1, ST_CHAIN_IN(Fs2), ST_PT_OUT(Fs2)) { (void)stress; st_add_tree<Fs2, true>(in, out); }
ST_OP(ST_G2S_DBL_ROUNDS, 1, ST_CHAIN_IN(Fs2), ST_PT_OUT(Fs2)) { (void)stress; st_dbl_chain<Fs2, true>(in, out); }
#endif

// ---- Fp12 (pairing29.hip.h): outputs are fed back in `stress` - 1 times, so the value bounds must close ----
FD void st_ld_f12(Fp12d &f, const uint32_t *w) { Fp *c = reinterpret_cast<Fp *>(&f); for (int k = 0; k < 12; k++) fp_from_abi(c[k], w + 12 * k); }
FD void st_st_f12(uint32_t *w, const Fp12d &f) { const Fp *c = reinterpret_cast<const Fp *>(&f); for (int k = 0; k < 12; k++) fp_to_abi(w + 12 * k, c[k]); }
ST_OP(ST_F12_MUL, 1, 144, 72) {
    Fp12d x, y, r; st_ld_f12(x, in); st_ld_f12(y, in + 144);
    f12_mul(r, x, y);
    for (int i = 1; i < stress; i++) { Fp12d t; f12_mul(t, r, y); r = t; }
    st_st_f12(out, r);
}
ST_OP(ST_F12_MUL_ROLES, 1, 144, 72) {       // every other repetition through f12_mul: both forms must accept each other's outputs
    Fp12d x, y, r; st_ld_f12(x, in); st_ld_f12(y, in + 144);
    f12_mul_roles(r, x, y);
    for (int i = 1; i < stress; i++) { Fp12d t; if (i & 1) f12_mul(t, r, y); else f12_mul_roles(t, r, y); r = t; }
    st_st_f12(out, r);
}
ST_OP(ST_F12_MUL_BY_014, 1, 108, 72) {
    Fp12d x; st_ld_f12(x, in); Fp2 k0, k1, k4; st_ld(k0, in + 144); st_ld(k1, in + 168); st_ld(k4, in + 192);
    for (int i = 0; i < stress; i++) f12_mul_by_014(x, k0, k1, k4);
    st_st_f12(out, x);
}

// ---- the line steps (pairing29.hip.h; what k_miller_lines and k_g2_prepare call): a row is R = (X, Y, Z), plus Q = (x, y) for the addition; the step is
// applied `stress` times with R fed back; out = R', then the last step's three line coefficients ----
FD void st_ld_proj(G2Proj &R, const uint32_t *w) { st_ld(R.x, w); st_ld(R.y, w + 24); st_ld(R.z, w + 48); }
FD void st_st_step(uint32_t *out, const G2Proj &R, const Line &l) {
    st_st(out, R.x); st_st(out + 24, R.y); st_st(out + 48, R.z); st_st(out + 72, l.c0); st_st(out + 96, l.c1); st_st(out + 120, l.c2);
}
ST_OP(ST_LINE_DBL, 1, 36, 72) {
    G2Proj R; Line l; st_ld_proj(R, in); fzero(l.c0); fzero(l.c1); fzero(l.c2);
#pragma unroll 1
    for (int i = 0; i < stress; i++) line_dbl_step(R, l);
    st_st_step(out, R, l);
}
ST_OP(ST_LINE_ADD, 1, 60, 72) {
    G2Proj R; Line l; Aff<Fp2> Q; st_ld_proj(R, in); st_ld_aff(Q, in + 72); fzero(l.c0); fzero(l.c1); fzero(l.c2);
#pragma unroll 1
    for (int i = 0; i < stress; i++) line_add_step(R, Q, l);
    st_st_step(out, R, l);
}

#if defined(__HIPCC__)
// ---- device only: the inversions of fp_inv.hip.h, the lane-shared forms, xyzz_phi ----
ST_DEV_OP(ST_FP2_INV, 1, 12, 12) { (void)stress; Fp2 x, r; st_ld(x, in); finv(r, x); st_st(out, r); }

// a lane pair per element: the even lane holds c0, the odd lane c1, of every operand and of the result
__device__ __forceinline__ void st_ldh(Fp2H &r, const uint32_t *w) { fp_from_abi(r.v, w + (pair_odd() ? 12 : 0)); }
__device__ __forceinline__ void st_ldh(Fs2H &r, const uint32_t *w) { fs_from_abi(r.v, w + (spair_odd() ? 12 : 0)); }
__device__ __forceinline__ void st_sth(uint32_t *w, const Fp2H &a) { fp_to_abi(w + (pair_odd() ? 12 : 0), a.v); }
__device__ __forceinline__ void st_sth(uint32_t *w, const Fs2H &a) { fs_to_abi(w + (spair_odd() ? 12 : 0), a.v); }
template <> struct SW<Fp2H> { static constexpr int N = 24; };
ST_DEV_OP(ST_FP2H_MUL, 2, 24, 12) { (void)stress; Fp2H x, y, r; st_ldh(x, in); st_ldh(y, in + 24); fmul(r, x, y); st_sth(out, r); }
ST_DEV_OP(ST_FP2H_SQR, 2, 12, 12) { (void)stress; Fp2H x, r; st_ldh(x, in); fsqr(r, x); st_sth(out, r); }
ST_DEV_OP(ST_FP2H_MUL_SUB, 2, 48, 12) {
    (void)stress; Fp2H a, b, c, d, r; st_ldh(a, in); st_ldh(b, in + 24); st_ldh(c, in + 48); st_ldh(d, in + 72);
    fmul_sub<SubM<Fp2H>::YN>(r, a, b, c, d); st_sth(out, r);
}
ST_DEV_OP(ST_FP2H_SQR_M, 2, 12, 12) { (void)stress; Fp2H x, r; st_ldh(x, in); f2_sqr_m<64>(r, x); st_sth(out, r); }
ST_DEV_OP(ST_FP2H_MUL_XI_N, 2, 12, 12) { (void)stress; Fp2H x, r; st_ldh(x, in); f2_mul_xi_n<8>(r, x); st_sth(out, r); }
ST_DEV_OP(ST_FP2H_INV, 2, 12, 12) { (void)stress; Fp2H x, r; st_ldh(x, in); finv(r, x); st_sth(out, r); }
ST_DEV_OP(ST_FS2H_MUL, 2, 24, 12) { (void)stress; Fs2H x, y, r; st_ldh(x, in); st_ldh(y, in + 24); fmul(r, x, y); st_sth(out, r); }
ST_DEV_OP(ST_FS2H_MUL_TWO, 2, 48, 24) {     // (a b, c d)
    (void)stress; Fs2H a, b, c, d, r1, r2; st_ldh(a, in); st_ldh(b, in + 24); st_ldh(c, in + 48); st_ldh(d, in + 72);
    fmul_two(r1, r2, a, b, c, d); st_sth(out, r1); st_sth(out + 24, r2);
}
ST_DEV_OP(ST_FS2H_SQR, 2, 12, 12) { (void)stress; Fs2H x, r; st_ldh(x, in); fsqr(r, x); st_sth(out, r); }
ST_DEV_OP(ST_FS2H_MUL_SUB, 2, 48, 12) {
    (void)stress; Fs2H a, b, c, d, r; st_ldh(a, in); st_ldh(b, in + 24); st_ldh(c, in + 48); st_ldh(d, in + 72);
    fmul_sub<0>(r, a, b, c, d); st_sth(out, r);
}

// two lanes per G1 point (Share2): both hold the whole point; the even lane stores X, Y and the odd lane ZZ, ZZZ, so both copies are checked
__device__ __forceinline__ void st_st_xyzz_2l(uint32_t *out, const Xyzz<Fp> &a, bool inf) {
    const bool B = pair_odd(); uint32_t *o = out + (B ? 24 : 0);
    if (inf) { st_zero(o, 24); return; }
    fp_to_abi(o, B ? a.zz : a.x); fp_to_abi(o + 12, B ? a.zzz : a.y);
}
ST_DEV_OP(ST_G1_MADD_2L, 2, ST_CHAIN_IN(Fp), ST_PT_OUT(Fp)) {
    (void)stress; const int n = st_count(in); const uint32_t neg = in[1];
    Xyzz<Fp> acc; bool inf = true; st_id(acc);
    for (int i = 0; i < n; i++) { Aff<Fp> p; st_ld_aff(p, in + 2 + 24 * i); xyzz_madd_2l(acc, inf, p, ((neg >> i) & 1u) != 0); }
    st_st_xyzz_2l(out, acc, inf);
}
ST_DEV_OP(ST_G1_DBL_2L, 2, ST_CHAIN_IN(Fp), ST_PT_OUT(Fp)) {      // 2^k P: P as (x, y, 1, 1), k shared doublings
    (void)stress; const int k = (int)(in[0] & 0xffu);
    Aff<Fp> p; st_ld_aff(p, in + 2);
    Xyzz<Fp> acc; acc.x = p.x; acc.y = p.y; fset_one(acc.zz); fset_one(acc.zzz);
    for (int i = 0; i < k; i++) { Xyzz<Fp> d; xyzz_dbl_2l(d, acc); acc = d; }
    st_st_xyzz_2l(out, acc, false);
}
// four lanes per G2 point (Share4 over Fp2H): the pairs of a quad both hold the point, halves on the lanes of a pair; pair A stores X, Y, pair B ZZ, ZZZ
__device__ __forceinline__ void st_ld_affh(Aff<Fp2H> &p, const uint32_t *w) { st_ldh(p.x, w); st_ldh(p.y, w + 24); }
__device__ __forceinline__ void st_st_xyzz_4l(uint32_t *out, const Xyzz<Fp2H> &a, bool inf) {
    const bool B = Share4::role(); uint32_t *o = out + (B ? 48 : 0);
    if (inf) { st_zero(o + (pair_odd() ? 12 : 0), 12); st_zero(o + 24 + (pair_odd() ? 12 : 0), 12); return; }
    st_sth(o, B ? a.zz : a.x); st_sth(o + 24, B ? a.zzz : a.y);
}
ST_DEV_OP(ST_G2_MADD_4L, 4, ST_CHAIN_IN(Fp2), ST_PT_OUT(Fp2)) {
    (void)stress; const int n = st_count(in); const uint32_t neg = in[1];
    Xyzz<Fp2H> acc; bool inf = true; st_id(acc);
    for (int i = 0; i < n; i++) { Aff<Fp2H> p; st_ld_affh(p, in + 2 + 48 * i); xyzz_madd_shared<Fp2H, Share4>(acc, inf, p, ((neg >> i) & 1u) != 0); }
    st_st_xyzz_4l(out, acc, inf);
}
ST_DEV_OP(ST_G2_DBL_4L, 4, ST_CHAIN_IN(Fp2), ST_PT_OUT(Fp2)) {
    (void)stress; const int k = (int)(in[0] & 0xffu);
    Aff<Fp2H> p; st_ld_affh(p, in + 2);
    Xyzz<Fp2H> acc; acc.x = p.x; acc.y = p.y; fset_one(acc.zz); fset_one(acc.zzz);
    for (int i = 0; i < k; i++) { Xyzz<Fp2H> d; xyzz_dbl_shared<Fp2H, Share4>(d, acc); acc = d; }
    st_st_xyzz_4l(out, acc, false);
}
ST_DEV_OP(ST_G1_PHI, 1, ST_CHAIN_IN(Fp), ST_PT_OUT(Fp)) {        // phi(sum of the row's chain); the identity stays the identity
    (void)stress; const int n = st_count(in); const uint32_t neg = in[1];
    Xyzz<Fp> acc; bool inf = true; st_id(acc);
    for (int i = 0; i < n; i++) { Aff<Fp> p; st_ld_aff(p, in + 2 + 24 * i); xyzz_madd(acc, inf, p, ((neg >> i) & 1u) != 0); }
    if (!inf) xyzz_phi(acc);
    st_st_xyzz(out, acc, inf);
}
// affine form of the row's chain sum: (x, y), then one word = 1 for the identity (x, y zero)
template <class F> __device__ __forceinline__ void st_to_affine(const uint32_t *in, uint32_t *out) {
    constexpr int N = SW<F>::N;
    const int n = st_count(in); const uint32_t neg = in[1];
    Xyzz<F> acc; bool inf = true; st_id(acc);
    for (int i = 0; i < n; i++) { Aff<F> p; st_ld_aff(p, in + 2 + 2 * N * i); xyzz_madd(acc, inf, p, ((neg >> i) & 1u) != 0); }
    out[2 * N] = inf ? 1u : 0u; out[2 * N + 1] = 0;
    if (inf) { st_zero(out, 2 * N); return; }
    Aff<F> a; xyzz_to_affine(a, acc);
    st_st(out, a.x); st_st(out + N, a.y);
}
ST_DEV_OP(ST_G1_TO_AFFINE, 1, ST_CHAIN_IN(Fp), 13) { (void)stress; st_to_affine<Fp>(in, out); }
ST_DEV_OP(ST_G2H_TO_AFFINE, 2, ST_CHAIN_IN(Fp2), 25) {            // the lane-pair form: each lane stores its halves, the even lane the flag
    (void)stress; const int n = st_count(in); const uint32_t neg = in[1];
    Xyzz<Fp2H> acc; bool inf = true; st_id(acc);
    for (int i = 0; i < n; i++) { Aff<Fp2H> p; st_ld_affh(p, in + 2 + 48 * i); xyzz_madd(acc, inf, p, ((neg >> i) & 1u) != 0); }
    if (!pair_odd()) { out[48] = inf ? 1u : 0u; out[49] = 0; }
    if (inf) { st_zero(out + (pair_odd() ? 12 : 0), 12); st_zero(out + 24 + (pair_odd() ? 12 : 0), 12); return; }
    Aff<Fp2H> a; xyzz_to_affine(a, acc);
    st_sth(out, a.x); st_sth(out + 24, a.y);
}

// ---- the kernels: one instantiation per op ----
template <int OP> __global__ void __launch_bounds__(64) k_selftest_arith(const uint32_t *__restrict__ in, size_t n, uint32_t *__restrict__ out, int stress) {
    using O = StOp<OP>;
    const size_t row = ((size_t)blockIdx.x * 64 + threadIdx.x) / O::LANES;      // 64 is a multiple of LANES: the lanes of a row live or leave together
    if (row >= n) return;
    O::run(in + row * (size_t)(2 * O::IN64), out + row * (size_t)(2 * O::OUT64), stress);
}
#if !defined(ST_PART) || ST_PART == 0      // (the kernels that are no templates: in one part of k_selftest.hip only)
__global__ void __launch_bounds__(64) k_selftest_fr_batch_inv(const uint32_t *__restrict__ in, size_t G, uint32_t *__restrict__ out, int share) {
    const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= G) return;
    st_fr_batch_inv_lane(in, out, g, G, share);
}

// ---- the two self-tests that predate this unit (tests/test_gpu_msm.py, tests/perf/gpu_check.py) ----
__global__ void k_selftest_fp_mul(const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp x, y, r; fp_from_abi(x, a + 12 * i); fp_from_abi(y, b + 12 * i);
    fp_mul(r, x, y);
    fp_to_abi(out + 12 * i, r);
}
// one thread: sum of (+/-) points by mixed additions, result in ABI XYZZ form
__global__ void k_selftest_g1_sum(const uint32_t *pts_abi, const uint8_t *neg, size_t n, uint32_t *out, uint8_t *out_inf) {
    if (blockIdx.x || threadIdx.x) return;
    Xyzz<Fp> acc; bool inf = true;
    fzero(acc.x); fzero(acc.y); fzero(acc.zz); fzero(acc.zzz);
    for (size_t i = 0; i < n; i++) {
        Aff<Fp> p; fp_from_abi(p.x, pts_abi + 24 * i); fp_from_abi(p.y, pts_abi + 24 * i + 12);
        xyzz_madd(acc, inf, p, neg && neg[i]);
    }
    *out_inf = inf;
    if (!inf) { fp_to_abi(out, acc.x); fp_to_abi(out + 12, acc.y); fp_to_abi(out + 24, acc.zz); fp_to_abi(out + 36, acc.zzz); }
}
#endif   // ST_PART
#endif   // __HIPCC__

}  // namespace selftest
