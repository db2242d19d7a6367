// crypto_amd/csrc/serde_kernels.hip.h — point decompression and validation on the device: the per-point work of dock_serde.cpp's
// dgpu_g1_deserialize / dgpu_g2_deserialize / dock::g*_words_valid, one point per lane, over the lazy 29-bit-limb fields (fp29.hip.h).
//
// The per-point routines are __host__ __device__ (FD) so tests/native/serde_dev_host_shim.cpp runs them on the host under the FP29_CHECK
// bound tracker.  They take the same decisions as the host code, in the same order of checks:
//   parse     big-endian coordinates, flags (compressed, infinity, largest) in the top bits of byte 0; G2 stores c1 before c0;
//   decompress  y^2 = x^3 + 4 (G1) / x^3 + 4 (1 + u) (G2); the sign from the flag ("largest": y > (p - 1) / 2, arkworks' c1-then-c0 order on Fq2);
//   validate  unless DGPU_SERDE_NO_VALIDATE: phi(P) + P == [x^2] P (G1), psi(P) == [x] P (G2), with the constants of dock_serde.cpp.
// Square roots use one exponentiation t = a^((p - 3) / 4) in Fq: sqrt(a) = t a, and 1 / sqrt(a) = t when a is a square.  The Fq2 root is the
// complex method with its inversion replaced by t (see fq2_sqrt_dev): two Fq exponentiations per G2 point, no inversion.
// Every lane runs the same instruction stream whatever its point (identity, malformed or not): the verdict only selects what is written.
//
// The other direction, dgpu_g1_serialize / dgpu_g2_serialize's bytes: encode_point takes affine ABI words, record_to_abi reads a resident base
// record (what k_prep_bases writes, also row 0 of a precomputed table) back to ABI words.  Canonical values come from fp_from_abi + fp_int, the
// "largest" flag from int_is_high (Fq2: c1, or c0 when c1 = 0, as dock_serde.cpp is_high2), the bytes from the inverses of be48_to_u64 and
// fp_from_canonical's split.
#pragma once
#include "fp29.hip.h"
#include "fp2_29.hip.h"
#include "ec29.hip.h"
#include "fp30s.hip.h"

namespace serde {
using namespace bls29;

enum : uint32_t { FLAG_COMPRESSED = 0x80000000u, FLAG_INF = 0x40000000u, FLAG_LARGEST = 0x20000000u };
constexpr uint64_t X_ABS = 0xd201000000010000ULL;                // |x|, the BLS parameter x is negative

FD uint32_t bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// 48 big-endian bytes (12 native-order 32-bit words as loaded from memory) -> six little-endian 64-bit limbs; `top_mask` clears flag bits of word 0
FD void be48_to_u64(uint64_t c[6], const uint32_t *w, uint32_t top_mask) {
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const uint32_t hi = bswap32(w[2 * (5 - i)]) & (i == 5 ? top_mask : 0xffffffffu), lo = bswap32(w[2 * (5 - i) + 1]);
        c[i] = ((uint64_t)hi << 32) | lo;
    }
}
FD bool u64_lt_p(const uint64_t c[6]) {
    constexpr uint64_t P64[6] = {0xb9feffffffffaaabULL, 0x1eabfffeb153ffffULL, 0x6730d2a0f6b0f624ULL, 0x64774b84f38512bfULL, 0x4b1ba7b6434bacd7ULL, 0x1a0111ea397fe69aULL};
    bool lt = false, decided = false;
#pragma unroll
    for (int i = 5; i >= 0; i--) { if (!decided && c[i] != P64[i]) { lt = c[i] < P64[i]; decided = true; } }
    return lt;
}
// canonical integer c < p (six 64-bit limbs) -> Montgomery form c 2^406: the 29-bit split of c times 2^812 mod p
FD void fp_from_canonical(Fp &r, const uint64_t c[6]) {
    constexpr uint32_t K812[NL] = {0x15bef7aeu, 0x1031cd0eu, 0x2dd93e8u, 0x9226323u, 0xe6e2cd2u, 0x11684daau, 0x1170e5dbu, 0x88e25b1u, 0x1b366399u, 0x1c536f47u, 0xd1f9cbcu, 0x278b67fu, 0x1ea66a2bu, 0xcu};
    Fp t, k;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const int bit = i * LB, wi = bit >> 6, sh = bit & 63;
        uint64_t v = c[wi] >> sh;
        if (sh + LB > 64 && wi + 1 < 6) v |= c[wi + 1] << (64 - sh);
        t.l[i] = (uint32_t)v & (i == NL - 1 ? 0xffffffffu : LMASK);
        k.l[i] = K812[i];
    }
    CHK(chk_set_N(t, 1.0); chk_set_N(k, 1.0);)
    fp_mul(r, t, k);
}
// Montgomery words with R = 2^384 (the ABI's form) of a host constant -> this field
FD void fp_from_u64(Fp &r, const uint64_t c[6]) {
    uint32_t w[12];
#pragma unroll
    for (int i = 0; i < 6; i++) { w[2 * i] = (uint32_t)c[i]; w[2 * i + 1] = (uint32_t)(c[i] >> 32); }
    fp_from_abi(r, w);
}
// abi words (12 x 32 bit, i.e. six 64-bit limbs) below p?
FD bool abi_lt_p(const uint32_t *w) {
    uint64_t c[6];
#pragma unroll
    for (int i = 0; i < 6; i++) c[i] = ((uint64_t)w[2 * i + 1] << 32) | w[2 * i];
    return u64_lt_p(c);
}

// ---- exact predicates -------------------------------------------------------------------------------------------------------------------
FD bool feq(const Fp &a, const Fp &b) { Fp d; fp_sub<64>(d, a, b); fp_norm(d, d); return fp_is_zero_exact(d); }
FD bool feq(const Fp2 &a, const Fp2 &b) { return feq(a.c0, b.c0) && feq(a.c1, b.c1); }
// canonical value in [0, p) (29-bit limbs) of a field element
FD void fp_int(Fp &c, const Fp &a) {
    Fp one; fp_zero(one); one.l[0] = 1;
    CHK(chk_set_N(one, 1.0);)
    Fp t; fp_mul(t, a, one);              // a 2^406 / 2^406
    fp_canon(c, t);
}
FD bool fp_int_is_zero(const Fp &c) { uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) o |= c.l[i];
    return o == 0; }
// c > (p - 1) / 2 for a canonical c  <=>  2 c mod p is odd (2 c < p leaves 2 c, even; otherwise 2 c - p, odd)
FD bool int_is_high(const Fp &c) { Fp d, e; fp_add(d, c, c); fp_canon(e, d); return (e.l[0] & 1u) != 0; }
FD bool is_high(const Fp &a) { Fp c; fp_int(c, a); return int_is_high(c); }
// arkworks' lexicographic order on Fq2: c1 first, c0 when c1 = 0
FD bool is_high(const Fp2 &a) { Fp c1, c0; fp_int(c1, a.c1); fp_int(c0, a.c0); return fp_int_is_zero(c1) ? int_is_high(c0) : int_is_high(c1); }
FD void fneg(Fp &r, const Fp &a) { Fp z; fp_zero(z); fp_sub<32>(r, z, a); fp_norm(r, r); }       // value grows by 32 p
FD void fneg(Fp2 &r, const Fp2 &a) { fneg(r.c0, a.c0); fneg(r.c1, a.c1); }
// the same value below 2 p (a product with one): what the group law expects of an affine coordinate
FD void freduce(Fp &r, const Fp &a) { Fp one; fp_set_one(one); fp_mul(r, a, one); }
FD void freduce(Fp2 &r, const Fp2 &a) { freduce(r.c0, a.c0); freduce(r.c1, a.c1); }
FD void fsel(Fp &r, bool c, const Fp &a, const Fp &b) { r = c ? a : b; }

// a^((p - 3) / 4): a fixed 2-bit window over the 379-bit exponent (378 squarings, 142 products, a table of a, a^2, a^3); the loop stays rolled
FD void fp_pow_pm3d4(Fp &r, const Fp &a) {
    constexpr uint64_t E[6] = {0xee7fbfffffffeaaaULL, 0x07aaffffac54ffffULL, 0xd9cc34a83dac3d89ULL, 0xd91dd2e13ce144afULL, 0x92c6e9ed90d2eb35ULL, 0x0680447a8e5ff9a6ULL};
    Fp a2, a3, acc;
    fp_sqr(a2, a); fp_mul(a3, a2, a);
    acc = a;                                                         // bit 378
#pragma unroll 1
    for (int k = 376; k >= 0; k -= 2) {                              // bits k + 1, k (one 64-bit word: k is even)
        fp_sqr(acc, acc); fp_sqr(acc, acc);
        const int j = k >> 6;                                        // (a select chain, not an indexed load: the array stays out of memory)
        const uint64_t e = j == 0 ? E[0] : j == 1 ? E[1] : j == 2 ? E[2] : j == 3 ? E[3] : j == 4 ? E[4] : E[5];
        const uint32_t w = (uint32_t)(e >> (k & 63)) & 3u;
        if (w) fp_mul(acc, acc, w == 1 ? a : (w == 2 ? a2 : a3));
    }
    r = acc;
}
// y = sqrt(a) if a is a square (returns false otherwise; y is then meaningless)
FD bool fq_sqrt_dev(Fp &y, const Fp &a) {
    Fp t, s, s2; fp_pow_pm3d4(t, a); fp_mul(s, t, a); fp_sqr(s2, s);
    y = s;
    return feq(s2, a);
}
// Fq2 square root, any root (the caller fixes the sign).  Complex method: alpha = sqrt(a0^2 + a1^2), delta = (a0 + alpha) / 2, t = delta^((p-3)/4),
// s = t delta.  If delta is a square (chi = t s = 1): sqrt(a) = s + (a1 t / 2) u, because 1 / s = t.  Otherwise (chi = -1) the other delta
// (a0 - alpha) / 2 = -a1^2 / (4 delta) is the square and sqrt(a) = -(a1 t / 2) + s u (s^2 = -delta, t^2 = -1 / delta).  a1 = 0: delta = a0 and the same
// two forms give sqrt(a0) or sqrt(-a0) u.  The candidate is checked by squaring, which also refuses a non-square a (no root of the norm).
FD bool fq2_sqrt_dev(Fp2 &y, const Fp2 &a) {
    constexpr uint64_t HALF[6] = {0x1804000000015554ULL, 0x855000053ab00001ULL, 0x633cb57c253c276fULL, 0x6e22d1ec31ebb502ULL, 0xd3916126f2d14ca2ULL, 0x17fbb8571a006596ULL};   // 1/2
    Fp half, nrm, tn, alpha, d, delta, t, s, chi, h, one, nh;
    fp_from_u64(half, HALF);
    fp_mul2(nrm, a.c0, a.c0, a.c1, a.c1);
    fp_pow_pm3d4(tn, nrm); fp_mul(alpha, tn, nrm);
    fp_add(d, a.c0, alpha); fp_norm(d, d); fp_mul(d, d, half);
    const bool a1_zero = fp_is_zero_exact(a.c1);
    fsel(delta, a1_zero, a.c0, d);
    fp_pow_pm3d4(t, delta); fp_mul(s, t, delta); fp_mul(chi, t, s);
    fp_set_one(one);
    const bool qr = feq(chi, one);
    fp_mul(h, a.c1, t); fp_mul(h, h, half);
    fneg(nh, h);
    Fp2 cand; fsel(cand.c0, qr, s, nh); fsel(cand.c1, qr, h, s);
    Fp2 sq; fsqr(sq, cand);
    freduce(y.c0, cand.c0); y.c1 = cand.c1;
    return feq(sq, a);
}

// ---- subgroup tests (dock_serde.cpp in_prime_subgroup) ------------------------------------------------------------------------------------
// a := 2 a unless a is the identity (no point of order 2 exists on either curve, so a doubling never yields the identity itself)
template <class F> FD void dbl_flag(Xyzz<F> &a, bool inf) { if (!inf) { Xyzz<F> d; xyzz_dbl(d, a); a = d; } }
template <class F> FD void from_affine(Xyzz<F> &r, const Aff<F> &p) { r.x = p.x; r.y = p.y; fset_one(r.zz); fset_one(r.zzz); }
// [|x|] P of an affine P: 63 doublings and 5 mixed additions (the top bit loads P); an intermediate identity (P of order 3) is carried by the flag
template <class F> FD void mul_x_abs(Xyzz<F> &acc, bool &inf, const Aff<F> &p) {
    from_affine(acc, p); inf = false;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        dbl_flag(acc, inf);
        if ((X_ABS >> i) & 1) xyzz_madd(acc, inf, p, false);
    }
}
// [|x|] Q of a projective Q (with its identity flag): the general addition
template <class F> FD void mul_x_abs(Xyzz<F> &acc, bool &inf, const Xyzz<F> &q, bool qinf) {
    acc = q; inf = qinf;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        dbl_flag(acc, inf);
        if ((X_ABS >> i) & 1) xyzz_add(acc, inf, q, qinf);
    }
}
// a == b as points (identity flags included)
template <class F> FD bool same_point(const Xyzz<F> &a, bool ainf, const Xyzz<F> &b, bool binf) {
    F l, r, l2, r2;
    fmul(l, a.x, b.zz); fmul(r, b.x, a.zz);
    fmul(l2, a.y, b.zzz); fmul(r2, b.y, a.zzz);
    const bool eq = feq(l, r) && feq(l2, r2);
    return (ainf || binf) ? (ainf && binf) : eq;
}
// G1: phi(P) + P == [x^2] P, phi(x, y) = (beta x, y); P affine on the curve
FD bool g1_in_subgroup(const Aff<Fp> &p) {
    constexpr uint64_t BETA[6] = {0xcd03c9e48671f071ULL, 0x5dab22461fcda5d2ULL, 0x587042afd3851b95ULL, 0x8eb60ebe01bacb9eULL, 0x03f97d6e83d050d2ULL, 0x18f0206554638741ULL};
    Fp beta; fp_from_u64(beta, BETA);
    Aff<Fp> ph; fp_mul(ph.x, beta, p.x); ph.y = p.y;
    Xyzz<Fp> lhs; bool linf = false; from_affine(lhs, ph);
    xyzz_madd(lhs, linf, p, false);
    Xyzz<Fp> x1, x2; bool i1, i2;
    mul_x_abs(x1, i1, p);
    mul_x_abs(x2, i2, x1, i1);
    return same_point(lhs, linf, x2, i2);
}
// G2: psi(P) == [x] P = -[|x|] P, psi(x, y) = (c1 conj(x), c2 conj(y)); P affine on the twist.
// On the device this is a real call: inlined into the decoding kernels (256 VGPRs + 256 AGPRs + scratch) it returned "outside G2" for points of
// G2 while the same source built for the host was right; as a call every verdict matches (tests/test_gpu_serde_device.py) and the kernels need
// less scratch.  The cause was not found.
#if defined(__HIPCC__)
__host__ __device__ __noinline__
#else
FD
#endif
bool g2_in_subgroup(const Aff<Fp2> &p) {
    constexpr uint64_t C1[6] = {0x890dc9e4867545c3ULL, 0x2af322533285a5d5ULL, 0x50880866309b7e2cULL, 0xa20d1b8c7e881024ULL, 0x14e4f04fe2db9068ULL, 0x14e56d3f1564853aULL};
    constexpr uint64_t C20[6] = {0x3e2f585da55c9ad1ULL, 0x4294213d86c18183ULL, 0x382844c88b623732ULL, 0x92ad2afd19103e18ULL, 0x1d794e4fac7cf0b9ULL, 0x0bd592fc7d825ec8ULL};
    constexpr uint64_t C21[6] = {0x7bcfa7a25aa30fdaULL, 0xdc17dec12a927e7cULL, 0x2f088dd86b4ebef1ULL, 0xd1ca2087da74d4a7ULL, 0x2da2596696cebc1dULL, 0x0e2b7eedbbfd87d2ULL};
    Fp2 c1, c2, xc, yc;
    fp_zero(c1.c0); fp_from_u64(c1.c1, C1); fp_from_u64(c2.c0, C20); fp_from_u64(c2.c1, C21);
    fneg_c1(xc, p.x); fnorm(xc, xc);
    fneg_c1(yc, p.y); fnorm(yc, yc);
    Xyzz<Fp2> psi, xp; bool xinf;
    fmul(psi.x, c1, xc); fmul(psi.y, c2, yc); fset_one(psi.zz); fset_one(psi.zzz);
    mul_x_abs(xp, xinf, p);
    fneg(xp.y, xp.y);                                                 // x is negative
    return same_point(psi, false, xp, xinf);
}

// ---- per-point routines ---------------------------------------------------------------------------------------------------------------------
FD void b_g1(Fp &b) { Fp one; fp_set_one(one); fp_add(b, one, one); fp_add(b, b, b); fp_norm(b, b); }           // 4
FD void b_g2(Fp2 &b) { b_g1(b.c0); b.c1 = b.c0; }                                                                 // 4 (1 + u)
FD void rhs_of(Fp &r, const Fp &x) { Fp b, t; b_g1(b); fp_sqr(t, x); fp_mul(t, t, x); fp_add(t, t, b); fp_norm(r, t); }
FD void rhs_of(Fp2 &r, const Fp2 &x) { Fp2 b, t; b_g2(b); fsqr(t, x); fmul(t, t, x); fadd(t, t, b); fnorm(r, t); }
FD bool sqrt_of(Fp &y, const Fp &a) { return fq_sqrt_dev(y, a); }
FD bool sqrt_of(Fp2 &y, const Fp2 &a) { return fq2_sqrt_dev(y, a); }
FD bool in_subgroup(const Aff<Fp> &p) { return g1_in_subgroup(p); }
FD bool in_subgroup(const Aff<Fp2> &p) { return g2_in_subgroup(p); }
FD void store_abi(uint32_t *w, const Fp &a) { fp_to_abi(w, a); }
FD void store_abi(uint32_t *w, const Fp2 &a) { fp_to_abi(w, a.c0); fp_to_abi(w + 12, a.c1); }
FD void load_abi(Fp &a, const uint32_t *w) { fp_from_abi(a, w); }
FD void load_abi(Fp2 &a, const uint32_t *w) { fp_from_abi(a.c0, w); fp_from_abi(a.c1, w + 12); }

template <class F> struct Curve;
template <> struct Curve<Fp> { static constexpr int NFP = 1; };
template <> struct Curve<Fp2> { static constexpr int NFP = 2; };

// one coordinate (48 big-endian bytes): ok := ok && value < p; a value >= p is replaced by 0 for the arithmetic (the point is refused anyway)
FD void load_coord(Fp &r, const uint32_t *w, uint32_t top_mask, bool &ok) {
    uint64_t c[6]; be48_to_u64(c, w, top_mask);
    const bool lt = u64_lt_p(c); ok = ok && lt;
#pragma unroll
    for (int i = 0; i < 6; i++) c[i] = lt ? c[i] : 0;
    fp_from_canonical(r, c);
}
FD void load_coord(Fp2 &r, const uint32_t *w, uint32_t top_mask, bool &ok) { load_coord(r.c1, w, top_mask, ok); load_coord(r.c0, w + 12, 0xffffffffu, ok); }   // c1 first

// One encoded point (rec: its 48 / 96 / 192 bytes as native-order 32-bit words) in the compressed (COMP) or uncompressed form.  Returns true if
// accepted; then out (2 NFP x 12 words: x, y as ABI Montgomery limbs; zeros for the identity) and *inf hold the point.  The same checks as
// dgpu_g*_deserialize: compression flag, canonical infinity, no "largest" flag on an uncompressed point, coordinates < p, on the curve (a root
// exists / y^2 = x^3 + b), and with `validate` the subgroup test.
template <class F, bool COMP>
FD bool decode_point(const uint32_t *rec, bool validate, uint32_t *out, uint8_t *inf) {
    constexpr int K = Curve<F>::NFP, WORDS = (COMP ? 12 : 24) * K;
    const uint32_t w0 = bswap32(rec[0]);
    const bool flag_ok = ((w0 & FLAG_COMPRESSED) != 0) == COMP;
    const bool is_inf = (w0 & FLAG_INF) != 0, largest = (w0 & FLAG_LARGEST) != 0;
    uint32_t payload = w0 & 0x1fffffffu;
#pragma unroll
    for (int k = 1; k < WORDS; k++) payload |= rec[k];
    const bool inf_ok = !largest && payload == 0;                    // a canonical infinity: no other flag, no payload bit
    bool coords_ok = true;
    F x, y, rhs;
    load_coord(x, rec, 0x1fffffffu, coords_ok);
    rhs_of(rhs, x);
    bool on_curve;
    if constexpr (COMP) {
        on_curve = sqrt_of(y, rhs);
        F ny; fneg(ny, y);
        if (is_high(y) != largest) y = ny;
        freduce(y, y);
    } else {
        load_coord(y, rec + 12 * K, 0xffffffffu, coords_ok);
        F y2; fsqr(y2, y);
        on_curve = feq(y2, rhs);
    }
    bool sub = true;
    if (validate) { const Aff<F> p{x, y}; sub = in_subgroup(p); }
    const bool ok = flag_ok && (is_inf ? inf_ok : ((COMP || !largest) && coords_ok && on_curve && sub));
    if (ok) {
        if (is_inf) {
#pragma unroll
            for (int k = 0; k < 24 * K; k++) out[k] = 0;
        } else { store_abi(out, x); store_abi(out + 12 * K, y); }
        *inf = is_inf ? 1 : 0;
    }
    return ok;
}

// Validate::Yes of affine ABI words (w: 2 NFP x 12 words): dock::g1_words_valid / g2_words_valid, plus the is_inf flag of the ABI
template <class F>
FD bool words_valid(const uint32_t *w, bool inf_flag) {
    constexpr int K = Curve<F>::NFP;
    uint32_t any = 0; bool reduced = true;
#pragma unroll
    for (int k = 0; k < 24 * K; k++) any |= w[k];
#pragma unroll
    for (int k = 0; k < 2 * K; k++) reduced = reduced && abi_lt_p(w + 12 * k);
    Aff<F> p; load_abi(p.x, w); load_abi(p.y, w + 12 * K);
    F rhs, y2; rhs_of(rhs, p.x); fsqr(y2, p.y);
    const bool on_curve = feq(y2, rhs);
    const bool sub = in_subgroup(p);
    return inf_flag || any == 0 || (reduced && on_curve && sub);
}


// ---- encoding (dgpu_g*_serialize on the device) -----------------------------------------------------------------------------------------------
// canonical 29-bit limbs (fp_int) -> six little-endian 64-bit limbs: the inverse of fp_from_canonical's split
FD void int_to_u64(uint64_t c[6], const Fp &a) {
#pragma unroll
    for (int i = 0; i < 6; i++) c[i] = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const int bit = i * LB, wi = bit >> 6, sh = bit & 63;
        c[wi] |= (uint64_t)a.l[i] << sh;
        if (sh + LB > 64 && wi + 1 < 6) c[wi + 1] |= (uint64_t)a.l[i] >> (64 - sh);
    }
}
// six little-endian 64-bit limbs -> 48 big-endian bytes as 12 native-order 32-bit words: the inverse of be48_to_u64
FD void u64_to_be48(uint32_t *w, const uint64_t c[6]) {
#pragma unroll
    for (int i = 0; i < 6; i++) { w[2 * (5 - i)] = bswap32((uint32_t)(c[i] >> 32)); w[2 * (5 - i) + 1] = bswap32((uint32_t)c[i]); }
}
// the canonical value in [0, p) of one coordinate component given as ABI words (Montgomery limbs, R = 2^384)
FD void abi_int(Fp &c, const uint32_t *w) { Fp a; fp_from_abi(a, w); fp_int(c, a); }

// Affine ABI words w (2 NFP x 12 words: x then y, c0 before c1) -> the point's record (12 / 24 NFP native-order words) in the compressed (COMP)
// or uncompressed form: the bytes of dgpu_g*_serialize.  The identity (inf_flag, or all-zero words) is the flag byte followed by zeros.
template <class F, bool COMP>
FD void encode_point(const uint32_t *w, bool inf_flag, uint32_t *rec) {
    constexpr int K = Curve<F>::NFP, RW = (COMP ? 12 : 24) * K;
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 24 * K; k++) any |= w[k];
    const bool inf = inf_flag || any == 0;
    Fp c[2 * K];                                                     // in byte order: x, then y; on Fq2 c1 before c0
#pragma unroll
    for (int j = 0; j < 2 * K; j++) abi_int(c[j], w + 12 * (K * (j / K) + (K == 2 ? 1 - j % K : 0)));
    bool high;
    if constexpr (K == 1) high = int_is_high(c[1]);
    else high = fp_int_is_zero(c[2]) ? int_is_high(c[3]) : int_is_high(c[2]);       // y.c1, or y.c0 when y.c1 = 0
#pragma unroll
    for (int j = 0; j < (COMP ? K : 2 * K); j++) { uint64_t u[6]; int_to_u64(u, c[j]); u64_to_be48(rec + 12 * j, u); }
    uint32_t top = (COMP ? FLAG_COMPRESSED : 0u) | (COMP && high ? FLAG_LARGEST : 0u);
    if (inf) {
#pragma unroll
        for (int k = 0; k < RW; k++) rec[k] = 0;
        top = (COMP ? FLAG_COMPRESSED : 0u) | FLAG_INF;
    }
    rec[0] |= bswap32(top);
}

// A resident base record (msm_kernels.hip.h, the MSM form of the curve: G1 -> G1S, G2 -> G2S) -> affine ABI words and the identity flag; an
// identity comes back as zero words.  The coordinates are the signed 30-bit field's Montgomery form (fp30s.hip.h) as fs_from_abi / the table
// construction's products left them (balanced digits).  G1: x[13] y[13] pad[2] flag pad[3]; G2: x.c0 x.c1 y.c0 y.c1 in slots of 14 words, flag
// in word 56.  dock_serde_dev.hip checks these numbers against msm::G1S / G2S.
template <class F> struct Rec;
template <> struct Rec<Fp> { static constexpr int WORDS = 32, SLOT = SN, FLAGW = 28; };
template <> struct Rec<Fp2> { static constexpr int WORDS = 64, SLOT = 14, FLAGW = 56; };
template <class F>
FD void record_to_abi(const uint32_t *rec, uint32_t *w, uint8_t *inf) {
    constexpr int K = Curve<F>::NFP;
    const bool id = rec[Rec<F>::FLAGW] != 0;
#pragma unroll
    for (int j = 0; j < 2 * K; j++) {
        Fs f;
#pragma unroll
        for (int i = 0; i < SN; i++) f.l[i] = (int32_t)rec[j * Rec<F>::SLOT + i];
        SCHK(schk_set_B(f, 1.0);)
        fs_to_abi(w + 12 * j, f);
    }
    if (id) {
#pragma unroll
        for (int k = 0; k < 24 * K; k++) w[k] = 0;
    }
    *inf = id ? 1 : 0;
}

#if defined(__HIPCC__)
constexpr int SERDE_BLOCK = 64;
// points [lo, hi) of `raw` (records of 12 / 24 NFP 32-bit words); the lowest refused index goes to *first_bad (atomic min; the caller sets it to ~0u)
template <class F, bool COMP>
__global__ void __launch_bounds__(SERDE_BLOCK) k_deserialize(const uint32_t *__restrict__ raw, size_t lo, size_t hi, int validate, uint32_t *__restrict__ xy,
                                                             uint8_t *__restrict__ is_inf, uint32_t *__restrict__ first_bad) {
    constexpr int K = Curve<F>::NFP, RW = (COMP ? 12 : 24) * K;
    const size_t i = lo + (size_t)blockIdx.x * SERDE_BLOCK + threadIdx.x;
    if (i >= hi) return;
    uint32_t rec[RW];
#pragma unroll
    for (int k = 0; k < RW; k += 4) { const uint4 v = *reinterpret_cast<const uint4 *>(raw + i * RW + k); rec[k] = v.x; rec[k + 1] = v.y; rec[k + 2] = v.z; rec[k + 3] = v.w; }
    uint32_t out[24 * K]; uint8_t inf = 0;
    if (decode_point<F, COMP>(rec, validate != 0, out, &inf)) {
#pragma unroll
        for (int k = 0; k < 24 * K; k += 4) *reinterpret_cast<uint4 *>(xy + i * 24 * K + k) = make_uint4(out[k], out[k + 1], out[k + 2], out[k + 3]);
        is_inf[i] = inf;
    } else {
        atomicMin(first_bad, (uint32_t)i);
    }
}
template <class F>
__global__ void __launch_bounds__(SERDE_BLOCK) k_validate_words(const uint32_t *__restrict__ xy, const uint8_t *__restrict__ is_inf, size_t lo, size_t hi, uint8_t *__restrict__ ok) {
    constexpr int K = Curve<F>::NFP;
    const size_t i = lo + (size_t)blockIdx.x * SERDE_BLOCK + threadIdx.x;
    if (i >= hi) return;
    uint32_t w[24 * K];
#pragma unroll
    for (int k = 0; k < 24 * K; k += 4) { const uint4 v = *reinterpret_cast<const uint4 *>(xy + i * 24 * K + k); w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w; }
    ok[i] = words_valid<F>(w, is_inf && is_inf[i]) ? 1 : 0;
}
// encoding: the ABI words of points [lo, hi) (is_inf may be null) -> their records in out (12 / 24 NFP words per point)
template <class F, bool COMP>
__global__ void __launch_bounds__(SERDE_BLOCK) k_serialize_words(const uint32_t *__restrict__ xy, const uint8_t *__restrict__ is_inf, size_t lo, size_t hi, uint32_t *__restrict__ out) {
    constexpr int K = Curve<F>::NFP, RW = (COMP ? 12 : 24) * K;
    const size_t i = lo + (size_t)blockIdx.x * SERDE_BLOCK + threadIdx.x;
    if (i >= hi) return;
    uint32_t w[24 * K], rec[RW];
#pragma unroll
    for (int k = 0; k < 24 * K; k += 4) { const uint4 v = *reinterpret_cast<const uint4 *>(xy + i * 24 * K + k); w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w; }
    encode_point<F, COMP>(w, is_inf && is_inf[i], rec);
#pragma unroll
    for (int k = 0; k < RW; k += 4) *reinterpret_cast<uint4 *>(out + i * RW + k) = make_uint4(rec[k], rec[k + 1], rec[k + 2], rec[k + 3]);
}
// resident base records of points [lo, hi) (recs: the first record of the range read) -> ABI words into xy and flags into is_inf (either may be
// null) when ENC = 0, else their records in out (ENC = 1 compressed, 2 uncompressed)
template <class F, int ENC>
__global__ void __launch_bounds__(SERDE_BLOCK) k_read_records(const uint32_t *__restrict__ recs, size_t lo, size_t hi, uint32_t *__restrict__ xy, uint8_t *__restrict__ is_inf,
                                                              uint32_t *__restrict__ out) {
    constexpr int K = Curve<F>::NFP, RW = (ENC == 1 ? 12 : 24) * K, RECW = Rec<F>::WORDS;
    const size_t i = lo + (size_t)blockIdx.x * SERDE_BLOCK + threadIdx.x;
    if (i >= hi) return;
    uint32_t r[RECW], w[24 * K]; uint8_t inf;
#pragma unroll
    for (int k = 0; k < RECW; k += 4) { const uint4 v = *reinterpret_cast<const uint4 *>(recs + i * RECW + k); r[k] = v.x; r[k + 1] = v.y; r[k + 2] = v.z; r[k + 3] = v.w; }
    record_to_abi<F>(r, w, &inf);
    if constexpr (ENC == 0) {
        if (xy) {
#pragma unroll
            for (int k = 0; k < 24 * K; k += 4) *reinterpret_cast<uint4 *>(xy + i * 24 * K + k) = make_uint4(w[k], w[k + 1], w[k + 2], w[k + 3]);
        }
        if (is_inf) is_inf[i] = inf;
    } else {
        uint32_t rec[RW];
        encode_point<F, ENC == 1>(w, inf != 0, rec);
#pragma unroll
        for (int k = 0; k < RW; k += 4) *reinterpret_cast<uint4 *>(out + i * RW + k) = make_uint4(rec[k], rec[k + 1], rec[k + 2], rec[k + 3]);
    }
}
#endif

}  // namespace serde
