// crypto_amd/csrc/gt_kernels.hip.h — batched Fp12 chains on the device: the tail of a segmented Miller loop and the final exponentiation,
// one element per GROUP of six lanes, host + device.
//
// dgpu_final_exponentiation runs hostf::final_exponentiation (host_field.hpp) on one core, ~0.27 ms per element; the verdict of every proof of a
// batch (dgpu_legogroth16_verify_each: the reference's verify_proof, legogroth16/src/verifier.rs:62-99, once per statement) needs one per proof, and
// the Miller loop of each proof its own 131-operation tail.  Thousands of independent elements are a throughput problem, so both chains run here.
//
// Layout.  An Fp12 is sum_e c_e w^e over Fp2 (w^6 = xi = 1 + u, w^2 = v): coefficient e = 2 j + i is the tower's c_i.c_j.  Lane e of a group holds
// c_e.  The per-step pieces are lane functions: lane e computes coefficient e of the result from the coefficients its group publishes into shared
// slots (GtLanes: LDS within ONE wave on the device — a group never straddles a wave, so no workgroup barrier; six host threads with a barrier in
// tests/native/gt_dev_host_shim.cpp, which runs this very code under the FP29_CHECK bound tracker).  Every lane executes the same instruction
// stream: what differs by lane is data (operand indices, selects), never control flow round an exchange.
//   product        lane e: sum_{s <= e} a_s b_{e-s} + xi sum_{s > e} a_s b_{e+6-s}        6 Fp2 products (schoolbook over w; 36 per element
//                  instead of Karatsuba's 18, but 6 deep instead of 18 deep)
//   cyclotomic sq. Granger-Scott as host_field.hpp: the pairs (c_j, c_{j+3}) are the Fq4 factors; lane j < 3 forms c_j^2 + xi c_{j+3}^2, lane
//                  j + 3 forms 2 c_j c_{j+3} (two Fp2 products each), then lane e combines 3 t +- 2 c_e
//   Frobenius      lane-local: c_e -> conj(c_e) g1[e] (p-power), c_e g2[e] (p^2-power), constants xi^(e (p - 1) / 6) and their norms
//   inverse        f^-1 = conj(f) / (f conj(f)); f conj(f) lies in Fp6 (even lanes), its inverse is ark-ff's Fp6::inverse spread over the lanes,
//                  one Fp2 inversion (fp_safegcd.hip.h) on every lane alike
// Everything is exact arithmetic on residues, so the results equal the host functions' word for word (GT and raw Miller outputs alike).
#pragma once
#include <stddef.h>
#include "pairing29.hip.h"
#include "fp_safegcd.hip.h"

namespace bls29 {

constexpr int GT_LANES = 6;
constexpr int GT_SLOTS = 2;       // shared Fp2 slots per group a step needs at once

// xi^(e (p - 1) / 6) (p-power Frobenius of w^e) and its norm (p^2-power), e = 0..5, in the Montgomery form of fp29.hip.h
#define GT_FROB1_TAB { {{0x3a9fb84u, 0xba00690u, 0x71288f1u, 0xf59bcc5u, 0x126cb614u, 0x585bf36u, 0x1b85ac3du, 0x1cf856fau, 0x1891ecbdu, 0x1a7eec05u, 0x155a88f0u, 0x741ac6du, 0x1317c30fu, 0x9u}, {0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u}}, {{0x1000a938u, 0x82633e3u, 0x19f1dadau, 0x14162cffu, 0x1caaaa9au, 0x13b1f614u, 0x11d37530u, 0x322a535u, 0xecf0fc0u, 0x13417b68u, 0x1433489fu, 0xbe62c9cu, 0x1257c722u, 0x2u}, {0xfff0173u, 0x7d1cc1cu, 0x1b0e2514u, 0x3e9d062u, 0x12b79750u, 0x159e8543u, 0x192a2792u, 0xd7bcb6cu, 0x895678bu, 0x1ed8e1feu, 0x1e93a14du, 0x719a097u, 0xdb95781u, 0xau}}, {{0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u}, {0x1195dfebu, 0x1b04e484u, 0x6026044u, 0x86070a2u, 0x1fd68858u, 0x137e9670u, 0x6871e67u, 0x1e736664u, 0x83b24f6u, 0x8a70373u, 0x2a012fdu, 0x112f94bu, 0x18a2733cu, 0x3u}}, {{0x16620abdu, 0x12fd467cu, 0xd1f4f6fu, 0x18780c70u, 0x3a0bc76u, 0x1c749a28u, 0x9efbfa9u, 0x91b1f3u, 0xe4ddb2au, 0x286f628u, 0xe8943au, 0x981f0b0u, 0xe14367cu, 0x0u}, {0x16620abdu, 0x12fd467cu, 0xd1f4f6fu, 0x18780c70u, 0x3a0bc76u, 0x1c749a28u, 0x9efbfa9u, 0x91b1f3u, 0xe4ddb2au, 0x286f628u, 0xe8943au, 0x981f0b0u, 0xe14367cu, 0x0u}}, {{0x154030c4u, 0x16aceb14u, 0x1814e947u, 0x1fba3004u, 0x2e0fc81u, 0xfb3da4fu, 0x170f2de1u, 0xacd4cbcu, 0x9689a69u, 0x110b9212u, 0x533b200u, 0x1554d884u, 0xba917a7u, 0x0u}, {0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u, 0x0u}}, {{0x662b3f5u, 0x1b237a60u, 0x7112a49u, 0xc8e3970u, 0x4b6711u, 0x1026903du, 0x1bc334dau, 0x3b45728u, 0x1d1ceaeau, 0x15c87190u, 0x151bdcd9u, 0x15681d4cu, 0x6bfd9eu, 0x3u}, {0x199cf6b6u, 0x14d4859fu, 0xdeed5a4u, 0xb71c3f2u, 0xf16dad9u, 0x1929eb1bu, 0xf3a67e8u, 0xcea1979u, 0x1a478c61u, 0x1c51ebd5u, 0x1dab0d13u, 0x1d97afe7u, 0x1fa52104u, 0x9u}}}
#define GT_FROB2_TAB { {0x3a9fb84u, 0xba00690u, 0x71288f1u, 0xf59bcc5u, 0x126cb614u, 0x585bf36u, 0x1b85ac3du, 0x1cf856fau, 0x1891ecbdu, 0x1a7eec05u, 0x155a88f0u, 0x741ac6du, 0x1317c30fu, 0x9u}, {0xe69cac0u, 0x14f31b7bu, 0xefd9fa9u, 0xf9f8cc0u, 0xf8bb992u, 0x15d1e4e7u, 0x4767e5bu, 0x122b0a3eu, 0xf295254u, 0x97359f3u, 0x1026d6f0u, 0x11ecd3e9u, 0x76eab67u, 0x9u}, {0xabf79e7u, 0x194b14ebu, 0x1ceb16a6u, 0x1845cd5du, 0xc814568u, 0x199ca109u, 0x13ee6ee1u, 0x5d123e5u, 0xdfbdce2u, 0x10ecb54u, 0xd9337edu, 0x1daaf4b0u, 0x146806fbu, 0xcu}, {0x1c55af27u, 0x457f96fu, 0xded76fdu, 0x8a6409du, 0x1cf58bd6u, 0x3cabc21u, 0xf77f086u, 0x13a619a7u, 0x1ed28a8du, 0x179b7160u, 0x1d6c60fcu, 0xbbe20c6u, 0xcf95b94u, 0x3u}, {0x1195dfebu, 0x1b04e484u, 0x6026044u, 0x86070a2u, 0x1fd68858u, 0x137e9670u, 0x6871e67u, 0x1e736664u, 0x83b24f6u, 0x8a70373u, 0x2a012fdu, 0x112f94bu, 0x18a2733cu, 0x3u}, {0x154030c4u, 0x16aceb14u, 0x1814e947u, 0x1fba3004u, 0x2e0fc81u, 0xfb3da4fu, 0x170f2de1u, 0xacd4cbcu, 0x9689a69u, 0x110b9212u, 0x533b200u, 0x1554d884u, 0xba917a7u, 0x0u}}

// tower index q (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2: the ABI order) of w-coefficient e, and back
FD int gt_tower_of(int e) { return (e & 1) ? 3 + (e >> 1) : (e >> 1); }

// r = a - k p for k = floor(top limb / 13.0021) (rounded down): class N in, fully carried limbs out, value < 2 p.  Values that leave a step
// are shrunk like this (~60 cheap instructions per Fp): the Granger-Scott combination 3 t +- 2 z would otherwise double the bound every squaring.
// a = sum l_i 2^(29 i) < (l_13 + 1) 2^377 and p > 13.0021 2^377 with 315 / 4096 < 1 / 13.0021, so 0 <= a - k p < (14.01 + l_13 / 2^13) 2^377 < 2 p.
FD void gt_shrink(Fp &r, const Fp &a) {
    BLS29_DECL_P;
    CHK(for (int i = 0; i < NL - 1; i++) assert(a.ub[i] <= (1ull << LB) + 7); assert(a.ub[NL - 1] < (1ull << 16)); chk_actual(a);)
    const uint32_t k = (a.l[NL - 1] * 315u) >> 12;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < NL - 1; i++) { const int64_t t = (int64_t)a.l[i] - (int64_t)k * P_[i] + c; r.l[i] = (uint32_t)t & LMASK; c = t >> LB; }
    r.l[NL - 1] = (uint32_t)((int64_t)a.l[NL - 1] - (int64_t)k * P_[NL - 1] + c);
    CHK(chk_set_N(r, 2.0); chk_actual(r);)
}
FD void gt_shrink(Fp2 &r, const Fp2 &a) { gt_shrink(r.c0, a.c0); gt_shrink(r.c1, a.c1); }
FD void gt_neg(Fp2 &r, const Fp2 &a) { Fp2 z; fzero(z); fsub<4>(r, z, a); fnorm(r, r); gt_shrink(r, r); }
// conjugation over Fp6 (w -> -w): the odd lanes negate.  Values between steps are class N with value < 2 p.
FD void gt_conj(Fp2 &r, const Fp2 &a, int e) { Fp2 n; gt_neg(n, a); fsel(r, (e & 1) != 0, n, a); }
// publish this lane's value in slot j and return the group's six
template <class X> FD const Fp2 *gt_share(X &x, int j, const Fp2 &v) { x.sync(); x.slot(j)[x.lane()] = v; x.sync(); return x.slot(j); }

// r = coefficient e of a b.  Inputs class N with value < 16 p; output class N, value < 2 p.
template <class X> FD void gt_mul(X &x, Fp2 &r, const Fp2 &a, const Fp2 &b) {
    const int e = x.lane();
    const Fp2 *A = gt_share(x, 0, a), *B = gt_share(x, 1, b);
    Fp2 lo, hi; fzero(lo); fzero(hi);
#pragma unroll 1
    for (int s = 0; s < GT_LANES; s++) {
        const int t = s <= e ? e - s : e + GT_LANES - s;
        const Fp2 as = A[s], bt = B[t];
        Fp2 m, nlo, nhi; fmul(m, as, bt);
        fadd(nlo, lo, m); fadd(nhi, hi, m);
        fsel(lo, s <= e, nlo, lo); fsel(hi, s > e, nhi, hi);
    }
    Fp2 xh, t; fnorm(hi, hi); f2_mul_xi_n<16>(xh, hi);
    fadd(t, lo, xh); fnorm(t, t); gt_shrink(r, t);
}
// Granger-Scott squaring of an element of the cyclotomic subgroup.  Input class N, value < 2 p.
template <class X> FD void gt_cyc_sqr(X &x, Fp2 &r, const Fp2 &z) {
    const int e = x.lane(), j = e % 3;
    const bool sq = e < 3;
    const Fp2 *Z = gt_share(x, 0, z);
    const Fp2 a = Z[j], b = Z[j + 3];
    Fp2 y1, x2, p1, p2, xp, t, tt;
    fsel(y1, sq, a, b); fsel(x2, sq, b, a);
    fmul(p1, a, y1); fmul(p2, x2, b);                     // lane j: a^2, b^2    lane j + 3: a b, a b
    f2_mul_xi_n<4>(xp, p2); fsel(p2, sq, xp, p2);
    fadd(t, p1, p2); fnorm(t, t);                         // a^2 + xi b^2  /  2 a b
    const Fp2 *T = gt_share(x, 1, t);
    const bool even = (e & 1) == 0;
    const int src = even ? (e >> 1) : 3 + ((e >> 1) + 2) % 3;
    Fp2 u = T[src], ux, zz, d, o;
    f2_mul_xi_n<8>(ux, u); fsel(u, e == 1, ux, u);         // c1.c0 takes xi t5
    gt_conj(zz, z, even ? 1 : 0);                         // even lanes: 3 t - 2 z, odd lanes: 3 t + 2 z
    fadd(d, u, zz); fnorm(d, d); fadd(o, d, d); fadd(o, o, u); fnorm(o, o); gt_shrink(r, o);
}
// p-power and p^2-power Frobenius (lane-local; the constant is picked by selects so that every lane runs the same code)
FD void gt_frob1(Fp2 &r, const Fp2 &a, int e) {
    constexpr uint32_t G[6][2][NL] = GT_FROB1_TAB;
    Fp2 g, c;
    for (int i = 0; i < NL; i++) { g.c0.l[i] = G[0][0][i]; g.c1.l[i] = G[0][1][i]; }
#pragma unroll
    for (int k = 1; k < 6; k++)
        for (int i = 0; i < NL; i++) { g.c0.l[i] = (k == e) ? G[k][0][i] : g.c0.l[i]; g.c1.l[i] = (k == e) ? G[k][1][i] : g.c1.l[i]; }
    CHK(chk_set_N(g.c0, 1.0); chk_set_N(g.c1, 1.0);)
    Fp z; fp_zero(z); c.c0 = a.c0; fp_sub<4>(c.c1, z, a.c1); fp_norm(c.c1, c.c1);
    fmul(r, c, g);
}
FD void gt_frob2(Fp2 &r, const Fp2 &a, int e) {
    constexpr uint32_t G[6][NL] = GT_FROB2_TAB;
    Fp g;
    for (int i = 0; i < NL; i++) g.l[i] = G[0][i];
#pragma unroll
    for (int k = 1; k < 6; k++)
        for (int i = 0; i < NL; i++) g.l[i] = (k == e) ? G[k][i] : g.l[i];
    CHK(chk_set_N(g, 1.0);)
    fmul_fp(r, a, g);
}
// 1 / (c0 + c1 u) = (c0 - c1 u) / (c0^2 + c1^2); 0 -> 0
FD void gt_f2_inv(Fp2 &r, const Fp2 &a) {
    Fp t, ti, n1, z;
    fp_mul2(t, a.c0, a.c0, a.c1, a.c1);
    fp_inv_safegcd(ti, t);
    fp_mul(r.c0, a.c0, ti);
    fp_mul(n1, a.c1, ti); fp_zero(z); fp_sub<4>(r.c1, z, n1); fp_norm(r.c1, r.c1);
}
// coefficient e of f^-1 (0 -> 0).  t = f conj(f) = c0^2 - v c1^2 is an Fp6 (even lanes: t0, t1, t2 at e = 0, 2, 4); ark-ff Fp6::inverse:
//   u0 = t0^2 - xi t1 t2,  u1 = xi t2^2 - t0 t1,  u2 = t1^2 - t0 t2,  n = t0 u0 + xi (t2 u1 + t1 u2),  t^-1 = (u0, u1, u2) / n
// lane e works on index j = e / 2 (lanes 2 j, 2 j + 1 alike; the odd one's copy is dropped), then f^-1 = conj(f) t^-1.
template <class X> FD void gt_inv(X &x, Fp2 &r, const Fp2 &f) {
    const int e = x.lane(), j = e >> 1;
    Fp2 cf, t; gt_conj(cf, f, e);
    gt_mul(x, t, f, cf);
    const Fp2 *T = gt_share(x, 0, t);
    const Fp2 t0 = T[0], t1 = T[2], t2 = T[4];
    Fp2 x1, x2, y2, p1, p2, q, u;
    fsel(x1, j == 0, t0, t1); fsel(x1, j == 1, t2, x1);                   // p1 = x1^2:  t0^2 | t2^2 | t1^2
    fsel(x2, j == 2, t0, t0); fsel(x2, j == 0, t1, x2);                   // p2 = x2 y2: t1 t2 | t0 t1 | t0 t2
    fsel(y2, j == 1, t1, t2);
    fmul(p1, x1, x1); fmul(p2, x2, y2);
    f2_mul_xi_n<4>(q, p1); fsel(p1, j == 1, q, p1);
    f2_mul_xi_n<4>(q, p2); fsel(p2, j == 0, q, p2);
    f2_sub_n<16>(u, p1, p2);
    const Fp2 *U = gt_share(x, 1, u);
    Fp2 w, m, nsum, n, ni, iv, zero, b;
    fsel(w, j == 0, t0, t1); fsel(w, j == 1, t2, w);                      // t0 u0 | t2 u1 | t1 u2
    fmul(m, w, u);
    const Fp2 *Q = gt_share(x, 0, m);
    fadd(nsum, Q[2], Q[4]); fnorm(nsum, nsum); f2_mul_xi_n<8>(n, nsum); fadd(n, n, Q[0]); fnorm(n, n);
    gt_f2_inv(ni, n);
    fmul(iv, U[2 * j], ni);
    fzero(zero); fsel(b, (e & 1) != 0, zero, iv);
    gt_mul(x, r, cf, b);
}
// a^|x| conjugated, i.e. a^x (x < 0), for a in the cyclotomic subgroup (host_field.hpp exp_by_x, starting at the top bit instead of at one)
template <class X> FD void gt_exp_by_x(X &x, Fp2 &r, const Fp2 &a) {
    Fp2 acc = a;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        gt_cyc_sqr(x, acc, acc);
        if ((BLS_X_ABS >> i) & 1) gt_mul(x, acc, acc, a);
    }
    gt_conj(r, acc, x.lane());
}
// ark-ec Bls12::final_exponentiation, step for step as hostf::final_exponentiation
template <class X> FD void gt_final_exp(X &x, Fp2 &out, const Fp2 &f) {
    const int e = x.lane();
    Fp2 f1, f2, r, y0, y1, y2, t;
    gt_conj(f1, f, e); gt_inv(x, f2, f); gt_mul(x, r, f1, f2); f2 = r;
    gt_frob2(t, r, e); gt_mul(x, r, t, f2);
    gt_cyc_sqr(x, y0, r); gt_exp_by_x(x, y1, r); gt_conj(y2, r, e);
    gt_mul(x, y1, y1, y2); gt_exp_by_x(x, y2, y1); gt_conj(y1, y1, e); gt_mul(x, y1, y1, y2);
    gt_exp_by_x(x, y2, y1); gt_frob1(t, y1, e); gt_mul(x, y1, t, y2); gt_mul(x, r, r, y0);
    gt_exp_by_x(x, y0, y1); gt_exp_by_x(x, y2, y0); gt_frob2(y0, y1, e); gt_conj(y1, y1, e);
    gt_mul(x, y1, y1, y2); gt_mul(x, y1, y1, y0); gt_mul(x, out, r, y1);
}
// the Miller-loop tail over the 68 per-step products: conj((...((L_0)^2 L_1)^2 ...)), the squaring before every doubling step but the first
// (dock_pairing.hip MlTail).  load(s, c) returns coefficient e of L_s.
template <class X, class Load> FD void gt_miller_tail(X &x, Fp2 &out, const Load &load) {
    Fp2 f, l;
    int idx = 0;
    load(idx++, f);
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        if (b != 62) { gt_mul(x, f, f, f); load(idx++, l); gt_mul(x, f, f, l); }
        if ((BLS_X_ABS >> b) & 1) { load(idx++, l); gt_mul(x, f, f, l); }
    }
    gt_conj(out, f, x.lane());
}

// ---- powers, products of powers and membership (k_gt_pow.hip; `PairingOutput::mul_bigint` and `Valid::check` over many elements) ----
// Between kernels and inside a kernel's table an element lives in the INTERNAL form: coefficient e as 2 NL limbs (class N, value < 2 p: what gt_mul
// and gt_cyc_sqr leave) at word e GT_TABW of its GT_ELW words.  Lane e stores and loads coefficient e only.
constexpr int GT_TABW = 2 * NL;                   // words of one coefficient
constexpr int GT_ELW = GT_LANES * GT_TABW;        // words of one element
constexpr int GT_ABIW = 144;                      // words of one element in the ABI form (72 u64)
constexpr int GT_TAB = 8;                         // table entries per base: a^1 .. a^8
constexpr int GT_MAX_K = 8;                       // bases per group
constexpr int GT_FOLD = 8;                        // inputs per group of a fold level

FD void gt_put(uint32_t *dst, const Fp2 &v) {
    CHK(assert(v.c0.vb <= 2.0 && v.c1.vb <= 2.0); for (int i = 0; i < NL - 1; i++) assert(v.c0.ub[i] <= (1ull << LB) + 7 && v.c1.ub[i] <= (1ull << LB) + 7);)
#pragma unroll
    for (int i = 0; i < NL; i++) { dst[i] = v.c0.l[i]; dst[NL + i] = v.c1.l[i]; }
}
FD void gt_get(Fp2 &v, const uint32_t *src) {
#pragma unroll
    for (int i = 0; i < NL; i++) { v.c0.l[i] = src[i]; v.c1.l[i] = src[NL + i]; }
    CHK(chk_set_N(v.c0, 2.0); chk_set_N(v.c1, 2.0); chk_actual(v.c0); chk_actual(v.c1);)
}
// coefficient e of an element in the ABI form (tower order, 12 words per Fp)
FD void gt_get_abi(Fp2 &v, const uint32_t *el, int e) {
    const uint32_t *src = el + gt_tower_of(e) * 24;
    uint32_t w[24];
#pragma unroll
    for (int k = 0; k < 24; k++) w[k] = src[k];
    fp_from_abi(v.c0, w); fp_from_abi(v.c1, w + 12);
}
FD void gt_put_abi(uint32_t *el, int e, const Fp2 &v) {
    uint32_t *dst = el + gt_tower_of(e) * 24;
    uint32_t w[24]; fp_to_abi(w, v.c0); fp_to_abi(w + 12, v.c1);
#pragma unroll
    for (int k = 0; k < 24; k++) dst[k] = w[k];
}
// coefficient e of the element one
FD void gt_one(Fp2 &r, int e) { Fp2 o, z; fset_one(o); fzero(z); fsel(r, e == 0, o, z); }
// r = c ? a : b where c depends on the DATA (a digit, a bit of an exponent): the check build keeps the wider of the two bounds
FD void gt_sel_data(Fp2 &r, bool c, const Fp2 &a, const Fp2 &b) {
    fsel(r, c, a, b);
    CHK(for (int i = 0; i < NL; i++) { r.c0.ub[i] = a.c0.ub[i] > b.c0.ub[i] ? a.c0.ub[i] : b.c0.ub[i]; r.c1.ub[i] = a.c1.ub[i] > b.c1.ub[i] ? a.c1.ub[i] : b.c1.ub[i]; }
        r.c0.vb = a.c0.vb > b.c0.vb ? a.c0.vb : b.c0.vb; r.c1.vb = a.c1.vb > b.c1.vb ? a.c1.vb : b.c1.vb;)
}

// Signed 4-bit digits of a 256-bit exponent (eight 32-bit words), d_w in [-7, 8], w = 0 .. 64, sum d_w 16^w = the exponent: the rule of
// signed_digits in dock_gt.cpp (v = nibble + carry; v > 8 gives v - 16 and a carry), digit 64 the carry out of bit 255.  A lane keeps the 64
// carries as one word (bit w = the carry OUT of window w) and forms a digit from the exponent word that holds its nibble.
FD uint64_t gt_digit_carries(const uint32_t e[8]) {
    uint64_t m = 0; uint32_t c = 0;
#pragma unroll 1
    for (int w = 0; w < 64; w++) { const uint32_t v = ((e[w >> 3] >> (4 * (w & 7))) & 15u) + c; c = v > 8 ? 1u : 0u; m |= (uint64_t)c << w; }
    return m;
}
FD int gt_digit(uint32_t word, uint64_t carries, int w) {       // word = exponent word w / 8 (anything for w = 64)
    const int nib = w < 64 ? (int)((word >> (4 * (w & 7))) & 15u) : 0;
    const int cin = w > 0 ? (int)((carries >> (w - 1)) & 1) : 0, cout = w < 64 ? (int)((carries >> w) & 1) : 0;
    return nib + cin - 16 * cout;
}
FD void gt_signed_digits(const uint32_t e[8], int8_t d[65]) {
    const uint64_t m = gt_digit_carries(e);
    for (int w = 0; w <= 64; w++) d[w] = (int8_t)gt_digit(e[w < 64 ? w >> 3 : 7], m, w);
}

// words of a and b in the ABI form compared: 0 iff a == b as residues.  (Values between steps are lazy residues: never compare those.)
FD uint32_t gt_abi_diff(const Fp2 &a, const Fp2 &b, uint32_t &any_b) {
    uint32_t wa[12], wb[12], d = 0;
    fp_to_abi(wa, a.c0); fp_to_abi(wb, b.c0);
#pragma unroll
    for (int k = 0; k < 12; k++) { d |= wa[k] ^ wb[k]; any_b |= wb[k]; }
    fp_to_abi(wa, a.c1); fp_to_abi(wb, b.c1);
#pragma unroll
    for (int k = 0; k < 12; k++) { d |= wa[k] ^ wb[k]; any_b |= wb[k]; }
    return d;
}
// f in the cyclotomic subgroup (in_cyclotomic of dock_gt.cpp): f^(p^4) f == f^(p^2), zero is not
template <class X> FD bool gt_in_cyclotomic(X &x, const Fp2 &f) {
    const int e = x.lane();
    Fp2 f2, f4, l; gt_frob2(f2, f, e); gt_frob2(f4, f2, e); gt_mul(x, l, f4, f);
    uint32_t any = 0;
    const uint32_t diff = gt_abi_diff(l, f2, any);
    const bool eq = x.all(diff == 0), zero = x.all(any == 0);          // (f^(p^2) is zero iff f is)
    return eq && !zero;
}
// f in GT (in_gt of dock_gt.cpp): in the cyclotomic subgroup and f^p == f^x.  Every lane runs the whole chain whatever the first test said.
template <class X> FD bool gt_in_gt(X &x, const Fp2 &f) {
    const bool cyc = gt_in_cyclotomic(x, f);
    Fp2 l, r; gt_frob1(l, f, x.lane()); gt_exp_by_x(x, r, f);
    uint32_t any = 0;
    const uint32_t diff = gt_abi_diff(l, r, any);
    return x.all(diff == 0) && cyc;
}

// tab[d - 1] = a^d, d = 1 .. 8, for a in the cyclotomic subgroup; entry 0 is already there.  `tab` is this lane's column of the base's table
// (entries GT_ELW words apart).  Seven steps: even d squares entry d / 2, odd d multiplies the entry before by a.
template <class X> FD void gt_pow_table(X &x, uint32_t *tab) {
    Fp2 a, cur; gt_get(a, tab); cur = a;
#pragma unroll 1
    for (int d = 2; d <= GT_TAB; d++) {
        if (d & 1) gt_mul(x, cur, cur, a);                               // (d is the same on every lane)
        else { Fp2 h; gt_get(h, tab + (d / 2 - 1) * GT_ELW); gt_cyc_sqr(x, cur, h); }
        gt_put(tab + (d - 1) * GT_ELW, cur);
    }
}
// acc = prod_j a_j^(e_j) over the k bases of a group, all of the cyclotomic subgroup, by signed 4-bit windows from the top: four Granger-Scott
// squarings shared by the group's bases, then per base ONE product by an operand picked by selects — the table entry of |d|, conjugated for d < 0,
// the element one for d = 0 — so every lane of a wave runs the same stream whatever the digits are (no `started` flag: the accumulator starts
// at one, and squaring one is harmless).  tab: this lane's column of the group's tables (base j at j GT_TAB GT_ELW); dig(j, w) = digit w of base j.
template <class X, class Dig> FD void gt_pow_cyc(X &x, Fp2 &acc, const uint32_t *tab, int k, const Dig &dig) {
    const int e = x.lane();
    Fp2 one; gt_one(one, e);
    acc = one;
#pragma unroll 1
    for (int w = 64; w >= 0; w--) {
#pragma unroll 1
        for (int s = 0; s < 4; s++) gt_cyc_sqr(x, acc, acc);
#pragma unroll 1
        for (int j = 0; j < k; j++) {
            const int d = dig(j, w), m = d < 0 ? -d : d;
            Fp2 tv, tc, op; gt_get(tv, tab + ((size_t)j * GT_TAB + (m ? m - 1 : 0)) * GT_ELW);
            gt_conj(tc, tv, e);
            gt_sel_data(op, d < 0, tc, tv); gt_sel_data(op, d == 0, one, op);
            gt_mul(x, acc, acc, op);
        }
    }
}
// the same product for ANY Fp12 bases (untrusted input, raw Miller outputs, zero): binary square-and-multiply from the top bit, the square a
// plain product, the multiplier a select between the base (entry 0 of its table) and one.  0^0 = one and 0^e = 0 fall out of it.
template <class X, class Bit> FD void gt_pow_generic(X &x, Fp2 &acc, const uint32_t *tab, int k, const Bit &bit) {
    Fp2 one; gt_one(one, x.lane());
    acc = one;
#pragma unroll 1
    for (int b = 255; b >= 0; b--) {
        gt_mul(x, acc, acc, acc);
#pragma unroll 1
        for (int j = 0; j < k; j++) {
            Fp2 a, op; gt_get(a, tab + (size_t)j * GT_TAB * GT_ELW);
            gt_sel_data(op, bit(j, b), a, one);
            gt_mul(x, acc, acc, op);
        }
    }
}

// What one group of k_gt_pow does: the product of the powers of bases [first, first + k) of nb (ABI form, `in`; missing ones count as one), exponent
// of base b at exps + b ew (ew = 8 words, or 0 for one exponent for all), into dst (this group's element, ABI or internal form).
// tab: the group's k tables; cm: k words of this lane's own (carries of the digits), cs apart.
// The short path needs every base of every group of the WAVE in the cyclotomic subgroup (x.wave_all: the branch is the same on every lane of the
// wave, so the lock step of the exchanges holds); otherwise the whole wave runs the generic one.  Both are exact, so the words are the same.
// force_generic: tests only.
template <class X> FD void gt_pow_group(X &x, const uint32_t *in, const uint32_t *exps, int ew, size_t nb, size_t first, int k, uint32_t *tab,
                                        uint64_t *cm, int cs, bool force_generic, uint32_t *dst, bool dst_abi) {
    const int e = x.lane();
    uint32_t *mytab = tab + e * GT_TABW;
    bool cyc = true;
#pragma unroll 1
    for (int j = 0; j < k; j++) {
        const bool valid = first + j < nb;
        const size_t b = valid ? first + j : nb - 1;
        Fp2 a, one; gt_get_abi(a, in + b * GT_ABIW, e); gt_one(one, e);
        gt_sel_data(a, valid, a, one);
        gt_put(mytab + (size_t)j * GT_TAB * GT_ELW, a);
        const bool c = gt_in_cyclotomic(x, a);
        cyc = cyc && c;
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = exps[b * ew + i];
        const uint64_t m = gt_digit_carries(w);
        cm[j * cs] = valid ? m : 0;
    }
    const bool use_cyc = x.wave_all(cyc) && !force_generic;
    auto word = [&](int j, int wi) -> uint32_t { const bool valid = first + j < nb; return valid ? exps[(first + j) * ew + wi] : 0u; };
    Fp2 acc;
    if (use_cyc) {
#pragma unroll 1
        for (int j = 0; j < k; j++) gt_pow_table(x, mytab + (size_t)j * GT_TAB * GT_ELW);
        gt_pow_cyc(x, acc, mytab, k, [&](int j, int w) { return gt_digit(word(j, w < 64 ? w >> 3 : 7), cm[j * cs], w); });
    } else {
        gt_pow_generic(x, acc, mytab, k, [&](int j, int b) { return ((word(j, b >> 5) >> (b & 31)) & 1u) != 0; });
    }
    if (dst_abi) gt_put_abi(dst, e, acc); else gt_put(dst + e * GT_TABW, acc);
}
// What one group of k_gt_fold does: the product of inputs [first, first + GT_FOLD) of n_in (a missing one counts as one; a lone input is copied)
template <class X> FD void gt_fold_group(X &x, const uint32_t *in, bool in_abi, size_t n_in, size_t first, uint32_t *dst, bool dst_abi) {
    const int e = x.lane();
    Fp2 acc, one; gt_one(one, e);
    auto get = [&](Fp2 &v, size_t idx) { if (in_abi) gt_get_abi(v, in + idx * GT_ABIW, e); else gt_get(v, in + idx * GT_ELW + e * GT_TABW); };
    get(acc, first);
#pragma unroll 1
    for (int s = 1; s < GT_FOLD; s++) {
        const bool valid = first + s < n_in;
        Fp2 v; get(v, valid ? first + s : first);
        gt_sel_data(v, valid, v, one);
        gt_mul(x, acc, acc, v);
    }
    if (dst_abi) gt_put_abi(dst, e, acc); else gt_put(dst + e * GT_TABW, acc);
}

}  // namespace bls29
