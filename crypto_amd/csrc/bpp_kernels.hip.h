// crypto_amd/csrc/bpp_kernels.hip.h — the scalar and staging half of verifying Bulletproofs++ range proofs in bulk on gfx950 (dock_bpp.hip drives it).
//
// Device side of bulletproofs_plus_plus's Proof::verify (range_proof.rs:773-873) over WeightedNormLinearArgument::verify_given_commitment_multiplicands
// (weighted_norm_linear_argument.rs:213-238, :380-453) for many proofs of ONE shape (base, num_bits, m values) over ONE setup [G, H_0 .. H_7, G_0 .. G_(NG-1)].
// bb = log2 base, dp = num_bits / bb digits a value, D = dp m digits, NG = max(dp, base) m, lg = log2 NG, K = max(3, lg) rounds.  A proof is the points
// V_0 .. V_(m-1), D, M, R, S, X_0 .. X_(K-1), R_0 .. R_(K-1), the scalars l0, n0 and the challenges e, x, y, r, lambda, delta, t, gamma_0 .. gamma_(K-1); q = r^2.
// It verifies iff ONE sum of 9 + NG shared and m + 4 + 2 K own terms is the identity:
//   slot 0            G     v - g_off          v = l0 <c, hm> + n0^2 r^(2 NG),  c = y (1/t, t, t^2, t^3, t^5, t^6, t^7, 0)
//   slot 1 + k        H_k   l0 hm_k            hm_k = prod_{j < 3, bit j of k} gamma_j
//   slot 9 + k        G_k   n0 gm_k - pub_k    gm_k = prod_{j < lg} (bit j of k ? gamma_j : r^(2^j))
//                                              pub_k = [k < D] (t^2 ad_k q^-(k+1) + t (e - x delta q^-(k+1))) + [k < base] t^3 x q^-(k+1) / (e + k)
//                                              ad_k = lambda^(k div dp) base^(k mod dp)
//   own               V_k: -2 t^3 lambda^k;  D: -t;  M: -delta;  R: -t^2;  S: -1/t;  X_j: -gamma_j;  R_j: -(gamma_j^2 - 1)
//   g_off = 2 t^3 (sum_{k < D} q^(k+1) + e sum_{k < D} ad_k - x delta sum_{k < D} ad_k q^-(k+1))
// The scalar field has to
//   per proof: the inverses (ONE fr_inv: fr_batch_inv over t, q, e + 0 .. e + base - 1), the powers, v, g_off, the own scalars, a record for the lanes below,
//   and the flag "an inverse does not exist" (status 2)                                                                     k_bpp_consts
//   per (proof, shared slot): the row's canonical scalar where the many-row MSM reads it                                    k_bpp_shared
//   one verdict: proof i of the batch weighs rho^i: the coefficients of the 9 + NG shared points, the own scalars times rho^i   k_bpp_col_sums, k_col_finish
// and two kernels move words only: k_bpp_stage lays a proof's own points and its P_i = <row_i, setup> out for the segment MSM, k_bpp_verdict makes the status
// byte.  The per-lane routines are FRD functions over load / store functors, as smc_kernels.hip.h's are: the same text runs on the host under -DFP29_CHECK
// (tests/native/bpp_dev_host_shim.cpp).  Operand classes as in col_sums.hip.h: "product" (limbs < 2^29, value < 2 r), "lazy sum" (one carry pass after
// every addition of a product).
//
// g_off's three sums over D <= 512 digits factor, because digit k = i dp + j carries lambda^i base^j q^+-(i dp + j + 1):
//   sum_k q^(k+1) = (sum_{i<m} (q^dp)^i) (sum_{j<dp} q^(j+1)),  sum_k ad_k = (sum_i lambda^i) (sum_j base^j),
//   sum_k ad_k q^-(k+1) = (sum_i (lambda q^-dp)^i) (sum_j base^j q^-(j+1))
// so a proof's lane adds dp + m <= 72 terms a sum, not 512, and g_off stays a serial pass of k_bpp_consts: about 5 (dp + m) products, fewer than the
// inversion's 431.  q^dp and q^-dp are the last powers of the inner loop.
//
// Bounds.  Every lazy sum below takes one carry pass after each addition, so its limbs stay <= 2^29 + 1 below the top one:
//   <c, hm>                 7 products                     value < 14 r      first operand of the product with y
//   the inner sums of g_off dp <= 64 products              value < 128 r     reduced by a product with one
//   the outer sums of g_off m <= 8 products                value < 16 r      first operand of the product with the inner sum
//   v                       2 products                     value < 4 r       the minuend of fr_sub<512, 30> (limbs < 2^30)
//   pub_k                   3 products                     value < 6 r       reduced by a product with one before it is subtracted
//   e + k                   a product plus one             value < 4 r       reduced by a product with one
// Every difference a - b is fr_sub<512, 30> (a: limbs < 2^30; b: a product; result: limbs < 2^31, value < value(a) + 512 r), at once the first operand of a
// product.  The batch's column sums are col_sums.hip.h's col_run / tree_step / col_finish with their bounds (a lane's run of COL_RUN = 16 proofs, a
// block's fixed tree: value < 2^13 r).  q^-(k+1) is the product of at most lg + 1 <= 10 entries of the proof's table of squarings (binary expansion of k + 1):
// at most 9 products a lane beside gm_k's 9, against 2 lg for a square-and-multiply of its own or NG serial products in the proof's lane for a full table.
#pragma once
#include "col_sums.hip.h"

namespace bppk {
using namespace fr29;
using colk::neg_product;

constexpr int FQW = 12;           // u32 words of a base-field element
constexpr int NH = 8;             // |H_vec|
constexpr int SHARED0 = 1 + NH;   // shared slots in front of the G_k
constexpr int MAX_K = 9, MAX_M = 8, MAX_BASE = 16;
constexpr int N_CHAL = 7;         // challenges in front of the gammas: e, x, y, r, lambda, delta, t
// the shape of a statement
struct Shape { int base, bb, dp, m, D, NG, lg, K, own; };      // own = m + 4 + 2 K own points a proof
FRD int log2u(unsigned v) { int l = 0; while ((1u << (l + 1)) <= v) l++; return l; }
FRD bool pow2(unsigned v) { return v && !(v & (v - 1)); }
FRD Shape make_shape(unsigned base, unsigned num_bits, unsigned m) {
    Shape s;
    s.base = (int)base; s.bb = log2u(base); s.dp = (int)num_bits / s.bb; s.m = (int)m; s.D = s.dp * s.m;
    s.NG = (s.dp > s.base ? s.dp : s.base) * s.m; s.lg = log2u((unsigned)s.NG); s.K = s.lg > 3 ? s.lg : 3; s.own = s.m + 4 + 2 * s.K;
    return s;
}
// base in {2, 4, 8, 16}, num_bits a power of two in [bb, 64], m a power of two in [1, 8].  Base 8 has dp = num_bits / 3 rounded down, as the reference's u16
// division has; where that leaves an NG that is no power of two (num_bits >= 32) the reference's argument refuses to be built, and so does the shape here
FRD bool shape_ok(unsigned base, unsigned num_bits, unsigned m) {
    if (base != 2 && base != 4 && base != 8 && base != 16) return false;
    if (!pow2(num_bits) || num_bits > 64 || num_bits < (unsigned)log2u(base)) return false;
    if (!pow2(m) || m > (unsigned)MAX_M) return false;
    return pow2((unsigned)make_shape(base, num_bits, m).NG);
}

// ---- the per-proof record: Fr values in the internal form, entry `idx` of proof i (the kernels keep it entry-major: lanes of neighbouring proofs read
// neighbouring words) ----
enum Rec {
    R_L0 = 0, R_N0, R_T, R_T2, R_T3X, R_E, R_XD, R_S0,       // l0, n0, t, t^2, t^3 x, e, x delta, v - g_off
    R_GAM = 8,                                               // gamma_j, j < K <= 9
    R_RSQ = R_GAM + MAX_K,                                   // r^(2^j), j <= lg + 1 <= 10  (j = 1: q; j = lg + 1: r^(2 NG))
    R_QIP = R_RSQ + MAX_K + 2,                               // q^-(2^j), j <= lg <= 9
    R_LAM = R_QIP + MAX_K + 1,                               // lambda^i, i < m <= 8
    R_EIN = R_LAM + MAX_M,                                   // t^3 x / (e + k), k < base <= 16
    R_INV = R_EIN + MAX_BASE,                                // 1/t, 1/q, 1/(e + k): the outputs of the batch inversion (its prefix products in between)
    R_ELT = R_INV + 2 + MAX_BASE,                            // t, q, e + k: its inputs (one in the place of a zero)
    R_V = R_ELT + 2 + MAX_BASE, R_2T3,                       // between the stages of bpp_consts: l0 <c, hm>, then v; 2 t^3
    REC_N
};

FRD bool is_zero_product(const Fr &a) {
    uint32_t w[8], o = 0;
    fr_to_words(w, a, false);
    for (int i = 0; i < 8; i++) o |= w[i];
    return o == 0;
}
// sum += a b, one carry pass.  a, b: products
FRD void add_product(Fr &sum, const Fr &a, const Fr &b) {
    Fr p; fr_mul(p, a, b);                            // 2 r * 2 r
    fr_add(sum, sum, p); fr_norm(sum, sum);
}
// sum += a, one carry pass.  a: a product
FRD void add_term(Fr &sum, const Fr &a) { fr_add(sum, sum, a); fr_norm(sum, sum); }
// o = a - b as a product.  a: limbs < 2^30 (a product, or a lazy sum of a few); b: a product
FRD void sub_product(Fr &o, const Fr &a, const Fr &b) {
    Fr d, one; fr_one(one);
    fr_sub<512, 30>(d, a, b);
    fr_mul(o, d, one);                                // (value(a) + 512 r) * r
}
// p = b^e by square and multiply over a product b (e = 0: one)
FRD void pow_small(Fr &p, const Fr &b0, unsigned e) {
    Fr b = b0; fr_one(p);
    for (; e; e >>= 1) { if (e & 1) fr_mul(p, p, b); if (e > 1) fr_mul(b, b, b); }
}

// Everything of one proof that does not depend on the slot.  in(k, Fr &): challenge k (0 e, 1 x, 2 y, 3 r, 4 lambda, 5 delta, 6 t, 7 + j gamma_j); ln(k, Fr &):
// 0 l0, 1 n0 — both load products.  rl(idx, Fr &) / rs(idx, const Fr &): the proof's record.  os(slot, const Fr &): own scalar `slot` < own (a product), in the
// order V_0 .., D, M, R, S, X_0 .., R_0 ..; with one_behind also slot `own` = one (the scalar of P_i in the proof's segment).  Returns the status-2 flag: one
// of t, r, e + k (k < base) is zero — the record and the own scalars are then those of a proof whose zero was one, and nobody looks at them.
template <class In, class LN, class RL, class RS, class OS> FRD bool bpp_consts(const Shape &s, bool one_behind, In in, LN ln, RL rl, RS rs, OS os) {
    // The work goes in stages that hand their results on through the record, not through registers: a stage keeps a dozen values alive, the whole routine
    // would keep some thirty (300 registers of limbs)
    Fr one;
    fr_one(one);
    bool bad;
    {   // the inverses: ONE fr_inv over t, q, e + 0 .. e + base - 1
        Fr e, r, t, q, a, b;
        in(0, e); in(3, r); in(6, t);
        fr_mul(q, r, r);
        const bool t_zero = is_zero_product(t), r_zero = is_zero_product(r);
        bad = t_zero || r_zero;
        rs(R_ELT, t_zero ? one : t); rs(R_ELT + 1, r_zero ? one : q);
        a = e;
        for (int k = 0; k < s.base; k++) {
            const bool z = is_zero_product(a);
            bad = bad || z;
            rs(R_ELT + 2 + k, z ? one : a);
            fr_add(b, a, one); fr_norm(b, b); fr_mul(a, b, one);      // 4 r * r
        }
        fr_batch_inv((size_t)(2 + s.base), [&](size_t k, Fr &v) { rl(R_ELT + (int)k, v); }, [&](size_t k, Fr &v) { rl(R_INV + (int)k, v); },
                     [&](size_t k, const Fr &v) { rs(R_INV + (int)k, v); });
        rs(R_E, e); rs(R_T, t);
        // r^(2^j): j < lg the factors of gm_k, j = 1 is q, j = lg + 1 the weight mu of the norm
        a = r;
        for (int j = 0; j <= s.lg + 1; j++) { rs(R_RSQ + j, a); fr_mul(a, a, a); }
    }
    {   // the powers of t, <c, hm> and what hangs on them
        Fr t, tinv, t2, t3, tp, a, b, c, g0, g1, g2;
        rl(R_T, t); rl(R_INV, tinv);
        fr_mul(t2, t, t); fr_mul(t3, t2, t);
        in(N_CHAL, g0); in(N_CHAL + 1, g1); in(N_CHAL + 2, g2);
        // <c, hm> = y (1/t + t g0 + t^2 g1 + t^3 g0 g1 + t^5 g2 + t^6 g0 g2 + t^7 g1 g2)   (c_7 = 0)
        fr_zero(c);
        add_term(c, tinv); add_product(c, t, g0); add_product(c, t2, g1);
        fr_mul(a, g0, g1); add_product(c, t3, a);
        fr_mul(tp, t3, t2); add_product(c, tp, g2);                   // t^5
        fr_mul(tp, t3, t3); fr_mul(a, g0, g2); add_product(c, tp, a); // t^6
        fr_mul(tp, tp, t); fr_mul(a, g1, g2); add_product(c, tp, a);  // t^7
        in(2, a); fr_mul(c, c, a);                        // 14 r * 2 r
        ln(0, a); rs(R_L0, a); fr_mul(c, a, c); rs(R_V, c);           // l0 <c, hm>
        rs(R_T2, t2);
        fr_add(a, t3, t3); fr_norm(a, a); fr_mul(b, a, one); rs(R_2T3, b);      // 4 r * r
        in(1, a); fr_mul(t3, t3, a); rs(R_T3X, t3);                   // t^3 x
        in(5, b); fr_mul(a, a, b); rs(R_XD, a);                       // x delta
        neg_product(a, t); os(s.m, a);
        neg_product(a, b); os(s.m + 1, a);
        neg_product(a, t2); os(s.m + 2, a);
        neg_product(a, tinv); os(s.m + 3, a);
    }
    {   // the tables of the lanes of k_bpp_shared; v = l0 <c, hm> + n0^2 mu
        Fr a, b, c;
        rl(R_INV + 1, a);
        for (int j = 0; j <= s.lg; j++) { rs(R_QIP + j, a); fr_mul(a, a, a); }
        in(4, b);
        a = one;
        for (int i = 0; i < s.m; i++) { rs(R_LAM + i, a); fr_mul(a, a, b); }
        rl(R_T3X, b);
        for (int k = 0; k < s.base; k++) { rl(R_INV + 2 + k, a); fr_mul(a, a, b); rs(R_EIN + k, a); }
        ln(1, a); rs(R_N0, a);
        fr_mul(a, a, a); rl(R_RSQ + s.lg + 1, b); fr_mul(a, a, b);
        rl(R_V, c);
        fr_add(c, c, a); fr_norm(c, c);                   // v < 4 r
        rs(R_V, c);
    }
    {   // g_off: the inner sums over the digits of one value, the outer ones over the values; slot 0 = v - g_off
        Fr a, b, c, d, q, qinv, bf, qp, qip, bp, s1, s2, s3;
        rl(R_RSQ + 1, q); rl(R_INV + 1, qinv);
        fr_add(a, one, one); fr_norm(a, a); fr_mul(bf, a, one);       // two
        { Fr two = bf; for (int i = 1; i < s.bb; i++) fr_mul(bf, bf, two); }      // base
        qp = q; qip = qinv; bp = one;
        fr_zero(s1); fr_zero(s2); fr_zero(s3);
        for (int j = 0; j < s.dp; j++) {
            add_term(s1, qp); add_term(s2, bp); add_product(s3, bp, qip);
            if (j + 1 == s.dp) break;
            fr_mul(qp, qp, q); fr_mul(qip, qip, qinv); fr_mul(bp, bp, bf);
        }
        // (qp, qip: q^dp and q^-dp, the last powers of the loop)
        fr_mul(s1, s1, one); fr_mul(s2, s2, one); fr_mul(s3, s3, one);            // 128 r * r
        Fr &lam = q, &lq = qinv, &u1 = bf, &u2 = bp;      // (q, qinv, base and its powers are done with)
        Fr u3, o1, o2, o3;
        in(4, lam);
        fr_mul(lq, lam, qip);
        u1 = one; u2 = one; u3 = one;
        fr_zero(o1); fr_zero(o2); fr_zero(o3);
        for (int i = 0; i < s.m; i++) {
            add_term(o1, u1); add_term(o2, u2); add_term(o3, u3);
            if (i + 1 == s.m) break;
            fr_mul(u1, u1, qp); fr_mul(u2, u2, lam); fr_mul(u3, u3, lq);
        }
        fr_mul(s1, o1, s1); fr_mul(s2, o2, s2); fr_mul(s3, o3, s3);               // 16 r * 2 r
        rl(R_E, a); fr_mul(a, a, s2);
        rl(R_XD, b); fr_mul(b, b, s3);
        fr_add(c, s1, a); fr_norm(c, c);                  // < 4 r
        fr_sub<512, 30>(d, c, b);
        rl(R_2T3, b); fr_mul(a, d, b);                    // g_off: 516 r * 2 r
        rl(R_V, c);
        sub_product(b, c, a);
        rs(R_S0, b);
    }
    {   // the own scalars over V, X, R
        Fr a, b, c;
        rl(R_2T3, c);
        for (int k = 0; k < s.m; k++) { rl(R_LAM + k, a); fr_mul(a, a, c); neg_product(b, a); os(k, b); }
        for (int j = 0; j < s.K; j++) {
            in(N_CHAL + j, a);
            rs(R_GAM + j, a);
            neg_product(b, a); os(s.m + 4 + j, b);
            fr_mul(c, a, a);
            sub_product(b, one, c); os(s.m + 4 + s.K + j, b);         // -(gamma^2 - 1)
        }
        if (one_behind) os(s.own, one);
    }
    return bad;
}

// The scalar of shared slot `slot` < 9 + NG of a proof, as a product.  rl(idx, Fr &): the proof's record
template <class RL> FRD void bpp_shared(const Shape &s, unsigned slot, RL rl, Fr &o) {
    Fr g, one;
    fr_one(one);
    if (slot == 0) { rl(R_S0, o); return; }
    if (slot < (unsigned)SHARED0) {
        const unsigned k = slot - 1;
        rl(R_L0, o);
        for (int j = 0; j < 3; j++) if (k >> j & 1) { rl(R_GAM + j, g); fr_mul(o, o, g); }
        return;
    }
    const unsigned k = slot - (unsigned)SHARED0;
    rl(R_N0, o);
    for (int j = 0; j < s.lg; j++) { rl((k >> j & 1) ? R_GAM + j : R_RSQ + j, g); fr_mul(o, o, g); }
    const bool digit = k < (unsigned)s.D, pole = k < (unsigned)s.base;
    if (!digit && !pole) return;
    Fr qi, a, b, c, d, pub;
    bool have = false;
    for (int j = 0; j <= s.lg; j++)
        if ((k + 1) >> j & 1) { rl(R_QIP + j, g); if (have) fr_mul(qi, qi, g); else { qi = g; have = true; } }
    fr_zero(pub);
    if (digit) {
        const unsigned sh = (unsigned)s.bb * (k % (unsigned)s.dp);            // base^(k mod dp) = 2^sh, sh < 64
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        w[sh >> 5] = 1u << (sh & 31);
        fr_from_words(b, w, false);
        rl(R_LAM + (int)(k / (unsigned)s.dp), a); fr_mul(a, a, b);
        rl(R_T2, b); fr_mul(a, a, b); fr_mul(a, a, qi);                       // t^2 ad_k q^-(k+1)
        rl(R_XD, b); fr_mul(b, b, qi);
        rl(R_E, c); fr_sub<512, 30>(d, c, b);
        rl(R_T, c); fr_mul(b, d, c);                                          // t (e - x delta q^-(k+1)): 514 r * 2 r
        add_term(pub, a); add_term(pub, b);
    }
    if (pole) { rl(R_EIN + (int)k, a); add_product(pub, a, qi); }
    fr_mul(pub, pub, one);                            // 6 r * r
    sub_product(o, o, pub);
}

// Where own slot q of proof i lies in the batch's weight array, whose order is that of the three point arrays of the call one behind the other:
// [values: rows x m | round_points: rows x 4 | wnla_points: rows x 2 K]
FRD size_t batch_weight_index(const Shape &s, size_t rows, size_t i, unsigned q) {
    if (q < (unsigned)s.m) return i * (size_t)s.m + q;
    if (q < (unsigned)s.m + 4) return rows * (size_t)s.m + i * 4 + (q - (unsigned)s.m);
    return rows * (size_t)(s.m + 4) + i * (size_t)(2 * s.K) + (q - (unsigned)s.m - 4);
}

#if defined(__HIPCC__)
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
using colk::ld_words;
using colk::st_words;
// the record of a chunk: word (idx * NL + limb) * rows + i
struct RecDev {
    uint32_t *__restrict__ p; size_t rows;
    __device__ __forceinline__ void ld(size_t i, int idx, Fr &x) const {
#pragma unroll
        for (int j = 0; j < NL; j++) x.l[j] = p[((size_t)idx * NL + j) * rows + i];
    }
    __device__ __forceinline__ void st(size_t i, int idx, const Fr &x) const {
#pragma unroll
        for (int j = 0; j < NL; j++) p[((size_t)idx * NL + j) * rows + i] = x.l[j];
    }
};
// One lane per proof.  chal: rows x (7 + K) x 8 words, l_n: rows x 2 x 8 (in the caller's form) -> the record, own[(i * own_stride + slot) * 8 ..] canonical
// words (own_stride = own, or own + 1 with a one behind), bad[i]
__global__ void __launch_bounds__(64) k_bpp_consts(Shape s, const uint32_t *__restrict__ chal, const uint32_t *__restrict__ l_n, bool mont, size_t rows, RecDev rec, int own_stride,
                                                   uint32_t *__restrict__ own, uint8_t *__restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const size_t nc = (size_t)(N_CHAL + s.K);
    const bool b = bpp_consts(s, own_stride > s.own, [&](int k, Fr &x) { ld_words(x, chal, i * nc + (size_t)k, mont); }, [&](int k, Fr &x) { ld_words(x, l_n, i * 2 + (size_t)k, mont); },
                              [&](int idx, Fr &x) { rec.ld(i, idx, x); }, [&](int idx, const Fr &x) { rec.st(i, idx, x); },
                              [&](int slot, const Fr &x) { st_words(own, i * (size_t)own_stride + (size_t)slot, x); });
    bad[i] = b ? 1 : 0;
}
// One lane per (proof, shared slot): out_rows[(i * (9 + NG) + slot) * 8 ..] = the canonical scalar, the packed rows many_rows_resident reads
__global__ void __launch_bounds__(256) k_bpp_shared(Shape s, size_t rows, RecDev rec, uint32_t *__restrict__ out_rows) {
    const size_t n = (size_t)(SHARED0 + s.NG), t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n;
    if (i >= rows) return;
    Fr o;
    bpp_shared(s, (unsigned)(t % n), [&](int idx, Fr &x) { rec.ld(i, idx, x); }, o);
    st_words(out_rows, t, o);
}
// One lane per (proof, slot <= own): bases[(i * (own + 1) + slot) * 24 ..] = the proof's own points in the order of its own scalars, then P_i (zero words where
// p_inf[i]).  values: rows x m x 24 words; round_points: rows x 4 x 24; wnla_points: rows x 2 K x 24; p: rows x 24
__global__ void __launch_bounds__(256) k_bpp_stage(Shape s, const uint32_t *__restrict__ values, const uint32_t *__restrict__ round_points, const uint32_t *__restrict__ wnla_points,
                                                   const uint32_t *__restrict__ p, const uint8_t *__restrict__ p_inf, size_t rows, uint32_t *__restrict__ bases) {
    const size_t T = (size_t)s.own + 1, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / T;
    const unsigned q = (unsigned)(t % T);
    if (i >= rows) return;
    const uint32_t *from = q < (unsigned)s.m ? values + (i * (size_t)s.m + q) * 2 * FQW
                         : q < (unsigned)s.m + 4 ? round_points + (i * 4 + (q - (unsigned)s.m)) * 2 * FQW
                         : q < (unsigned)s.own ? wnla_points + (i * (size_t)(2 * s.K) + (q - (unsigned)s.m - 4)) * 2 * FQW : p + i * 2 * FQW;
    const bool zero = q == (unsigned)s.own && p_inf[i] != 0;
    const uint4 *src = reinterpret_cast<const uint4 *>(from);
    uint4 *dst = reinterpret_cast<uint4 *>(bases + t * 2 * FQW);
    for (int k = 0; k < 6; k++) dst[k] = zero ? make_uint4(0, 0, 0, 0) : src[k];
}
// One lane per proof: seg_inf[i] the identity flag of its segment's sum -> status[i]: 2 an inverse does not exist, 1 the equation fails, 0 verified
__global__ void __launch_bounds__(256) k_bpp_verdict(const uint8_t *__restrict__ seg_inf, const uint8_t *__restrict__ bad, size_t rows, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    status[i] = bad[i] ? 2 : seg_inf[i] ? 0 : 1;
}
// grid (9 + NG, blocks): block (k, b) sums column k of the packed rows over the proofs [b * 256 * run, ..) of the chunk, proof i weighing rho^(i0 + i) (a lane's
// own start power, a fixed tree in LDS, part[(k * gridDim.y + b) * NL ..] in the internal form).  The lanes of column 0 also write the batch's weights over the
// own points: wts[8 batch_weight_index(i, q) ..] = rho^(i0 + i) own[i][q] as canonical words.  rows_sc: k_bpp_shared's output; own: k_bpp_consts's, own scalars apart
__global__ void __launch_bounds__(256) k_bpp_col_sums(Shape s, const uint32_t *__restrict__ rows_sc, const uint32_t *__restrict__ own, colk::RhoWords rho_words, bool mont, size_t rows,
                                                      size_t i0, size_t run, uint32_t *__restrict__ part, uint32_t *__restrict__ wts) {
    const size_t n = (size_t)(SHARED0 + s.NG), k = blockIdx.x;
    Fr rho;
    fr_from_words(rho, rho_words.w, mont);
    colk::col_block_sum(k, rows, run, part, [&](size_t lo, size_t cnt, Fr &sum) {
        colk::col_run(rho, i0 + lo, cnt, [&](size_t j, Fr &v) { ld_words(v, rows_sc, (lo + j) * n + k, false); },
                      [&](size_t j, const Fr &w) {
                          if (k != 0) return;
                          for (int q = 0; q < s.own; q++) {
                              Fr a, b;
                              ld_words(a, own, (lo + j) * (size_t)s.own + (size_t)q, false);
                              fr_mul(b, a, w);
                              st_words(wts, batch_weight_index(s, rows, lo + j, (unsigned)q), b);
                          }
                      },
                      sum);
    });
}
#endif

}  // namespace bppk
