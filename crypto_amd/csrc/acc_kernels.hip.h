// crypto_amd/csrc/acc_kernels.hip.h — the scalar half of the accumulator manager's batch witness update on gfx950 (dock_accumulator.hip drives it).
//
// Device side of Witness::compute_update_using_secret_key_after_batch_updates (vb_accumulator/src/witness.rs:165-285) and of the
// polynomial evaluations it calls (vb_accumulator/src/batch_utils.rs:81-470: Poly_d::eval_direct, Poly_v_A / Poly_v_D / Poly_v_AD::eval_direct and
// their *_on_batch forms).  After additions a_0 .. and removals r_0 .. the witness C of the element y becomes
//   C' = (d_A(y) / d_D(y)) C + (v_AD(y) / d_D(y)) V,      d_U(y) = prod_{u in U} (u - y),   v_AD = v_A - Phi v_D
// with, over the host's tables F_s = prod_{i<s} (a_i + alpha), G_s = prod_{i<=s} (r_i + alpha)^-1, Phi = prod_i (a_i + alpha)  (alpha stays on the host),
//   additions, one forward pass per y:   S <- S (a_s - y) + F_s,  P <- P (a_s - y)     from S = 0, P = 1 to S = v_A(y), P = d_A(y)
//   removals,  one forward pass per y:   S <- S + G_s P,          P <- P (r_s - y)     from S = 0, P = 1 to S = v_D(y), P = d_D(y)
// Both passes compose affine maps, so a pass over [lo, hi) started from (P, S) = (1, 0) yields (P_c, S_c) and the chunks combine left to right:
//   additions S <- S P_c + S_c,  removals S <- S + P S_c,  both P <- P P_c          (what fills the chip when there are few elements and long lists).
// The per-lane routines are plain FRD functions over load / store functors (as fr_batch_inv is): the same text runs on the host under -DFP29_CHECK, where
// every product asserts its operand contract (tests/native/acc_dev_host_shim.cpp).  Operand classes used below:
//   "product"  limbs < 2^29, value < 2 r   (what fr_mul returns; the table entries and y are products)
//   "lazy sum" one carry pass after every addition of a product: limbs <= 2^29 + 1 below the top limb, value < 2 r per term (at most 2^31 terms: < 2^32 r)
#pragma once
#include "fr29.hip.h"

namespace acck {
using namespace fr29;

// one step of the additions pass.  a, F: table entries, y: products; P: a product; S: limbs <= 2^29, value < 4 r.
FRD void add_step(Fr &P, Fr &S, const Fr &y, const Fr &a, const Fr &F) {
    Fr d, t;
    fr_sub<512, 30>(d, a, y);             // a - y + 512 r: limbs < 2^31, value < 514 r — the first operand of both products, no carry pass
    fr_mul(t, d, S);                      // 514 r * 4 r
    fr_mul(P, d, P);                      // 514 r * 2 r
    fr_add(S, t, F); fr_norm(S, S);       // a product plus a table entry: limbs <= 2^29 after the carry pass (the second operand of the next step), value < 4 r
}
// one step of the removals pass.  rr, G: table entries, y: products; P: a product; S: a lazy sum.
FRD void rem_step(Fr &P, Fr &S, const Fr &y, const Fr &rr, const Fr &G) {
    Fr d, t;
    fr_sub<512, 30>(d, rr, y);            // as above
    fr_mul(t, P, G);                      // 2 r * 2 r (the P of before the step)
    fr_mul(P, d, P);                      // 514 r * 2 r
    fr_add(S, S, t); fr_norm(S, S);       // lazy sum: one more term
}
// the chunk [alo, ahi) of the additions pass and [rlo, rhi) of the removals pass for one y, both started from (1, 0).  The passes are independent
// chains: their steps are interleaved while both have entries left (four independent products per iteration).  ta(s, a, F) / tr(s, r, G) load entry s
// of the tables.  Results: products (the sums are reduced by a product with one).
template <class TA, class TR> FRD void eval_chunk(const Fr &y, size_t alo, size_t ahi, size_t rlo, size_t rhi, TA ta, TR tr, Fr &PA, Fr &SA, Fr &PD, Fr &SD) {
    Fr one; fr_one(one);
    PA = one; PD = one; fr_zero(SA); fr_zero(SD);
    const size_t na = ahi - alo, nr = rhi - rlo, both = na < nr ? na : nr;
    Fr u, v, w, x;
    for (size_t s = 0; s < both; s++) {
        ta(alo + s, u, v); tr(rlo + s, w, x);
        add_step(PA, SA, y, u, v);
        rem_step(PD, SD, y, w, x);
    }
    for (size_t s = both; s < na; s++) { ta(alo + s, u, v); add_step(PA, SA, y, u, v); }
    for (size_t s = both; s < nr; s++) { tr(rlo + s, w, x); rem_step(PD, SD, y, w, x); }
    fr_mul(SA, SA, one);                  // 4 r * r
    fr_mul(SD, SD, one);                  // 2^32 r * r
}
// the running state (PA, SA, PD, SD) of an element, started from (1, 0, 1, 0), takes the next chunk's results (products) on its right.
// PA, PD: products; SA: limbs < 2^30, value < 4 r (a first operand); SD: a lazy sum (at most 2^31 chunks).
FRD void combine_step(Fr &PA, Fr &SA, Fr &PD, Fr &SD, const Fr &pa, const Fr &sa, const Fr &pd, const Fr &sd) {
    Fr t;
    fr_mul(t, SA, pa); fr_add(SA, t, sa);                      // 4 r * 2 r; two products added: limbs < 2^30
    fr_mul(t, PD, sd); fr_add(SD, SD, t); fr_norm(SD, SD);     // 2 r * 2 r (the PD of before the step)
    fr_mul(PA, PA, pa); fr_mul(PD, PD, pd);
}
// value = 0 mod r, for a product
FRD bool is_zero(const Fr &a) {
    Fr c; fr_canon<2>(c, a);
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) t |= c.l[i];
    return t == 0;
}
// f = d_A / d_D and g = (v_A - Phi v_D) / d_D for the n elements of one lane's share, with ONE fr_inv (Montgomery's trick, fr_batch_inv).
//   elem(k, PA, SA, PD, SD)   the finished passes of element k: PA, PD products; SA limbs < 2^30, value < 4 r; SD a lazy sum or a product
//   ld(k, q, Fr &) / st(k, q, const Fr &)   four scratch slots per element: q = 0, 1 the numerators of f and g, 2 the denominator, 3 the prefix product, then the inverse
//   out(k, f, g)              products
// A zero d_D (the element is among the removals) must not poison the trick: one takes its place in the product and the element gets f = g = 0, which is
// what ark-ff's batch_inversion leaves for a zero entry [ark-0.4, recalled] and so what the reference's arithmetic yields there.
template <class E, class LD, class ST, class OUT> FRD void finish_share(size_t n, const Fr &phi, E elem, LD ld, ST st, OUT out) {
    for (size_t k = 0; k < n; k++) {
        Fr PA, SA, PD, SD, t, ng;
        elem(k, PA, SA, PD, SD);
        fr_mul(t, SD, phi);                                    // 2^32 r * 2 r
        fr_sub(ng, SA, t); fr_norm(ng, ng);                    // v_AD: limbs < 2^29 + 8, value < 516 r — the first operand of the product with the inverse
        if (is_zero(PD)) { fr_zero(PA); fr_zero(ng); fr_one(PD); }
        st(k, 0, PA); st(k, 1, ng); st(k, 2, PD);
    }
    fr_batch_inv(n, [&](size_t k, Fr &v) { ld(k, 2, v); }, [&](size_t k, Fr &v) { ld(k, 3, v); }, [&](size_t k, const Fr &v) { st(k, 3, v); });
    for (size_t k = 0; k < n; k++) {
        Fr nf, ng, inv, f, g;
        ld(k, 0, nf); ld(k, 1, ng); ld(k, 3, inv);
        fr_mul(f, nf, inv);                                    // 2 r * 2 r
        fr_mul(g, ng, inv);                                    // 516 r * 2 r
        out(k, f, g);
    }
}

// ---- Omega (batch_utils.rs:498-509): the coefficients of v_AD from its values at the N-th roots of unity ---------------------------------------------
// v_AD has max(|A|, |D|) coefficients, so its values at the N >= max(|A|, |D|) roots of unity and one inverse transform of size N give them exactly.
// The finishing of one evaluation point when v_AD alone is wanted: no d_D, no inversion.  SA, SD as finish_share takes them; the result is a product
// (what the transform takes).
FRD void omega_value(Fr &v, const Fr &SA, const Fr &SD, const Fr &phi) {
    Fr t, one; fr_one(one);
    fr_mul(t, SD, phi);                                        // 2^32 r * 2 r
    fr_sub(v, SA, t); fr_norm(v, v);                           // limbs < 2^29 + 8, value < 516 r
    fr_mul(v, v, one);                                         // 516 r * r
}
// the transform of size two with its scaling: c_0 = (e_0 + e_1) / 2, c_1 = (e_0 - e_1) / 2.  e_0, e_1, half: products.
FRD void omega_pair(Fr &c0, Fr &c1, const Fr &e0, const Fr &e1, const Fr &half) {
    Fr s, d;
    fr_add(s, e0, e1);                                         // two products: limbs < 2^30, value < 4 r
    fr_sub<512, 30>(d, e0, e1);                                // limbs < 2^31, value < 514 r
    fr_mul(c0, s, half); fr_mul(c1, d, half);                  // 4 r * 2 r, 514 r * 2 r
}

// ---- the holders' update from public information (witness.rs:292-314) --------------------------------------------------------------------------------
// Per holder f = d_A(y) / d_D(y) and s = 1 / d_D(y); the row [s, s y, .., s y^(n-1)] then meets Omega in an MSM.  No secret, no F / G / Phi.
// the chunk [alo, ahi) of d_A(y) = prod (a_s - y) and [rlo, rhi) of d_D(y), both started from one: two independent chains, interleaved while both have
// entries left.  la(s, a) / lr(s, r) load entry s of the lists (products); y: a product.  Chunks combine by a plain product.
template <class LA, class LR> FRD void pub_chunk(const Fr &y, size_t alo, size_t ahi, size_t rlo, size_t rhi, LA la, LR lr, Fr &PA, Fr &PD) {
    fr_one(PA); PD = PA;
    const size_t na = ahi - alo, nr = rhi - rlo, both = na < nr ? na : nr;
    Fr u, w, d, e;
    for (size_t s = 0; s < both; s++) {
        la(alo + s, u); lr(rlo + s, w);
        fr_sub<512, 30>(d, u, y); fr_sub<512, 30>(e, w, y);   // limbs < 2^31, value < 514 r: first operands, no carry pass
        fr_mul(PA, d, PA); fr_mul(PD, e, PD);                  // 514 r * 2 r
    }
    for (size_t s = both; s < na; s++) { la(alo + s, u); fr_sub<512, 30>(d, u, y); fr_mul(PA, d, PA); }
    for (size_t s = both; s < nr; s++) { lr(rlo + s, w); fr_sub<512, 30>(e, w, y); fr_mul(PD, e, PD); }
}
// f = d_A / d_D and s = 1 / d_D for the n holders of one lane's share, with ONE fr_inv (fr_batch_inv, as finish_share uses it).
//   elem(k, PA, PD)    the finished products of holder k (products)
//   ld / st            four scratch slots per holder as in finish_share: 0 the numerator of f, 1 the mark (one, or zero for a zero d_D), 2 the denominator, 3 the
//                      prefix product, then the inverse
//   out(k, f, s, ok)   products; a zero d_D (the element is among the removals: the reference's Err(CannotBeZero)) gives f = s = 0 and ok = false, and one
//                      takes its place in the trick
template <class E, class LD, class ST, class OUT> FRD void pub_finish_share(size_t n, E elem, LD ld, ST st, OUT out) {
    for (size_t k = 0; k < n; k++) {
        Fr PA, PD, mk;
        elem(k, PA, PD);
        fr_one(mk);
        if (is_zero(PD)) { fr_zero(PA); fr_zero(mk); fr_one(PD); }
        st(k, 0, PA); st(k, 1, mk); st(k, 2, PD);
    }
    fr_batch_inv(n, [&](size_t k, Fr &v) { ld(k, 2, v); }, [&](size_t k, Fr &v) { ld(k, 3, v); }, [&](size_t k, const Fr &v) { st(k, 3, v); });
    for (size_t k = 0; k < n; k++) {
        Fr nf, mk, inv, f, s;
        ld(k, 0, nf); ld(k, 1, mk); ld(k, 3, inv);
        fr_mul(f, nf, inv);                                    // 2 r * 2 r
        fr_mul(s, inv, mk);                                    // 2 r * r
        out(k, f, s, !is_zero(mk));
    }
}
// cnt consecutive entries j0, j0 + 1, .. of the row s y^j: the start power by square and multiply (at most 2 log2(j0) products), then one product per
// entry, so that the lanes of a row share it in runs.  y, s and everything derived from them are products: every fr_mul below is 2 r * 2 r.
template <class OUT> FRD void pub_row_run(const Fr &y, const Fr &s, size_t j0, size_t cnt, OUT out) {
    Fr cur = s, b = y;
    for (size_t e = j0; e; e >>= 1) { if (e & 1) fr_mul(cur, cur, b); if (e > 1) fr_mul(b, b, b); }
    for (size_t j = 0; j < cnt; j++) { out(j0 + j, cur); if (j + 1 < cnt) fr_mul(cur, cur, y); }
}

// ---- issuing witnesses (universal.rs:461-535, positive.rs:369-381) ------------------------------------------------------------------------------------
// d_i = f_V(-y_i) = prod_j (member_j - y_i) over ALL members of the accumulator: few points, an enormous list.  One lane owns U non-members y[0 .. owned)
// and walks the members [lo, hi) ONCE: one load per member (lm(s, member): a table entry, a product) feeds U independent chains, each started from one.
// Chains the lane does not own (j >= owned: the tail lane of a call whose m is no multiple of U) are skipped; their P stays one.  y: products.  Chunks
// combine by a plain product (d_times).
template <int U, class LM> FRD void d_chunk(const Fr (&y)[U], int owned, size_t lo, size_t hi, LM lm, Fr (&P)[U]) {
#pragma unroll
    for (int j = 0; j < U; j++) fr_one(P[j]);
    Fr t, d;
    for (size_t s = lo; s < hi; s++) {
        lm(s, t);
#pragma unroll
        for (int j = 0; j < U; j++)
            if (j < owned) {
                fr_sub<512, 30>(d, t, y[j]);      // member - y + 512 r: limbs < 2^31, value < 514 r — the first operand, no carry pass
                fr_mul(P[j], d, P[j]);            // 514 r * 2 r
            }
    }
}
// the running product D (a product; d_in as it was loaded, limbs <= 2^29 + 1 and value < 3 r at most) takes a chunk's or a pass's product P (a product) on its right
FRD void d_times(Fr &D, const Fr &P) { fr_mul(D, P, D); }        // 2 r * 3 r
// the scalar of one witness: (f_V - d) t for a non-membership witness (with_d), t itself for a membership witness; t = 1 / (y + alpha) from the host.
// fv, d, t: products.  Returns true for d = 0 (the reference's Err(CannotBeZero)): the scalar is zero then.
FRD bool issue_scalar(Fr &sc, bool with_d, const Fr &fv, const Fr &d, const Fr &t) {
    if (!with_d) { sc = t; return false; }
    Fr e;
    fr_sub<512, 30>(e, fv, d);                    // f_V - d + 512 r: limbs < 2^31, value < 514 r — a first operand, no carry pass
    fr_mul(sc, e, t);                             // 514 r * 2 r
    if (!is_zero(d)) return false;
    fr_zero(sc);
    return true;
}

#if defined(__HIPCC__)
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
// Tables: entry e of the internal-form table at tab[e * NL ..]: [a_0 .. | F_0 .. | r_0 .. | G_0 .. | Phi], 2 na + 2 nr + 1 entries.  Every lane of a block
// reads the same entry in the same step (the chunk is the block's, not the lane's), so the loads are uniform.
// part (K > 1): word l of result q (PA, SA, PD, SD) of chunk c of element i at part[((q * NL + l) * K + c) * m + i].
// scratch: word l of slot q of element i at scratch[(q * NL + l) * m + i].  fg: canonical words, f_i at fg[8 i ..], g_i at fg[8 (m + i) ..].
__device__ __forceinline__ void ld_tab(Fr &r, const uint32_t *__restrict__ tab, size_t e) {
#pragma unroll
    for (int l = 0; l < NL; l++) r.l[l] = tab[e * NL + l];
}
__device__ __forceinline__ void ld_words(Fr &r, const uint32_t *__restrict__ words, size_t i, bool mont) {
    const uint4 *q = reinterpret_cast<const uint4 *>(words + i * 8);
    const uint4 a = q[0], b = q[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    fr_from_words(r, w, mont);
}
__device__ __forceinline__ void st_words(uint32_t *__restrict__ words, size_t i, const Fr &x) {
    uint32_t w[8]; fr_to_words(w, x, false);
    uint4 *q = reinterpret_cast<uint4 *>(words + i * 8);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]); q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// the host's tables (ark-ff Montgomery words), or the caller's public lists (mont = 0: canonical words) -> internal form, once per call
__global__ void __launch_bounds__(256) k_acc_prep(const uint32_t *__restrict__ words, size_t n, uint32_t *__restrict__ tab, int mont) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    Fr x; ld_words(x, words, e, mont != 0);
#pragma unroll
    for (int l = 0; l < NL; l++) tab[e * NL + l] = x.l[l];
}
struct ScratchIo {
    uint32_t *__restrict__ scratch; uint32_t *__restrict__ fg; size_t m, g, G;
    __device__ __forceinline__ void ld(size_t k, int q, Fr &v) const {
#pragma unroll
        for (int l = 0; l < NL; l++) v.l[l] = scratch[(size_t)(q * NL + l) * m + g + k * G];
    }
    __device__ __forceinline__ void st(size_t k, int q, const Fr &v) const {
#pragma unroll
        for (int l = 0; l < NL; l++) scratch[(size_t)(q * NL + l) * m + g + k * G] = v.l[l];
    }
    __device__ __forceinline__ void out(size_t k, const Fr &f, const Fr &gg) const { st_words(fg, g + k * G, f); st_words(fg, m + g + k * G, gg); }
};
// grid (lanes / 256, K).  K = 1: lane g of G owns the elements g + k G, runs both passes whole for each and finishes them.  K > 1: lane (i, c) runs chunk c of
// both passes of element i (G = m) and leaves the results to k_acc_combine.
__global__ void __launch_bounds__(256) k_acc_eval(const uint32_t *__restrict__ tab, size_t na, size_t nr, const uint32_t *__restrict__ elems, int mont, size_t m, uint32_t K, size_t G,
                                                  uint32_t *__restrict__ part, uint32_t *__restrict__ scratch, uint32_t *__restrict__ fg) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint32_t *ta_ = tab, *tf_ = tab + na * NL, *tr_ = tab + 2 * na * NL, *tg_ = tab + (2 * na + nr) * NL;
    auto ta = [&](size_t s, Fr &a, Fr &F) { ld_tab(a, ta_, s); ld_tab(F, tf_, s); };
    auto tr = [&](size_t s, Fr &r, Fr &Gs) { ld_tab(r, tr_, s); ld_tab(Gs, tg_, s); };
    if (K == 1) {
        const ScratchIo io{scratch, fg, m, g, G};
        Fr phi; ld_tab(phi, tab, 2 * na + 2 * nr);
        finish_share((m - g + G - 1) / G, phi,
                     [&](size_t k, Fr &PA, Fr &SA, Fr &PD, Fr &SD) { Fr y; ld_words(y, elems, g + k * G, mont != 0); eval_chunk(y, 0, na, 0, nr, ta, tr, PA, SA, PD, SD); },
                     [&](size_t k, int q, Fr &v) { io.ld(k, q, v); }, [&](size_t k, int q, const Fr &v) { io.st(k, q, v); },
                     [&](size_t k, const Fr &f, const Fr &gg) { io.out(k, f, gg); });
        return;
    }
    const size_t c = blockIdx.y;
    Fr y, r[4]; ld_words(y, elems, g, mont != 0);
    eval_chunk(y, na * c / K, na * (c + 1) / K, nr * c / K, nr * (c + 1) / K, ta, tr, r[0], r[1], r[2], r[3]);
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int l = 0; l < NL; l++) part[((size_t)(q * NL + l) * K + c) * m + g] = r[q].l[l];
}
// K > 1: lane g of G owns the elements g + k G, combines each one's K chunks left to right and finishes them
__global__ void __launch_bounds__(256) k_acc_combine(const uint32_t *__restrict__ tab, size_t na, size_t nr, const uint32_t *__restrict__ part, size_t m, uint32_t K, size_t G,
                                                     uint32_t *__restrict__ scratch, uint32_t *__restrict__ fg) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const ScratchIo io{scratch, fg, m, g, G};
    Fr phi; ld_tab(phi, tab, 2 * na + 2 * nr);
    finish_share((m - g + G - 1) / G, phi,
                 [&](size_t k, Fr &PA, Fr &SA, Fr &PD, Fr &SD) {
                     const size_t i = g + k * G;
                     fr_one(PA); PD = PA; fr_zero(SA); fr_zero(SD);
                     for (uint32_t c = 0; c < K; c++) {
                         Fr r[4];
#pragma unroll
                         for (int q = 0; q < 4; q++)
#pragma unroll
                             for (int l = 0; l < NL; l++) r[q].l[l] = part[((size_t)(q * NL + l) * K + c) * m + i];
                         combine_step(PA, SA, PD, SD, r[0], r[1], r[2], r[3]);
                     }
                 },
                 [&](size_t k, int q, Fr &v) { io.ld(k, q, v); }, [&](size_t k, int q, const Fr &v) { io.st(k, q, v); },
                 [&](size_t k, const Fr &f, const Fr &gg) { io.out(k, f, gg); });
}
// ---- Omega -----------------------------------------------------------------------------------------------------------------------------------------------
// pts, ev: N elements in the transform's form (limb-major: word l of element i at [l * N + i]); pts = the N-th roots of unity, ev = v_AD there.
__device__ __forceinline__ void ld_soa(Fr &r, const uint32_t *__restrict__ a, size_t n, size_t i) {
#pragma unroll
    for (int l = 0; l < NL; l++) r.l[l] = a[(size_t)l * n + i];
}
__device__ __forceinline__ void st_soa(uint32_t *__restrict__ a, size_t n, size_t i, const Fr &x) {
#pragma unroll
    for (int l = 0; l < NL; l++) a[(size_t)l * n + i] = x.l[l];
}
// grid (N / 256, K): lane (i, c) runs chunk c of both passes at point i.  K = 1: the passes run whole and ev[i] = v_A - Phi v_D is written; K > 1: the chunk's
// results go to part (the layout of k_acc_eval, m = N) for k_acc_omega_combine.
__global__ void __launch_bounds__(256) k_acc_omega_eval(const uint32_t *__restrict__ tab, size_t na, size_t nr, const uint32_t *__restrict__ pts, size_t N, uint32_t K,
                                                        uint32_t *__restrict__ part, uint32_t *__restrict__ ev) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    const uint32_t *ta_ = tab, *tf_ = tab + na * NL, *tr_ = tab + 2 * na * NL, *tg_ = tab + (2 * na + nr) * NL;
    auto ta = [&](size_t s, Fr &a, Fr &F) { ld_tab(a, ta_, s); ld_tab(F, tf_, s); };
    auto tr = [&](size_t s, Fr &r, Fr &Gs) { ld_tab(r, tr_, s); ld_tab(Gs, tg_, s); };
    const size_t c = blockIdx.y;
    Fr y, r[4]; ld_soa(y, pts, N, g);
    eval_chunk(y, na * c / K, na * (c + 1) / K, nr * c / K, nr * (c + 1) / K, ta, tr, r[0], r[1], r[2], r[3]);
    if (K == 1) {
        Fr phi, v; ld_tab(phi, tab, 2 * na + 2 * nr);
        omega_value(v, r[1], r[3], phi);
        st_soa(ev, N, g, v);
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int l = 0; l < NL; l++) part[((size_t)(q * NL + l) * K + c) * N + g] = r[q].l[l];
}
__global__ void __launch_bounds__(256) k_acc_omega_combine(const uint32_t *__restrict__ tab, size_t na, size_t nr, const uint32_t *__restrict__ part, size_t N, uint32_t K,
                                                           uint32_t *__restrict__ ev) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    Fr PA, SA, PD, SD, phi, v;
    fr_one(PA); PD = PA; fr_zero(SA); fr_zero(SD);
    for (uint32_t c = 0; c < K; c++) {
        Fr r[4];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int l = 0; l < NL; l++) r[q].l[l] = part[((size_t)(q * NL + l) * K + c) * N + g];
        combine_step(PA, SA, PD, SD, r[0], r[1], r[2], r[3]);
    }
    ld_tab(phi, tab, 2 * na + 2 * nr);
    omega_value(v, SA, SD, phi);
    st_soa(ev, N, g, v);
}
// After the inverse transform (decimation in frequency: bit-reversed, times N) of N = 2^logn >= 4 values, or instead of it for N = 1 (nothing to do) and
// N = 2 (omega_pair): coefficient k = ev[rev k] / N as canonical words at coeff[8 k ..] and nz[k] = (it is not zero), for the k < len the polynomial can have.
struct Words8 { uint32_t w[8]; };
__global__ void __launch_bounds__(256) k_acc_omega_coeffs(const uint32_t *__restrict__ ev, int logn, Words8 ninv_words, size_t len, uint32_t *__restrict__ coeff, uint8_t *__restrict__ nz) {
    const size_t N = (size_t)1 << logn, p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return;
    Fr ninv, c; fr_from_words(ninv, ninv_words.w, false);
    size_t k = p;
    if (logn == 1) {
        Fr e0, e1, c0, c1; ld_soa(e0, ev, N, 0); ld_soa(e1, ev, N, 1);
        omega_pair(c0, c1, e0, e1, ninv);
        c = p ? c1 : c0;
    } else {
        Fr x; ld_soa(x, ev, N, p);
        fr_mul(c, x, ninv);                                    // the transform's output is a first operand (as k_coset_scale takes it); ninv: a product
        if (logn > 1) k = (size_t)(__brev((uint32_t)p) >> (32 - logn));
    }
    if (k >= len) return;
    st_words(coeff, k, c);
    nz[k] = is_zero(c) ? 0 : 1;
}

// ---- the public update ------------------------------------------------------------------------------------------------------------------------------------
// lists: the internal-form entries [a_0 .. | r_0 ..] (k_acc_prep).  part (K > 1): word l of result q (PA, PD) of chunk c of holder i at
// part[((q * NL + l) * K + c) * m + i].  scratch: as above.  fs: canonical words, f_i at fs[8 i ..], s_i at fs[8 (m + i) ..].  ok[i] = (d_D(y_i) != 0).
struct PubIo {
    uint32_t *__restrict__ scratch; uint32_t *__restrict__ fs; uint8_t *__restrict__ ok; size_t m, g, G;
    __device__ __forceinline__ void ld(size_t k, int q, Fr &v) const {
#pragma unroll
        for (int l = 0; l < NL; l++) v.l[l] = scratch[(size_t)(q * NL + l) * m + g + k * G];
    }
    __device__ __forceinline__ void st(size_t k, int q, const Fr &v) const {
#pragma unroll
        for (int l = 0; l < NL; l++) scratch[(size_t)(q * NL + l) * m + g + k * G] = v.l[l];
    }
    __device__ __forceinline__ void out(size_t k, const Fr &f, const Fr &s, bool good) const { st_words(fs, g + k * G, f); st_words(fs, m + g + k * G, s); ok[g + k * G] = good ? 1 : 0; }
};
// grid (lanes / 256, K), as k_acc_eval: K = 1: lane g of G owns the holders g + k G, runs both products whole and finishes them; K > 1: lane (i, c) runs chunk c
// of holder i (G = m) and leaves the results to k_acc_pub_combine.
__global__ void __launch_bounds__(256) k_acc_pub_factors(const uint32_t *__restrict__ lists, size_t na, size_t nr, const uint32_t *__restrict__ elems, int mont, size_t m, uint32_t K, size_t G,
                                                         uint32_t *__restrict__ part, uint32_t *__restrict__ scratch, uint32_t *__restrict__ fs, uint8_t *__restrict__ ok) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint32_t *lr_ = lists + na * NL;
    auto la = [&](size_t s, Fr &a) { ld_tab(a, lists, s); };
    auto lr = [&](size_t s, Fr &r) { ld_tab(r, lr_, s); };
    if (K == 1) {
        const PubIo io{scratch, fs, ok, m, g, G};
        pub_finish_share((m - g + G - 1) / G,
                         [&](size_t k, Fr &PA, Fr &PD) { Fr y; ld_words(y, elems, g + k * G, mont != 0); pub_chunk(y, 0, na, 0, nr, la, lr, PA, PD); },
                         [&](size_t k, int q, Fr &v) { io.ld(k, q, v); }, [&](size_t k, int q, const Fr &v) { io.st(k, q, v); },
                         [&](size_t k, const Fr &f, const Fr &s, bool good) { io.out(k, f, s, good); });
        return;
    }
    const size_t c = blockIdx.y;
    Fr y, r[2]; ld_words(y, elems, g, mont != 0);
    pub_chunk(y, na * c / K, na * (c + 1) / K, nr * c / K, nr * (c + 1) / K, la, lr, r[0], r[1]);
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int l = 0; l < NL; l++) part[((size_t)(q * NL + l) * K + c) * m + g] = r[q].l[l];
}
__global__ void __launch_bounds__(256) k_acc_pub_combine(const uint32_t *__restrict__ part, size_t m, uint32_t K, size_t G, uint32_t *__restrict__ scratch, uint32_t *__restrict__ fs,
                                                         uint8_t *__restrict__ ok) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const PubIo io{scratch, fs, ok, m, g, G};
    pub_finish_share((m - g + G - 1) / G,
                     [&](size_t k, Fr &PA, Fr &PD) {
                         const size_t i = g + k * G;
                         fr_one(PA); PD = PA;
                         for (uint32_t c = 0; c < K; c++) {
                             Fr r[2];
#pragma unroll
                             for (int q = 0; q < 2; q++)
#pragma unroll
                                 for (int l = 0; l < NL; l++) r[q].l[l] = part[((size_t)(q * NL + l) * K + c) * m + i];
                             fr_mul(PA, PA, r[0]); fr_mul(PD, PD, r[1]);      // 2 r * 2 r
                         }
                     },
                     [&](size_t k, int q, Fr &v) { io.ld(k, q, v); }, [&](size_t k, int q, const Fr &v) { io.st(k, q, v); },
                     [&](size_t k, const Fr &f, const Fr &s, bool good) { io.out(k, f, s, good); });
}
// rows[(i * n + j) * 8 ..] = the canonical words of s_i y_i^j for the holders i < rows and j < n: the scalars of the many-row MSM, rows packed.  A row is shared by
// ceil(n / run) lanes, each walking `run` consecutive powers from a start power of its own (pub_row_run).
__global__ void __launch_bounds__(256) k_acc_pub_rows(const uint32_t *__restrict__ elems, int mont, const uint32_t *__restrict__ s_words, size_t rows, size_t n, size_t run,
                                                      uint32_t *__restrict__ out_rows) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per_row = (n + run - 1) / run, i = t / per_row;
    if (i >= rows) return;
    const size_t j0 = (t % per_row) * run, cnt = n - j0 < run ? n - j0 : run;
    Fr y, s; ld_words(y, elems, i, mont != 0); ld_words(s, s_words, i, false);
    pub_row_run(y, s, j0, cnt, [&](size_t j, const Fr &v) { st_words(out_rows, i * n + j, v); });
}

// ---- issuing witnesses ----------------------------------------------------------------------------------------------------------------------------------
// tab: the members of one pass in internal form (k_acc_prep), n of them.  run: the running product of every non-member between the passes, limb-major
// (ld_soa / st_soa over m).  part (K > 1): word l of chunk c of non-member i at part[(l * K + c) * m + i].  d_words: m x 8 words in the caller's form (mont).
struct DOut {
    const uint32_t *__restrict__ d_in; uint32_t *__restrict__ run; uint32_t *__restrict__ d_words; uint8_t *__restrict__ nz; size_t m; int mont, first, last;
    // the product before this pass: d_in (one for NULL) on the first pass, else what the pass before left
    __device__ __forceinline__ void start(Fr &D, size_t i) const {
        if (!first) ld_soa(D, run, m, i);
        else if (d_in) ld_words(D, d_in, i, mont != 0);
        else fr_one(D);
    }
    // after this pass: words and the non-zero flag on the last pass, else the internal form for the next
    __device__ __forceinline__ void finish(const Fr &D, size_t i) const {
        if (!last) { st_soa(run, m, i, D); return; }
        uint32_t w[8]; fr_to_words(w, D, mont != 0);
        uint4 *q = reinterpret_cast<uint4 *>(d_words + i * 8);
        q[0] = make_uint4(w[0], w[1], w[2], w[3]); q[1] = make_uint4(w[4], w[5], w[6], w[7]);
        nz[i] = is_zero(D) ? 0 : 1;
    }
};
// grid (lanes / 256, K): lane g of G = ceil(m / U) owns the non-members g + j G (j < U: the loads of y coalesce) and runs chunk c = blockIdx.y of the pass for
// all of them at once; every lane of a block reads the same member in the same step.  K = 1 finishes in place (DOut); K > 1 leaves the chunk's products to
// k_acc_d_combine.
template <int U> __global__ void __launch_bounds__(256) k_acc_d(const uint32_t *__restrict__ tab, size_t n, const uint32_t *__restrict__ elems, size_t m, uint32_t K, size_t G,
                                                                 uint32_t *__restrict__ part, DOut o) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int owned = (int)((m - g + G - 1) / G < (size_t)U ? (m - g + G - 1) / G : (size_t)U);
    Fr y[U], P[U];
#pragma unroll
    for (int j = 0; j < U; j++) { if (j < owned) ld_words(y[j], elems, g + j * G, o.mont != 0); else fr_zero(y[j]); }
    const size_t c = blockIdx.y;
    d_chunk<U>(y, owned, n * c / K, n * (c + 1) / K, [&](size_t s, Fr &a) { ld_tab(a, tab, s); }, P);
    if (K == 1) {
        // one copy of the finishing code for all chains: P[j] by selects, so that P stays in registers (an index known only at run time would put it in scratch)
#pragma unroll 1
        for (int j = 0; j < owned; j++) {
            Fr Pj = P[0], D;
#pragma unroll
            for (int q = 1; q < U; q++) if (j == q) Pj = P[q];
            const size_t i = g + j * G;
            o.start(D, i); d_times(D, Pj); o.finish(D, i);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < U; j++)
        if (j < owned) {
#pragma unroll
            for (int l = 0; l < NL; l++) part[((size_t)l * K + c) * m + g + j * G] = P[j].l[l];
        }
}
// K > 1: one lane per non-member: the running product times its K chunk products
__global__ void __launch_bounds__(256) k_acc_d_combine(const uint32_t *__restrict__ part, size_t m, uint32_t K, DOut o) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    Fr D, P; o.start(D, i);
    for (uint32_t c = 0; c < K; c++) {
#pragma unroll
        for (int l = 0; l < NL; l++) P.l[l] = part[((size_t)l * K + c) * m + i];
        d_times(D, P);
    }
    o.finish(D, i);
}
// sc[8 i ..] = the canonical words of (f_V - d_i) t_i (with_d) or of t_i, the scalars of k_fb_mul; zero[i] = (d_i is zero): that scalar is zero.
// d_words: the caller's form (mont); t_words: ark-ff Montgomery words from the host; fv: the caller's form.
__global__ void __launch_bounds__(256) k_acc_issue_scalars(const uint32_t *__restrict__ d_words, const uint32_t *__restrict__ t_words, Words8 fv_words, int mont, int with_d, size_t m,
                                                           uint32_t *__restrict__ sc, uint8_t *__restrict__ zero) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    Fr fv, d, t, s;
    fr_zero(fv); fr_zero(d);
    ld_words(t, t_words, i, true);
    if (with_d) { fr_from_words(fv, fv_words.w, mont != 0); ld_words(d, d_words, i, mont != 0); }
    const bool z = issue_scalar(s, with_d != 0, fv, d, t);
    st_words(sc, i, s);
    zero[i] = z ? 1 : 0;
}
#endif

}  // namespace acck
