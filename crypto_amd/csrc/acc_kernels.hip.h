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
// the host's tables (ark-ff Montgomery words) -> internal form, once per call
__global__ void __launch_bounds__(256) k_acc_prep(const uint32_t *__restrict__ words, size_t n, uint32_t *__restrict__ tab) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    Fr x; ld_words(x, words, e, true);
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
#endif

}  // namespace acck
