// crypto_amd/csrc/bbs_routines.hip.h — the per-lane Fr routines the BBS+ scalar kernels share (bbs_kernels.hip.h: signatures; bbs_pok_kernels.hip.h: proofs of
// knowledge): plain FRD functions over load / store functors, so the same text runs on the host under -DFP29_CHECK, where every product asserts its operand
// contract (tests/native/bbs_dev_host_shim.cpp, bbs_pok_dev_host_shim.cpp); and, for device code, the loads and stores of 8-word scalars.  Operand classes, as in
// acc_kernels.hip.h:
//   "product"  limbs < 2^29, value < 2 r   (what fr_mul and fr_from_words return)
//   "lazy sum" one carry pass after every addition of a product: limbs <= 2^29 + 1 below the top limb, value < 2 r per term
#pragma once
#include "fr29.hip.h"

namespace bbsk {
using namespace fr29;

// entry k of row i before its multiplier, with `fixed` columns in front of the messages: one, [s_i,] m_i(k-fixed).  fixed = 2: BBS+ (1, s_i, m_i ..);
// fixed = 1: the 2023 scheme (1, m_i ..), where s is never called.  s(i, Fr &) / m(i, j, Fr &) load products.
template <class S, class M> FRD void row_value_fixed(Fr &v, size_t i, size_t k, size_t fixed, S s, M m) {
    if (k == 0) fr_one(v); else if (k < fixed) s(i, v); else m(i, k - fixed, v);
}
// the BBS+ row: one, s_i, m_i(k-2)
template <class S, class M> FRD void row_value(Fr &v, size_t i, size_t k, S s, M m) { row_value_fixed(v, i, k, 2, s, m); }
// o = mult v.  v, mult: products (mult: t_i, or one)
FRD void row_entry(Fr &o, const Fr &v, const Fr &mult) { fr_mul(o, v, mult); }      // 2 r * 2 r
// o = -v as a product.  v: a product; 512 r - v has limbs < 2^31 and value < 514 r: a first operand, no carry pass
FRD void neg_product(Fr &o, const Fr &v) {
    Fr z, d, one; fr_zero(z); fr_one(one);
    fr_sub<512, 30>(d, z, v);
    fr_mul(o, d, one);                                // 514 r * r
}
// p = rho^e by square and multiply (at most 2 log2(e) products; e = 0: one).  rho: a product; so is everything derived from it.
FRD void pow_start(Fr &p, const Fr &rho, size_t e) {
    Fr b = rho; fr_one(p);
    for (; e; e >>= 1) { if (e & 1) fr_mul(p, p, b); if (e > 1) fr_mul(b, b, b); }
}
// One lane's run of a column: sum = sum_{j < cnt} rho^(e0 + j) val(j), reduced to a product.  val(j, Fr &) loads the column's entry of the run's j-th row (a
// product); weight(j, w) sees w = rho^(e0 + j) (the lanes of column 0 write the weights and rho^i e_i from it).  The sum is a lazy sum of cnt <= 2^30 terms.
template <class V, class W> FRD void col_run(const Fr &rho, size_t e0, size_t cnt, V val, W weight, Fr &sum) {
    Fr w, v, t, one; fr_one(one);
    pow_start(w, rho, e0);
    fr_zero(sum);
    for (size_t j = 0; j < cnt; j++) {
        val(j, v);
        fr_mul(t, v, w);                              // 2 r * 2 r
        fr_add(sum, sum, t); fr_norm(sum, sum);
        weight(j, w);
        if (j + 1 < cnt) fr_mul(w, w, rho);
    }
    fr_mul(sum, sum, one);
}
// One step of a fixed tree over the lanes of a block: slot t takes slot t + d.  Every level adds two sums of equal depth, so after the eight levels of a block
// of 256 a slot holds at most 256 products: limbs <= 2^29 + 1 after each carry pass, value < 512 r.
template <class LD, class ST> FRD void tree_step(unsigned t, unsigned d, LD ld, ST st) {
    Fr a, b; ld(t, a); ld(t + d, b);
    fr_add(a, a, b); fr_norm(a, a);
    st(t, a);
}
// The second pass: c = start + part(0) + part(1) + .. in that order, reduced to a product; parts and start are products (start: the column's sum over the
// chunks before this one, or zero).
template <class P> FRD void col_finish(const Fr &start, size_t nparts, P part, Fr &c) {
    Fr one, v; fr_one(one);
    c = start;
    for (size_t b = 0; b < nparts; b++) { part(b, v); fr_add(c, c, v); fr_norm(c, c); }
    fr_mul(c, c, one);
}

#if defined(__HIPCC__)
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
struct RhoWords { uint32_t w[8]; };
#endif

}  // namespace bbsk
