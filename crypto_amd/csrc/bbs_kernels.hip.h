// crypto_amd/csrc/bbs_kernels.hip.h — the scalar half of BBS+ signing and verification in bulk on gfx950 (dock_bbs.hip drives it).
//
// Device side of SignatureG1::new (bbs_plus/src/signature.rs:138-211) and SignatureG1::verify (:272-296) for many signatures of one key.  With the
// signature parameters [g1, h_0, h_1 .. h_L] as ONE base set, b_i = g1 + s_i h_0 + sum_j m_ij h_j (bbs_plus/src/setup.rs:128-146) is the small MSM of the row
//   (1, s_i, m_i1 .. m_iL)
// and everything the scalar field has to do is to write such rows where the many-row MSM reads them (msm_many.hip.h many_rows_resident):
//   signing        row i times t_i = 1 / (x + e_i), the host's inverse: the MSM then yields A_i = t_i b_i itself                     k_bbs_rows (mult = t_i)
//   verification   row i as it stands: the MSM yields b_i, the addend of -((-e_i) A_i + b_i) = e_i A_i - b_i                          k_bbs_rows (mult = 1)
//   one verdict    the L + 2 column sums c_k = sum_i rho^i row_ik, the weights rho^i and rho^i e_i of the two MSMs over the A_i       k_bbs_col_sums, k_bbs_col_finish
// The per-lane routines are plain FRD functions over load / store functors (as acc_kernels.hip.h's are): the same text runs on the host under -DFP29_CHECK,
// where every product asserts its operand contract (tests/native/bbs_dev_host_shim.cpp).  Operand classes, as in acc_kernels.hip.h:
//   "product"  limbs < 2^29, value < 2 r   (what fr_mul and fr_from_words return)
//   "lazy sum" one carry pass after every addition of a product: limbs <= 2^29 + 1 below the top limb, value < 2 r per term
#pragma once
#include "fr29.hip.h"

namespace bbsk {
using namespace fr29;

// entry k of row i before its multiplier: one, s_i, m_i(k-2).  s(i, Fr &) / m(i, j, Fr &) load products.
template <class S, class M> FRD void row_value(Fr &v, size_t i, size_t k, S s, M m) {
    if (k == 0) fr_one(v); else if (k == 1) s(i, v); else m(i, k - 2, v);
}
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
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
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
// rows[(i * n + k) * 8 ..] = the canonical words (below r: bit 255 is never set) of mult_i (1, s_i, m_i1 .. m_iL)_k for i < rows, k < n = L + 2: one lane per
// entry, the lanes of a row neighbours.  s: rows x 8 words, msgs: rows x L x 8 words packed, both in the caller's form (mont).  t_words (ark-ff Montgomery
// words from the host) != NULL: mult_i = t_i; else one.
__global__ void __launch_bounds__(256) k_bbs_rows(const uint32_t *__restrict__ s, const uint32_t *__restrict__ msgs, const uint32_t *__restrict__ t_words, int mont, size_t rows,
                                                  size_t n, uint32_t *__restrict__ out_rows) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n, k = t % n;
    if (i >= rows) return;
    Fr v, mult, o;
    row_value(v, i, k, [&](size_t r, Fr &x) { ld_words(x, s, r, mont != 0); }, [&](size_t r, size_t j, Fr &x) { ld_words(x, msgs, r * (n - 2) + j, mont != 0); });
    if (t_words) ld_words(mult, t_words, i, true); else fr_one(mult);
    row_entry(o, v, mult);
    st_words(out_rows, t, o);
}
// grid (L + 2, blocks): block (k, b) sums column k over the rows [b * 256 * run, ..) of the chunk, lane t the `run` rows from (b * 256 + t) * run on with a start
// power of its own, rho^(i0 + that row); the block's 256 sums fold by a fixed tree in LDS and leave as part[(k * gridDim.y + b) * NL ..] in the internal form.
// Column 0 also writes wts[8 i ..] = rho^(i0 + i) and we[8 i ..] = rho^(i0 + i) e_i as canonical words.  rho_words, e, s, msgs: the caller's form (mont).
struct RhoWords { uint32_t w[8]; };
__global__ void __launch_bounds__(256) k_bbs_col_sums(const uint32_t *__restrict__ e, const uint32_t *__restrict__ s, const uint32_t *__restrict__ msgs, RhoWords rho_words, int mont,
                                                      size_t rows, size_t n, size_t i0, size_t run, uint32_t *__restrict__ part, uint32_t *__restrict__ wts, uint32_t *__restrict__ we) {
    __shared__ uint32_t sh[NL][256];
    const unsigned t = threadIdx.x;
    const size_t k = blockIdx.x, lo = ((size_t)blockIdx.y * 256 + t) * run, cnt = lo >= rows ? 0 : (rows - lo < run ? rows - lo : run);
    Fr rho, sum;
    fr_from_words(rho, rho_words.w, mont != 0);
    fr_zero(sum);
    if (cnt)
        col_run(rho, i0 + lo, cnt,
                [&](size_t j, Fr &v) {
                    row_value(v, lo + j, k, [&](size_t r, Fr &x) { ld_words(x, s, r, mont != 0); }, [&](size_t r, size_t c, Fr &x) { ld_words(x, msgs, r * (n - 2) + c, mont != 0); });
                },
                [&](size_t j, const Fr &w) {
                    if (k != 0) return;
                    Fr ei, p; ld_words(ei, e, lo + j, mont != 0);
                    fr_mul(p, ei, w);                 // 2 r * 2 r
                    st_words(wts, lo + j, w); st_words(we, lo + j, p);
                },
                sum);
#pragma unroll
    for (int l = 0; l < NL; l++) sh[l][t] = sum.l[l];
    __syncthreads();
    for (unsigned d = 128; d >= 1; d >>= 1) {
        if (t < d)
            tree_step(t, d, [&](unsigned q, Fr &x) { for (int l = 0; l < NL; l++) x.l[l] = sh[l][q]; }, [&](unsigned q, const Fr &x) { for (int l = 0; l < NL; l++) sh[l][q] = x.l[l]; });
        __syncthreads();
    }
    if (t == 0) {
        Fr one, r0; fr_one(one);
        for (int l = 0; l < NL; l++) r0.l[l] = sh[l][0];
        fr_mul(r0, r0, one);
        for (int l = 0; l < NL; l++) part[(k * gridDim.y + blockIdx.y) * NL + l] = r0.l[l];
    }
}
// one lane per column: the chunk's block sums onto the running sum (run_sums[k * NL ..], internal form; first: it starts from zero), in block order; the running
// sum goes back, and out_words[8 k ..] = the canonical words of -c_k (neg) or c_k as they stand after this chunk.
__global__ void __launch_bounds__(64) k_bbs_col_finish(const uint32_t *__restrict__ part, size_t nparts, size_t n, int first, int neg, uint32_t *__restrict__ run_sums,
                                                       uint32_t *__restrict__ out_words) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Fr start, c, o;
    if (first) fr_zero(start); else for (int l = 0; l < NL; l++) start.l[l] = run_sums[k * NL + l];
    col_finish(start, nparts, [&](size_t b, Fr &v) { for (int l = 0; l < NL; l++) v.l[l] = part[(k * nparts + b) * NL + l]; }, c);
    for (int l = 0; l < NL; l++) run_sums[k * NL + l] = c.l[l];
    if (neg) neg_product(o, c); else o = c;
    st_words(out_words, k, o);
}
#endif

}  // namespace bbsk
