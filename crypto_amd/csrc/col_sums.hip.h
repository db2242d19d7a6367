// crypto_amd/csrc/col_sums.hip.h — the column sums c_k = sum_i rho^i row_ik behind every "one verdict for n proofs" call: the per-lane Fr routines every scheme
// shares, and the ONE frame of a sums kernel's block.  The routines are plain FRD functions over load / store functors, so the same text runs on the host under
// -DFP29_CHECK, where every product asserts its operand contract (tests/native/col_frame_host.hpp walks chunks, columns, blocks, lanes, tree and finish as the
// kernels do, for every scheme's shim).  Operand classes, as in acc_kernels.hip.h:
//   "product"  limbs < 2^29, value < 2 r   (what fr_mul and fr_from_words return)
//   "lazy sum" one carry pass after every addition of a product: limbs <= 2^29 + 1 below the top limb, value < 2 r per term
// How a chunk of `count` rows becomes column sums (col_launch.hip.h has the launch side: COL_RUN, col_blocks, col_part_words, launch_col_finish):
//   a scheme's k_*_col_sums, grid (columns, col_blocks(count)), 256 lanes: load rho, then col_block_sum(k, count, run, part, lane_run).  Lane t of block b takes
//     the `run` rows from lo = (b * 256 + t) * run on (cnt of them are inside the chunk) and, where cnt != 0, lane_run(lo, cnt, sum) makes their sum a product —
//     the scheme's own term, start power and weight stores; the block's 256 sums fold by a fixed tree in LDS and leave as part[(k * gridDim.y + b) * NL ..]
//   k_col_finish (k_cols.hip), one lane per column: the chunk's block sums onto the running sum in block order; columns in [neg_lo, neg_hi) leave negated
// No atomics, no dependence on the order of execution: every word is the same in every run.
#pragma once
#include "fr29.hip.h"

namespace colk {
using namespace fr29;

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
// The frame of a sums kernel's block (k, blockIdx.y) of 256 lanes over a chunk of `count` rows: the lane's range, lane_run(lo, cnt, Fr &sum) where it is not
// empty, the 256 sums through LDS and the fixed tree, and lane 0's product as part[(k * gridDim.y + blockIdx.y) * NL ..] in the internal form.
template <class F> __device__ __forceinline__ void col_block_sum(size_t k, size_t count, size_t run, uint32_t *__restrict__ part, F lane_run) {
    __shared__ uint32_t sh[NL][256];
    const unsigned t = threadIdx.x;
    const size_t lo = ((size_t)blockIdx.y * 256 + t) * run, cnt = lo >= count ? 0 : (count - lo < run ? count - lo : run);
    Fr sum;
    fr_zero(sum);
    if (cnt) lane_run(lo, cnt, sum);
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
#endif

}  // namespace colk

// These routines grew up in bbs_routines.hip.h as bbsk::...: the BBS units, and host code written against any scheme's kernel header while they lived there,
// still find them under that name.  No scheme's header or launch file spells it.
namespace bbsk { using namespace colk; }
