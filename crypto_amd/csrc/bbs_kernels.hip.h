// crypto_amd/csrc/bbs_kernels.hip.h — the scalar half of BBS+ signing and verification in bulk on gfx950 (dock_bbs.hip drives it).
//
// Device side of SignatureG1::new (bbs_plus/src/signature.rs:138-211) and SignatureG1::verify (:272-296) for many signatures of one key.  With the
// signature parameters [g1, h_0, h_1 .. h_L] as ONE base set, b_i = g1 + s_i h_0 + sum_j m_ij h_j (bbs_plus/src/setup.rs:128-146) is the small MSM of the row
//   (1, s_i, m_i1 .. m_iL)
// and everything the scalar field has to do is to write such rows where the many-row MSM reads them (msm_many.hip.h many_rows_resident):
//   signing        row i times t_i = 1 / (x + e_i), the host's inverse: the MSM then yields A_i = t_i b_i itself                     k_bbs_rows (mult = t_i)
//   verification   row i as it stands: the MSM yields b_i, the addend of -((-e_i) A_i + b_i) = e_i A_i - b_i                          k_bbs_rows (mult = 1)
//   one verdict    the L + 2 column sums c_k = sum_i rho^i row_ik, the weights rho^i and rho^i e_i of the two MSMs over the A_i       k_bbs_col_sums, colk::k_col_finish
// The 2023 scheme (bbs_plus/src/signature_23.rs: no s, no h_0; parameters [g1, h_1 .. h_L], row (1, m_i1 .. m_iL)) is the same text with ONE fixed column in
// front of the messages instead of two: k_bbs_rows and k_bbs_col_sums take the count (`fixed`: 2 here, 1 there) and n = L + fixed.
// The row's routines (row_value, row_entry) are in bbs_routines.hip.h, shared with the proofs of knowledge (bbs_pok_kernels.hip.h); the column sums' (pow_start,
// col_run, the block frame col_block_sum, the second pass) in col_sums.hip.h, shared with every batch verifier; the kernels here drive them.
#pragma once
#include "bbs_routines.hip.h"

namespace bbsk {
#if defined(__HIPCC__)
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
// rows[(i * n + k) * 8 ..] = the canonical words (below r: bit 255 is never set) of mult_i (1, s_i, m_i1 .. m_iL)_k for i < rows, k < n = L + 2: one lane per
// entry, the lanes of a row neighbours.  s: rows x 8 words, msgs: rows x L x 8 words packed, both in the caller's form (mont).  t_words (ark-ff Montgomery
// words from the host) != NULL: mult_i = t_i; else one.  fixed = 2: the BBS+ row; fixed = 1: the 2023 scheme's mult_i (1, m_i1 .. m_iL), n = L + 1, s never read.
__global__ void __launch_bounds__(256) k_bbs_rows(const uint32_t *__restrict__ s, const uint32_t *__restrict__ msgs, const uint32_t *__restrict__ t_words, int mont, size_t rows,
                                                  size_t n, size_t fixed, uint32_t *__restrict__ out_rows) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n, k = t % n;
    if (i >= rows) return;
    Fr v, mult, o;
    row_value_fixed(v, i, k, fixed, [&](size_t r, Fr &x) { ld_words(x, s, r, mont != 0); }, [&](size_t r, size_t j, Fr &x) { ld_words(x, msgs, r * (n - fixed) + j, mont != 0); });
    if (t_words) ld_words(mult, t_words, i, true); else fr_one(mult);
    row_entry(o, v, mult);
    st_words(out_rows, t, o);
}
// grid (L + 2, blocks): block (k, b) sums column k over the rows [b * 256 * run, ..) of the chunk (col_sums.hip.h col_block_sum), a lane its `run` rows with a
// start power of its own, rho^(i0 + its first row).  Column 0 also writes wts[8 i ..] = rho^(i0 + i) and we[8 i ..] = rho^(i0 + i) e_i as canonical words.
// rho_words, e, s, msgs: the caller's form (mont). fixed as in k_bbs_rows: the grid's first dimension is L + fixed.
__global__ void __launch_bounds__(256) k_bbs_col_sums(const uint32_t *__restrict__ e, const uint32_t *__restrict__ s, const uint32_t *__restrict__ msgs, RhoWords rho_words, int mont,
                                                      size_t rows, size_t n, size_t fixed, size_t i0, size_t run, uint32_t *__restrict__ part, uint32_t *__restrict__ wts,
                                                      uint32_t *__restrict__ we) {
    const size_t k = blockIdx.x;
    Fr rho;
    fr_from_words(rho, rho_words.w, mont != 0);
    col_block_sum(k, rows, run, part, [&](size_t lo, size_t cnt, Fr &sum) {
        col_run(rho, i0 + lo, cnt,
                [&](size_t j, Fr &v) {
                    row_value_fixed(v, lo + j, k, fixed, [&](size_t r, Fr &x) { ld_words(x, s, r, mont != 0); },
                                    [&](size_t r, size_t c, Fr &x) { ld_words(x, msgs, r * (n - fixed) + c, mont != 0); });
                },
                [&](size_t j, const Fr &w) {
                    if (k != 0) return;
                    Fr ei, p; ld_words(ei, e, lo + j, mont != 0);
                    fr_mul(p, ei, w);                 // 2 r * 2 r
                    st_words(wts, lo + j, w); st_words(we, lo + j, p);
                },
                sum);
    });
}
#endif

}  // namespace bbsk
