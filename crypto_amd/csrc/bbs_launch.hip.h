// crypto_amd/csrc/bbs_launch.hip.h — host-callable launchers of the BBS+ scalar kernels (k_bbs.hip, bbs_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "col_launch.hip.h"
namespace bbsk {
// How a call is cut.  All of these are UNMEASURED (tests/perf/bbs_timing.py reports what they would be tuned from):
//   BBS_EACH_CHUNK   signatures per chunk of dgpu_bbs_plus_verify_each_g1, at most: the Miller loop's lines and per-step products are 91 KB per signature
//                    (0.37 GB at 4096), the figure dgpu_legogroth16_verify_each settled on for its 115 KB per proof.
//   BBS_BATCH_TERMS  scalars of messages per chunk of dgpu_bbs_plus_verify_batch_g1 (32 MB), and BBS_BATCH_CHUNK its rows at most: the two MSMs over the A_i run per chunk.
//   BBS_COL_RUN      rows per lane of k_bbs_col_sums: col_launch.hip.h's COL_RUN under the name it had while it was set here (k_bbs.hip asserts that they agree);
//                    every other scheme's sums kernel takes COL_RUN.
constexpr size_t BBS_EACH_CHUNK = 4096, BBS_BATCH_TERMS = (size_t)1 << 20, BBS_BATCH_CHUNK = 65536, BBS_COL_RUN = 16;
// rows x n canonical words-of-8, packed, n = L + 2: row i = mult_i (1, s_i, m_i1 .. m_iL); s: rows x 8 words, msgs: rows x L x 8 words packed (mont: ark-ff
// Montgomery form, else any 256-bit value); t_words: mult_i as ark-ff Montgomery words, or NULL for one.  fixed: the columns in front of the messages, 2 for
// BBS+; 1 for the 2023 scheme: n = L + 1, row i = mult_i (1, m_i1 .. m_iL), s_words is not read (NULL)
void launch_bbs_rows(hipStream_t s, const uint32_t *s_words, const uint32_t *msgs, const uint32_t *t_words, int mont, size_t rows, size_t n, size_t fixed, uint32_t *out_rows);
// The chunk [i0, i0 + rows) of a batch: c_k += sum_i rho^(i0 + i) row_ik for the n = L + fixed columns (part: colk::col_part_words(rows, n) words; run_sums: n
// x 10 words, the sums between chunks; first: they start from zero), wts[8 i ..] = rho^(i0 + i), we[8 i ..] = rho^(i0 + i) e_i (canonical words), c_words[8 k
// ..] = -c_k as it stands after this chunk. Two launches: the partial sums of every block, then one lane per column that adds them in block order — no atomics,
// no dependence on the order of execution.
void launch_bbs_columns(hipStream_t s, const uint32_t *e, const uint32_t *s_words, const uint32_t *msgs, const uint32_t rho_words[8], int mont, size_t rows, size_t n, size_t fixed,
                        size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *wts, uint32_t *we, uint32_t *c_words);
}  // namespace bbsk
