// crypto_amd/csrc/bbs_pok_launch.hip.h — host-callable launchers of the kernels behind the bulk verification of BBS+ proofs of knowledge (k_bbs_pok.hip,
// bbs_pok_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace bbspk {
// How a call is cut (tests/perf/bbs_pok_timing.py reports what they would be tuned from).  POK_EACH_CHUNK was seen at 2048 (3.2 x slower at 16384
// proofs: the Fp12 chains of the pairing check cost more per 2048 elements than per 4096) and at 4096, nowhere else; POK_BATCH_CHUNK is UNMEASURED:
//   POK_EACH_CHUNK   proofs per chunk of dgpu_bbs_plus_pok_verify_each_g1, at most: BBS_EACH_CHUNK's figure, for its reason (91 KB of lines and per-step products per
//                    proof).  The two segments per proof make 8192 segments and 28672 terms a launch of the segmented small MSM: 0.12 GB of window sums, 51 MB of table
//   POK_BATCH_CHUNK  proofs per chunk of dgpu_bbs_plus_pok_verify_batch_g1, at most, beside bbs_launch.hip.h's BBS_BATCH_TERMS scalars of values: the
//                    variable-base MSM over the chunk's 5 n own points runs per chunk
// A lane of k_bbs_pok_col_sums takes col_launch.hip.h's COL_RUN rows.
constexpr size_t POK_EACH_CHUNK = 4096, POK_BATCH_CHUNK = 65536;
// the proofs of a chunk on the device, in the caller's form (mont: ark-ff Montgomery words, else any 256-bit value): chal rows x 8 words, fixed rows x 4 x 8
// words (z1, z2, z3, z4), vals rows x L x 8 words packed, rev rows x L bytes
struct PokDev { const uint32_t *chal, *fixed, *vals; const uint8_t *rev; size_t L; int mont; };
// out_rows: rows x (L + 2) canonical words-of-8, row i = (c_i, z4_i, y_i1 .. y_iL); own: rows x 7 canonical words-of-8, (z1, z2, -c, c, -1 | z3, -1)
void launch_pok_rows(hipStream_t s, const PokDev &in, size_t rows, uint32_t *out_rows, uint32_t *own);
// points: rows x 5 x 24 words (A', Abar, d, T1, T2) -> own_pts: rows x 7 x 24 words [A', h_0, Abar, d, T1 | d, T2], pa: rows x 24 words A', pb: -Abar,
// skip[0 .. rows) / skip[rows .. 2 rows): A' / Abar is the identity
void launch_pok_stage(hipStream_t s, const uint32_t *points, const uint32_t h0[24], size_t rows, uint32_t *own_pts, uint32_t *pa, uint32_t *pb, uint8_t *skip);
// seg: 2 rows normalised Jacobian results (36 words each: the first check's sum, then z3 d - T2) with flags seg_inf; b: rows x 24 words P_i with b_inf;
// pairing: rows verdict bytes; a_inf: rows bytes -> status: rows bytes
void launch_pok_verdict(hipStream_t s, const uint32_t *seg, const uint8_t *seg_inf, const uint32_t *b, const uint8_t *b_inf, const uint8_t *pairing, const uint8_t *a_inf, size_t rows,
                        uint8_t *status);
// The chunk [i0, i0 + rows) of a batch: C_k += this chunk's share for the n = L + 2 columns (run_sums: n x 10 words between chunks; first: from zero; part:
// colk::col_part_words(rows, n) words), c_words[8 k ..] = C_k as it stands, w5[(5 i + q) * 8 ..] the weights over the own points, tp / tn[8 i ..] = +- rho^(i0 + i).
// Two launches, no atomics.
void launch_pok_columns(hipStream_t s, const PokDev &in, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *w5,
                        uint32_t *tp, uint32_t *tn, uint32_t *c_words);
}  // namespace bbspk
