// crypto_amd/csrc/smc_launch.hip.h — host-callable launchers of the kernels behind the bulk verification of range proofs over weak-BB signatures (k_smc.hip,
// smc_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace smck {
// How a call is cut (tests/perf/smc_timing.py reports what they would be tuned from).  Both are UNMEASURED as constants:
//   SMC_EACH_SLICES   two-pair pairing slices per chunk of dgpu_smc_range_proofs_verify_each_g1, at most: a chunk is the largest count of proofs with
//                     rows S l <= 4096 (the pairing tail's 4096-row size, 91 KB of lines and per-step products a slice), at least one proof; with l = 0 the
//                     same bound falls on the rows S segments
//   SMC_BATCH_EQS     equations per chunk of dgpu_smc_range_proofs_verify_batch_g1, at most (at least one proof): the variable-base MSM over the chunk's
//                     own points (fewer than 3 per equation) runs per chunk
// A lane of k_smc_col_sums takes col_launch.hip.h's COL_RUN equations.
constexpr size_t SMC_EACH_SLICES = 4096, SMC_BATCH_EQS = 16384;
constexpr int SMC_MAX_L = 64;
constexpr size_t SMC_STMT_CONSTS = 6;       // the statement on the device: (a, b, e) of side 0, of side 1 (zeros for one side), then w_0 .. w_(l-1); 8 words each
// the proofs of a chunk on the device, in the caller's form (mont: ark-ff Montgomery words, else any 256-bit value): chal rows x 8 words, zr rows x S x 8,
// z rows x S l x 2 x 8 (z1, z2), stmt (6 + l) x 8
struct ProofDev { const uint32_t *chal, *zr, *z, *stmt; int sides, l, mont; };
// own: rows x M x 4 canonical words-of-8, M = S (l + 1): (a_s c, b_s c + sum_j w_j z2_sj, e_s zr_s, -1) per side, then (z1, -z2, -c, -1) per digit
void launch_smc_own(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *own);
// commitments: rows x 24 words; side_points: rows x S x 24; digit_points: rows x S l x 3 x 24; shared: 3 x 24 words (g1, g, h) -> bases: rows x M x 4 x 24 words,
// [C, g, h, D_s] per side then [g1, A', Abar, T] per digit; pa: rows x S l x 24 words A', pb: -Abar; skip[0 .. slices) / [slices .. 2 slices): A', Abar is the identity
void launch_smc_stage(hipStream_t s, const uint32_t *commitments, const uint32_t *side_points, const uint32_t *digit_points, const uint32_t *shared, int sides, int l, size_t rows,
                      uint32_t *bases, uint32_t *pa, uint32_t *pb, uint8_t *skip);
// seg_inf: rows x M identity flags of the segment sums; pairing: rows x S l verdict bytes (merged: rows, one per proof); skip: as the stage kernel wrote it
// -> status: rows bytes, detail: rows int32
void launch_smc_verdict(hipStream_t s, const uint8_t *seg_inf, const uint8_t *pairing, const uint8_t *skip, int sides, int l, bool merged, size_t rows, uint8_t *status,
                        int32_t *detail);
// The merged form of the each call.  random: rows x 8 words in the caller's form -> tw: 2 x rows x S l canonical words-of-8, random_i^d twice over (the scalars
// of the proof's segment over its A', then of the one over its -Abar)
void launch_smc_merge_weights(hipStream_t s, const uint32_t *random, int sides, int l, int mont, size_t rows, uint32_t *tw);
// sums: 2 rows normalised Jacobian results of 36 words (the rows' sums over A', then over -Abar) with their identity flags inf -> pa, pb: rows x 24 words,
// skip[0 .. rows) / [rows .. 2 rows)
void launch_smc_merged_sides(hipStream_t s, const uint32_t *sums, const uint8_t *inf, size_t rows, uint32_t *pa, uint32_t *pb, uint8_t *skip);
// The chunk of `rows` proofs from proof i0 on of a batch: the coefficients of g1, g, h += this chunk's share (run_sums: 3 x 10 words between chunks; first: from
// zero; part: smc_part_words(rows, sides, l) words), c_words[8 k ..] = the coefficient of shared point k as it stands; w_side[8 i ..] the weights over the C_i then
// (from 8 rows on) over the D_is, w_digit[8 (3 slice + q) ..] over A', Abar, T, tp / tn[8 slice ..] = +- rho^(i0 S l + slice).  own: launch_smc_own's output.
// Two launches, no atomics.
size_t smc_part_words(size_t rows, int sides, int l);
void launch_smc_columns(hipStream_t s, const uint32_t *own, const uint32_t rho_words[8], int sides, int l, int mont, size_t rows, size_t i0, bool first, uint32_t *part,
                        uint32_t *run_sums, uint32_t *w_side, uint32_t *w_digit, uint32_t *tp, uint32_t *tn, uint32_t *c_words);
}  // namespace smck
