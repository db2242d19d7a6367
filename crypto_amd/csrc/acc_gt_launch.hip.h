// crypto_amd/csrc/acc_gt_launch.hip.h — host-callable launchers of the kernels behind the bulk verification of the accumulator proofs with a GT commitment
// (k_acc_gt.hip, acc_gt_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace accgt {
// How a call is cut (tests/perf/acc_gt_timing.py reports what they would be tuned from).  Both are UNMEASURED as constants:
//   ACC_GT_EACH_CHUNK   proofs per chunk of the two ..._proofs_verify_each_g1 calls, at most: acc_pok_launch.hip.h's ACC_POK_EACH_CHUNK, for its reason (91 KB of
//                       lines and per-step products per proof).  A non-membership chunk is 32768 segments and 110592 terms a launch of the segmented small MSM
//   ACC_GT_BATCH_CHUNK  proofs per chunk of the two ..._proofs_verify_batch_g1 calls, at most: dock_gt_dev.hip's GT_POW_CHUNK, for its reason (5.4 KB of power
//                       table per R_E); the variable-base MSM over the chunk's 7 n or 11 n own points runs per chunk
// A lane of k_acc_gt_col_sums takes col_launch.hip.h's COL_RUN rows.
constexpr size_t ACC_GT_EACH_CHUNK = 4096, ACC_GT_BATCH_CHUNK = 16384;
// kind: 0 membership (7 points, 5 responses, 17 own scalars in 6 segments, 4 Schnorr checks, 5 columns), 1 non-membership (11 points, 8 responses, 27 own
// scalars in 8 segments, 6 Schnorr checks, 8 columns); g1cols columns close the G1 equation (X, Y, respectively P, K, X, Y), pcols the side against P~ (Z, V
// [, K]), the last one the side against pk (Z)
constexpr int KIND_MEMBERSHIP = 0, KIND_NON_MEMBERSHIP = 1;
struct KindShape { int pts, resp, own, segs, checks, g1cols, pcols; };
KindShape kind_shape(int kind);
// the ends of a row's segments in own scalars (segs of them)
void kind_seg_ends(int kind, unsigned ends[8]);
// the proofs of a chunk on the device, in the caller's form (mont: ark-ff Montgomery words, else any 256-bit value): chal rows x 8 words, resp rows x resp x 8 words
struct ProofDev { const uint32_t *chal, *resp; int kind, mont; };
// own: rows x own canonical words-of-8 (acc_gt_kernels.hip.h own_code)
void launch_acc_gt_own(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *own);
// points: rows x pts x 24 words; shared: 6 x 24 words V, X, Y, Z, K, P (those the kind does not use: any) -> bases: rows x own x 24 words in segment order
void launch_acc_gt_stage(hipStream_t s, const uint32_t *points, const uint32_t *shared, int kind, size_t rows, uint32_t *bases);
// sums: segs x rows normalised (x, y, z) of 36 words, inf: their identity flags -> pa: rows x 24 words q (against pk), pb: p (against P~), skip[0 .. rows) /
// [rows .. 2 rows): that side is the identity
void launch_acc_gt_sides(hipStream_t s, const uint32_t *sums, const uint8_t *inf, int kind, size_t rows, uint32_t *pa, uint32_t *pb, uint8_t *skip);
// seg_inf: segs x rows identity flags of the segment sums; gt: rows x 144 words, the pairings' values; r_e: rows x 144 words, the proofs' own -> status: rows bytes
void launch_acc_gt_verdict(hipStream_t s, const uint8_t *seg_inf, const uint32_t *gt, const uint32_t *r_e, int kind, size_t rows, uint8_t *status);
// The chunk [i0, i0 + rows) of a batch: the coefficients of the shared points += this chunk's share (run_sums: columns x 10 words between chunks; first: from
// zero; part: acc_gt_part_words(rows, kind) words), c_words[8 k ..] = the coefficient of column k as it stands (the columns of the two sides negated),
// wts[(pts i + q) * 8 ..] the weights over the own points, wp / wq / tp[8 i ..] = t s_y, t c, t = rho^(i0 + i).  Two launches, no atomics.
size_t acc_gt_part_words(size_t rows, int kind);
void launch_acc_gt_columns(hipStream_t s, const ProofDev &in, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *wts,
                           uint32_t *wp, uint32_t *wq, uint32_t *tp, uint32_t *c_words);
}  // namespace accgt
