// crypto_amd/csrc/acc_pok_launch.hip.h — host-callable launchers of the kernels behind the bulk verification of accumulator proofs (k_acc_pok.hip,
// acc_pok_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace accpk {
// How a call is cut (tests/perf/acc_pok_timing.py reports what they would be tuned from).  Both are UNMEASURED as constants:
//   ACC_POK_EACH_CHUNK   proofs per chunk of the two ..._proofs_verify_each_g1 calls, at most: bbs_pok_launch.hip.h's POK_EACH_CHUNK, for its reason (91 KB of
//                        lines and per-step products per proof).  A non-membership chunk is 8192 segments and 32768 terms a launch of the segmented small MSM
//   ACC_POK_BATCH_CHUNK  proofs per chunk of the two ..._proofs_verify_batch_g1 calls, at most: the variable-base MSM over the chunk's 3 n or 5 n own points
//                        runs per chunk
// A lane of k_acc_pok_col_sums takes col_launch.hip.h's COL_RUN rows.
constexpr size_t ACC_POK_EACH_CHUNK = 4096, ACC_POK_BATCH_CHUNK = 65536;
// kind: 0 membership (3 points A', Abar, T; 2 responses z1, z2; 4 own scalars in 1 segment; 1 shared point V), 1 non-membership (5 points C', Cbar, J, T1, T2;
// 3 responses s_r, s_y, s_d; 8 own scalars in 2 segments; 3 shared points V, P, Q)
constexpr int KIND_MEMBERSHIP = 0, KIND_NON_MEMBERSHIP = 1;
struct KindShape { int pts, resp, own, segs, shared; };
KindShape kind_shape(int kind);
// the proofs of a chunk on the device, in the caller's form (mont: ark-ff Montgomery words, else any 256-bit value): chal rows x 8 words, resp rows x resp x 8 words
struct ProofDev { const uint32_t *chal, *resp; int kind, mont; };
// own: rows x own canonical words-of-8: (z1, -z2, -c, -1), respectively (s_d, -c, -1 | s_r, -s_y, -s_d, -c, -1)
void launch_acc_pok_own(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *own);
// points: rows x pts x 24 words; shared: shared x 24 words (V [, P, Q]) -> own_pts: rows x own x 24 words [V, A', Abar, T], respectively
// [Q, J, T2 | V, C', P, Cbar, T1]; pa: rows x 24 words A' / C', pb: -Abar / -Cbar; skip[0 .. rows) / [rows .. 2 rows) / [2 rows .. 3 rows): the first point,
// the second, J is the identity
void launch_acc_pok_stage(hipStream_t s, const uint32_t *points, const uint32_t *shared, int kind, size_t rows, uint32_t *own_pts, uint32_t *pa, uint32_t *pb, uint8_t *skip);
// seg_inf: segs x rows identity flags of the segment sums; pairing: rows verdict bytes; skip: as the stage kernel wrote it -> status: rows bytes
void launch_acc_pok_verdict(hipStream_t s, const uint8_t *seg_inf, const uint8_t *pairing, const uint8_t *skip, int kind, size_t rows, uint8_t *status);
// The chunk [i0, i0 + rows) of a batch: the coefficients of the shared points += this chunk's share (run_sums: shared x 10 words between chunks; first: from
// zero; part: acc_pok_part_words(rows, kind) words), c_words[8 k ..] = the coefficient of shared point k as it stands (V: sum u z1 / sum u s_r, P: -sum u s_d,
// Q: sum v s_d), wts[(pts i + q) * 8 ..] the weights over the own points, tp / tn[8 i ..] = +- rho^(i0 + i).  Two launches, no atomics.
size_t acc_pok_part_words(size_t rows, int kind);
void launch_acc_pok_columns(hipStream_t s, const ProofDev &in, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *wts,
                            uint32_t *tp, uint32_t *tn, uint32_t *c_words);
}  // namespace accpk
