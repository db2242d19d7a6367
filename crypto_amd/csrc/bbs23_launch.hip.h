// crypto_amd/csrc/bbs23_launch.hip.h — host-callable launchers of the kernels behind the bulk verification of BBS (2023) proofs of knowledge (k_bbs23.hip,
// bbs23_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace bbs23k {
// How a call is cut (tests/perf/bbs23_timing.py reports what they would be tuned from).  Both are UNMEASURED as constants:
//   BBS23_EACH_CHUNK   proofs per chunk of the two ..._verify_each_g1 calls, at most: bbs_pok_launch.hip.h's POK_EACH_CHUNK, for its reason (91 KB of lines and
//                      per-step products per proof).  A CDL chunk is 8192 segments and 24576 terms a launch of the segmented small MSM, an IETF chunk 4096 and 12288
//   BBS23_BATCH_CHUNK  proofs per chunk of the two ..._verify_batch_g1 calls, at most, beside bbs_launch.hip.h's BBS_BATCH_TERMS scalars of values: the
//                      variable-base MSM over the chunk's 5 n or 3 n own points runs per chunk
// A lane of k_bbs23_col_sums takes col_launch.hip.h's COL_RUN rows.
constexpr size_t BBS23_EACH_CHUNK = 4096, BBS23_BATCH_CHUNK = 65536;
// kind: 0 CDL (proof_23_cdl.rs: 5 points Abar, Bbar, d, T1, T2; 3 responses z1, z2, z3; 6 own scalars in 2 segments), 1 IETF (proof_23_ietf.rs: 3 points
// Abar, Bbar, T; 2 responses z_a, z_b; 3 own scalars in 1 segment)
constexpr int KIND_CDL = 0, KIND_IETF = 1;
struct KindShape { int pts, resp, own, segs; };
KindShape kind_shape(int kind);
// the proofs of a chunk on the device, in the caller's form (mont: ark-ff Montgomery words, else any 256-bit value): chal rows x 8 words, resp rows x resp x 8
// words, vals rows x L x 8 words packed, rev rows x L bytes
struct ProofDev { const uint32_t *chal, *resp, *vals; const uint8_t *rev; size_t L; int kind, mont; };
// out_rows: rows x (L + 1) canonical words-of-8, row i = (c_i, y_i1 .. y_iL); own: rows x own canonical words-of-8, (z1, z2, -c, -1 | z3, -1), respectively
// (z_a, z_b, -1)
void launch_bbs23_rows(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *out_rows, uint32_t *own);
// points: rows x pts x 24 words -> own_pts: rows x own x 24 words [Abar, d, Bbar, T1 | d, T2], respectively [Abar, Bbar, T]; pa: rows x 24 words Abar,
// pb: -Bbar; skip[0 .. rows) / skip[rows .. 2 rows): Abar / Bbar is the identity
void launch_bbs23_stage(hipStream_t s, const uint32_t *points, int kind, size_t rows, uint32_t *own_pts, uint32_t *pa, uint32_t *pb, uint8_t *skip);
// seg: segs x rows normalised Jacobian results (36 words each) with flags seg_inf; b: rows x 24 words P_i with b_inf; pairing: rows verdict bytes; a_inf: rows
// bytes -> status: rows bytes
void launch_bbs23_verdict(hipStream_t s, const uint32_t *seg, const uint8_t *seg_inf, const uint32_t *b, const uint8_t *b_inf, const uint8_t *pairing, const uint8_t *a_inf, int kind,
                          size_t rows, uint8_t *status);
// The chunk [i0, i0 + rows) of a batch: C_k += this chunk's share for the n = L + 1 columns (run_sums: n x 10 words between chunks; first: from zero; part:
// colk::col_part_words(rows, n) words), c_words[8 k ..] = C_k as it stands, wts[(pts i + q) * 8 ..] the weights over the own points, tp / tn[8 i ..] =
// +- rho^(i0 + i).  Two launches, no atomics.
void launch_bbs23_columns(hipStream_t s, const ProofDev &in, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part, uint32_t *run_sums, uint32_t *wts,
                          uint32_t *tp, uint32_t *tn, uint32_t *c_words);
}  // namespace bbs23k
