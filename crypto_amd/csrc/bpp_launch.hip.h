// crypto_amd/csrc/bpp_launch.hip.h — host-callable launchers of the kernels behind the bulk verification of Bulletproofs++ range proofs (k_bpp.hip,
// bpp_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace bppk {
// How a call is cut (tests/perf/bpp_timing.py reports what they would be tuned from).  Both are UNMEASURED as constants:
//   BPP_EACH_CHUNK    proofs per chunk of dgpu_bpp_range_proofs_verify_each_g1, at most, beside the many-row kernels' own rule for rows of 9 + NG terms
//   BPP_BATCH_POINTS  own points per chunk of dgpu_bpp_range_proofs_verify_batch_g1, at most (at least one proof): the variable-base MSM over them runs per chunk
// A lane of k_bpp_col_sums takes col_launch.hip.h's COL_RUN proofs.
constexpr size_t BPP_EACH_CHUNK = 4096, BPP_BATCH_POINTS = (size_t)1 << 16;
// what a shape comes to (bpp_kernels.hip.h make_shape): ok = 0 for anything outside base in {2, 4, 8, 16}, num_bits a power of two in [log2 base, 64], m a power
// of two in [1, 8], NG a power of two
struct ShapeInfo { int ok; size_t NG, K, own, shared; };      // own = m + 4 + 2 K, shared = 9 + NG
ShapeInfo bpp_shape(uint32_t base, uint32_t num_bits, uint32_t m);
size_t bpp_rec_words(size_t rows);           // words of the record of a chunk
// the proofs of a chunk on the device, in the caller's form (mont: ark-ff Montgomery words, else any 256-bit value): chal rows x (7 + K) x 8 words
// (e, x, y, r, lambda, delta, t, gamma_0 ..), l_n rows x 2 x 8 (l0, n0)
struct ProofDev { const uint32_t *chal, *l_n; uint32_t base, num_bits, m; int mont; };
// -> rec: bpp_rec_words(rows); own: rows x own_stride canonical words-of-8, own_stride = own (-2 t^3 lambda^k .., -t, -delta, -t^2, -1/t, -gamma_j .., 1 - gamma_j^2 ..)
// or own + 1 (a one behind them: the scalar of P_i); bad: rows bytes, 1 where one of t, r, e + k (k < base) is zero
void launch_bpp_consts(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *rec, size_t own_stride, uint32_t *own, uint8_t *bad);
// rec -> out_rows: rows x (9 + NG) canonical words-of-8, packed: the rows over [G, H_0 .. H_7, G_0 ..]
void launch_bpp_shared(hipStream_t s, const ProofDev &in, size_t rows, uint32_t *rec, uint32_t *out_rows);
// values: rows x m x 24 words; round_points: rows x 4 x 24 (D, M, R, S); wnla_points: rows x 2 K x 24 (X_0 .., R_0 ..); p: rows x 24 with identity flags p_inf
// -> bases: rows x (own + 1) x 24 words
void launch_bpp_stage(hipStream_t s, const ProofDev &in, const uint32_t *values, const uint32_t *round_points, const uint32_t *wnla_points, const uint32_t *p, const uint8_t *p_inf,
                      size_t rows, uint32_t *bases);
void launch_bpp_verdict(hipStream_t s, const uint8_t *seg_inf, const uint8_t *bad, size_t rows, uint8_t *status);
// The chunk of `rows` proofs from proof i0 on of a batch: the coefficients of the 9 + NG shared points += this chunk's share (run_sums: (9 + NG) x 10 words between
// chunks; first: from zero; part: bpp_part_words words), c_words[8 k ..] = the coefficient of shared point k as it stands; wts: rows x own canonical words-of-8 in
// the order [over values | over round_points | over wnla_points], own scalar times rho^(i0 + i).  rows_sc: launch_bpp_shared's output, own: launch_bpp_consts's with
// own_stride = own.  Two launches, no atomics.
size_t bpp_part_words(size_t rows, size_t shared);
void launch_bpp_columns(hipStream_t s, const ProofDev &in, const uint32_t *rows_sc, const uint32_t *own, const uint32_t rho_words[8], size_t rows, size_t i0, bool first, uint32_t *part,
                        uint32_t *run_sums, uint32_t *wts, uint32_t *c_words);
}  // namespace bppk
