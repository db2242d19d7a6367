/* include/dock_gpu_smc.h — range proofs over weak-BB signatures (the reference's smc_range_proof crate: BoundCheckSmc) verified in bulk: the C ABI of
 * crypto_amd/libdock_gpu_smc.so beyond include/dock_gpu.h.  Conventions, error codes and DGPU_G2_PREPARED_WORDS: include/dock_gpu.h. */
#ifndef DOCK_GPU_SMC_H
#define DOCK_GPU_SMC_H
#include "dock_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- CLSRangeProof / CCSArbitraryRangeProof in bulk (crypto_amd/csrc/dock_smc.hip) ----
 * These two calls are NOT part of libdock_gpu.so: they are served by libdock_gpu_smc.so, the product's objects plus dock_smc.o and k_smc.o — a library of its own
 * beside the product, as libdock_gpu_saver.so is, with its own contexts: bring it up with its own dgpu_init.  It exports everything include/dock_gpu.h declares
 * as well.
 *
 * One call serves ONE statement — (min, max, base), the weak-BB parameters g1, g2, pk and the commitment key (g, h) — and n proofs of it.  The statement arrives
 * as its constants: sides S (1: CLSRangeProof, cls_range_proof/range_proof_cdh.rs; 2: CCSArbitraryRangeProof, ccs_range_proof/arbitrary_range_cdh.rs, side 0
 * the min half and side 1 the max half), the digits per side l (0 <= l <= 64), the weights w_j (j < l) and per side (a_s, b_s, e_s); crypto_amd.smc_range_proof
 * derives them from (min, max, base) by the reference's rules.  Proof i holds a commitment C_i, a challenge c_i, per side a point D_is and a response zr_is, and
 * per digit d = s l + j (side-major) the points A', Abar, T and the responses z1 (over g1), z2 (over -A') of short_group_sig/src/weak_bb_sig_pok_cdh.rs.  The
 * reference's checks:
 *   per side s     a_s c_i C_i + (b_s c_i + sum_j w_j z2_isj) g + e_s zr_is h - D_is = O                        else InvalidRangeProof
 *   per digit      (k = 1) A' is not the identity; (k = 2) z1 g1 - z2 A' - c_i Abar - T = O; (k = 3) e(A', pk) e(-Abar, g2) = 1      else ShortGroupSig(InvalidProof)
 * G1 points are affine Montgomery words (zero words: the identity), taken as members of the subgroup; scalars are canonical words, or ark-ff Montgomery words
 * when `montgomery` is set (the statement's constants and `random` too); pk_pc and g2_pc are prepared coefficients (dgpu_g2_prepare).
 *
 * dgpu_smc_range_proofs_verify_each_g1 writes per proof status[i] (and detail[i] when detail is not NULL):
 *   0, 0           verified
 *   1, s + 1       the commitment equation of side s failed (the first such side).  It wins over any bad digit
 *   2, 4 q + k     the digit at position q of the reference's order of verification (CLS: q = j; CCS: min[0], max[0], min[1], .. i.e. q = 2 j + s) failed its check
 *                  k; the smallest 4 q + k is reported
 * random == NULL is this exact form.  random != NULL (n scalars, one per proof, each non-zero modulo r, else DGPU_E_BADARG) is the merged form, the mirror of
 * verify_given_randomized_pairing_checker with one checker per proof: the commitment equations and the checks k = 1, k = 2 as above, and the proof's pairings
 * as ONE two-pair check e(sum_d t_d A'_d, pk) e(-sum_d t_d Abar_d, g2) = 1 with t_d = random_i^d in the order of the reference's add_sources (d side-major: CLS
 * the digits' order; CCS all of min, then all of max).  Its failure is status 3, detail 0, reported when nothing above failed; a proof whose pairing errors
 * cancel under random_i passes, with probability at most S l / r over random_i.  With l = 0 there is no pairing and random is only checked.
 *
 * dgpu_smc_range_proofs_verify_batch_g1 gives one verdict under rho = random (non-zero modulo r, else DGPU_E_BADARG): *ok = 0 at once if any A' is the identity
 * (decided on the zero words); else equation m of proof i (m = s for the sides, then m = S + d for the digits; M = S (l + 1) a proof) is weighed by
 * rho^(i M + m) and the pairing of digit d by rho^(i S l + d), and *ok = 1 iff the weighted sum of all G1 equations is the identity and
 * e(sum t A', pk) e(-sum t Abar, g2) = 1.  An invalid batch passes with probability at most n M / r over rho (the degree of either polynomial in rho is below
 * n M).  An empty batch verifies.
 *
 * n = 0 returns DGPU_OK without looking at anything else.  Then a NULL pointer (weights, digit_points and digit_responses may be NULL when l = 0; detail always),
 * sides outside {1, 2}, l > 64 and n >= 2^31 are DGPU_E_BADARG before the device is looked at; then DGPU_E_NODEVICE.  Never DGPU_E_TOO_SMALL.  Thread-safe; one
 * slot per call.  Chunks: the each call takes the largest count of proofs with rows S l <= 4096 two-pair pairing slices (l = 0: rows S <= 4096 segments), at
 * least one; the batch call the largest with rows M <= 16384; dgpu_set_many_chunk_rows of the development surface cuts the proofs per chunk of both further.  Stage
 * timers smc.own, smc.stage, smc.verdict, smc.merge_weights, smc.merged_sides (the merged form), smc.columns (the batch) beside msm.* and bbs.*. */
int32_t dgpu_smc_range_proofs_verify_each_g1(const uint64_t g1_xy[12], const uint64_t ck_g_xy[12], const uint64_t ck_h_xy[12], const uint64_t *pk_pc, const uint64_t *g2_pc,
                                             int32_t sides, size_t l, const uint64_t *weights /* l*4 */, const uint64_t *side_consts /* sides*3*4: a, b, e */,
                                             const uint64_t *commitments /* n*12 */, const uint64_t *digit_points /* n*sides*l*36: A', Abar, T */,
                                             const uint64_t *digit_responses /* n*sides*l*8: z1, z2 */, const uint64_t *side_points /* n*sides*12 */,
                                             const uint64_t *side_responses /* n*sides*4 */, const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery,
                                             const uint64_t *random /* NULL */, uint8_t *status /* n */, int32_t *detail /* n or NULL */);
int32_t dgpu_smc_range_proofs_verify_batch_g1(const uint64_t g1_xy[12], const uint64_t ck_g_xy[12], const uint64_t ck_h_xy[12], const uint64_t *pk_pc, const uint64_t *g2_pc,
                                              int32_t sides, size_t l, const uint64_t *weights /* l*4 */, const uint64_t *side_consts /* sides*3*4: a, b, e */,
                                              const uint64_t *commitments /* n*12 */, const uint64_t *digit_points /* n*sides*l*36: A', Abar, T */,
                                              const uint64_t *digit_responses /* n*sides*l*8: z1, z2 */, const uint64_t *side_points /* n*sides*12 */,
                                              const uint64_t *side_responses /* n*sides*4 */, const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery,
                                              const uint64_t random[4], int32_t *ok);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
