/* include/dock_gpu_acc_gt.h — the accumulator proofs with a GT commitment (the reference's vb_accumulator/src/proofs.rs: what the statements VBAccumulatorMembership,
 * VBAccumulatorNonMembership and, through kb_universal_accumulator/proofs.rs, KBUniversalAccumulatorMembership / KBUniversalAccumulatorNonMembership carry) verified in
 * bulk: the C ABI of crypto_amd/libdock_gpu_acc_gt.so beyond include/dock_gpu.h.  Conventions, error codes and DGPU_G2_PREPARED_WORDS: include/dock_gpu.h. */
#ifndef DOCK_GPU_ACC_GT_H
#define DOCK_GPU_ACC_GT_H
#include "dock_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- MembershipProof / NonMembershipProof of proofs.rs in bulk (crypto_amd/csrc/dock_acc_gt.hip) ----
 * These four calls are NOT part of libdock_gpu.so: they are served by libdock_gpu_acc_gt.so, the product's objects plus dock_acc_gt.o and k_acc_gt.o — a library
 * of its own beside the product, as libdock_gpu_smc.so is, with its own contexts: bring it up with its own dgpu_init.  It exports everything include/dock_gpu.h
 * declares as well.
 *
 * One call serves ONE accumulator value V and one key, and n proofs against them:
 *   accumulator_xy    V: 12 words, affine Montgomery coordinates; all-zero words are the identity
 *   prk_xy            the proving key: membership 3 x 12 words X, Y, Z; non-membership 4 x 12 words X, Y, Z, K
 *   p_xy              non-membership: params.P
 *   pk_pc, ptilde_pc  the prepared coefficients (DGPU_G2_PREPARED_WORDS words each, dgpu_g2_prepare) of pk = Q~ and of P~
 *   points            membership: n x 7 x 12 words, E_C, T_sigma, T_rho (the randomized witness), R_sigma, R_rho, R_delta_sigma, R_delta_rho (the Schnorr commitment)
 *                     of proof i at points + 84 i; non-membership: n x 11 x 12 words, those seven, then E_d, E_d_inv, R_A, R_B, of proof i at points + 132 i
 *   r_e               n x 72 words: the proofs' GT elements R_E, laid out as dgpu_fp12_pow takes them (ark-ff Fp12: twelve base-field elements of 6 Montgomery
 *                     words, canonical, i.e. below p — what serialization with validation yields)
 *   responses         membership: n x 5 scalars s_sigma, s_rho, s_delta_sigma, s_delta_rho, s_y; non-membership: n x 8, those five, then s_u, s_v, s_w.  A partial
 *                     proof (verify_partial, resp_for_element) needs no path of its own: the caller writes resp_for_element into s_y; the reference's
 *                     MissingSchnorrResponseForElement (neither is there) stays with the caller
 *   challenge         n scalars, one per proof, computed by the caller (hashing stays on the host).  montgomery != 0: ark-ff `&[Fr]` limbs; else canonical
 *                     words, any 256-bit value counting modulo r — responses and `random` alike
 * The reference's checks in the order it returns their errors (proofs.rs:1516-1580, :890-996, :697-724), c the proof's challenge:
 *   non-membership only   s_u P + s_v K - c E_d - R_A = O                            else E_d_ResponseInvalid
 *                         s_w K + s_u E_d_inv - c P - R_B = O                        else E_d_inv_ResponseInvalid
 *   both                  s_sigma X - c T_sigma - R_sigma = O                        else SigmaResponseInvalid
 *                         s_rho Y - c T_rho - R_rho = O                              else RhoResponseInvalid
 *                         s_y T_sigma - s_delta_sigma X - R_delta_sigma = O          else DeltaSigmaResponseInvalid
 *                         s_y T_rho - s_delta_rho Y - R_delta_rho = O                else DeltaRhoResponseInvalid
 *                         e(p, P~) e(q, pk) = R_E                                    else PairingResponseInvalid
 *                           p = s_y E_C - (s_delta_sigma + s_delta_rho) Z - c V  [+ c E_d - s_v K for non-membership],   q = -(s_sigma + s_rho) Z + c E_C
 * The reference makes no non-zero checks on these proofs: an identity among the points of a proof that otherwise holds verifies, and an identity p or q
 * contributes the factor one to the pairing.
 *
 * The two ..._verify_each_g1 calls write status[i] = 0 (verified) or the number of the FIRST check that fails, counted from 1 in the order above: membership
 * 1 .. 4 the Schnorr checks and 5 the pairing, non-membership 1 .. 6 and 7.  Per chunk of rows one device pipeline, no host round trip between its stages:
 * the own scalars (k_acc_gt_own), the bases with the shared points copied into every row (k_acc_gt_stage), six segments a row of the segmented small MSM
 * (3, 3, 3, 3, 3, 2 terms), respectively eight (4, 4, 3, 3, 3, 3, 5, 2), whose last two sums become the two sides of the row's pairing (k_acc_gt_sides), the lines
 * of the two prepared points shared by every row, the Miller loops' tail and the final exponentiation, which leaves the pairing values on the device, and
 * k_acc_gt_verdict, which compares each value with the row's own R_E; only the n status bytes come back.
 *
 * The two ..._verify_batch_g1 calls: ONE verdict under rho = random (rho = 0 mod r: DGPU_E_BADARG, decided on the host).  With J = 4 (membership) or 6
 * (non-membership), Schnorr check j (from 0, in the order above) of proof i is weighed by rho^(J i + j), the pairing and R_E of proof i by t_i = rho^i, and
 * *ok = 1 iff
 *     the sum of all weighed Schnorr checks is the identity                                      (ONE G1 equation), and
 *     e(sum t_i p_i, P~) e(sum t_i q_i, pk) = prod R_E_i^(t_i)
 * — the coefficients of the shared points (X, Y [, P, K] in the G1 equation; Z, V [, K] and Z in the two sides) are column sums, every weight is computed on the
 * device (k_acc_gt_col_sums, k_col_finish: two passes, no atomics), per chunk one variable-base MSM over the chunk's 7 n (11 n) own points and one (two) per
 * side, the GT product by the GT power kernel and a product fold (chunk partials are multiplied on the host), then small MSMs over the shared points and one
 * two-pair Miller loop and final exponentiation whose value is compared with the GT product.  A failing G1 equation returns before any pairing.  n = 0 gives
 * *ok = 1.  Soundness: as polynomials in rho the G1 equation has degree below J n and the GT equation degree below n, so for a random rho a batch with a
 * failing proof passes with probability at most J n / r, respectively n / r, per equation.  rho = 1 adds the rows up unweighted: errors that cancel between rows
 * then pass, in G1 and in GT alike, as they would in the reference's checker with that scalar.
 *
 * All four take the points as members of the prime-order subgroup and every R_E as a member of GT, as the reference does after deserialising with validation:
 * validate untrusted ones first (dgpu_g1_validate_batch, dgpu_gt_in_subgroup_device).  n = 0 is DGPU_OK without touching a device or any pointer; with n > 0 a
 * NULL pointer or n >= 2^31 is DGPU_E_BADARG before the device is looked at; then DGPU_E_NODEVICE.  Never DGPU_E_TOO_SMALL.  Thread-safe; one slot per call; a
 * second call of a shape allocates nothing.  Chunks: each 4096 rows, batch 16384 (both provisional, not measured); the development surface's
 * dgpu_set_many_chunk_rows cuts both.  Nothing secret passes through.  Stage timers acc.gt_own, acc.gt_stage, acc.gt_sides, acc.gt_verdict, acc.gt_columns,
 * gt.multi_pow, gt.fold beside bbs.lines .. bbs.final_exp (the shared pairing tail) and those of the MSMs. */
int32_t dgpu_accumulator_gt_membership_proofs_verify_each_g1(const uint64_t accumulator_xy[12], const uint64_t prk_xy[36] /* X, Y, Z */, const uint64_t *pk_pc,
                                                             const uint64_t *ptilde_pc, const uint64_t *points /* n*84 */, const uint64_t *r_e /* n*72 */,
                                                             const uint64_t *responses /* n*20 */, const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery,
                                                             uint8_t *status /* n */);
int32_t dgpu_accumulator_gt_membership_proofs_verify_batch_g1(const uint64_t accumulator_xy[12], const uint64_t prk_xy[36] /* X, Y, Z */, const uint64_t *pk_pc,
                                                              const uint64_t *ptilde_pc, const uint64_t *points /* n*84 */, const uint64_t *r_e /* n*72 */,
                                                              const uint64_t *responses /* n*20 */, const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery,
                                                              const uint64_t random[4], int32_t *ok);
int32_t dgpu_accumulator_gt_non_membership_proofs_verify_each_g1(const uint64_t accumulator_xy[12], const uint64_t p_xy[12], const uint64_t prk_xy[48] /* X, Y, Z, K */,
                                                                 const uint64_t *pk_pc, const uint64_t *ptilde_pc, const uint64_t *points /* n*132 */,
                                                                 const uint64_t *r_e /* n*72 */, const uint64_t *responses /* n*32 */, const uint64_t *challenge /* n*4 */,
                                                                 size_t n, int32_t montgomery, uint8_t *status /* n */);
int32_t dgpu_accumulator_gt_non_membership_proofs_verify_batch_g1(const uint64_t accumulator_xy[12], const uint64_t p_xy[12], const uint64_t prk_xy[48] /* X, Y, Z, K */,
                                                                  const uint64_t *pk_pc, const uint64_t *ptilde_pc, const uint64_t *points /* n*132 */,
                                                                  const uint64_t *r_e /* n*72 */, const uint64_t *responses /* n*32 */, const uint64_t *challenge /* n*4 */,
                                                                  size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
