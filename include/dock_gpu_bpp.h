/* include/dock_gpu_bpp.h — Bulletproofs++ range proofs (the reference's bulletproofs_plus_plus crate: BoundCheckBpp) verified in bulk: the C ABI of
 * crypto_amd/libdock_gpu_bpp.so beyond include/dock_gpu.h.  Conventions and error codes: include/dock_gpu.h. */
#ifndef DOCK_GPU_BPP_H
#define DOCK_GPU_BPP_H
#include "dock_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- Proof::verify of range_proof.rs in bulk (crypto_amd/csrc/dock_bpp.hip) ----
 * These two calls are NOT part of libdock_gpu.so: they are served by libdock_gpu_bpp.so, the product's objects plus dock_bpp.o and k_bpp.o — a library of its own
 * beside the product, as libdock_gpu_saver.so and libdock_gpu_smc.so are, with its own contexts: bring it up with its own dgpu_init.  It exports everything
 * include/dock_gpu.h declares as well.
 *
 * One call serves ONE shape (base, num_bits, m values a proof) over ONE setup and n proofs of it.  With bb = log2 base, dp = num_bits / bb, D = dp m,
 * NG = max(dp, base) m and K = max(3, log2 NG), the setup is a resident G1 bases handle (dgpu_bases_upload_g1) of exactly 9 + NG points
 * [G, H_0 .. H_7, G_0 .. G_(NG-1)].  Proof i holds the points V_0 .. V_(m-1) (values), D, M, R, S (round_points, in this order), X_0 .. X_(K-1) then
 * R_0 .. R_(K-1) (wnla_points), the scalars l0, n0 (l_n: the weighted-norm linear argument's l and n, one element each after K rounds) and its Fiat-Shamir
 * challenges e, x, y, r, lambda, delta, t, gamma_0 .. gamma_(K-1), which the caller derives (range_proof.rs:86-131, weighted_norm_linear_argument.rs:413-418;
 * crypto_amd.bpp_range_proof.challenges): in proof_system the transcript is shared with the other statements of a presentation.  With q = r^2 the proof
 * verifies iff
 *   (v - g_off) G + sum_{k<8} l0 hm_k H_k + sum_{k<NG} (n0 gm_k - pub_k) G_k
 *     - sum_j gamma_j X_j - sum_j (gamma_j^2 - 1) R_j - sum_{k<m} 2 t^3 lambda^k V_k - S / t - delta M - t D - t^2 R = O
 * where hm_k = prod_{j<3, bit j of k} gamma_j, gm_k = prod_{j<log2 NG} (bit j of k ? gamma_j : r^(2^j)), v = l0 <c, hm> + n0^2 r^(2 NG) with
 * c = y (1/t, t, t^2, t^3, t^5, t^6, t^7, 0), ad_k = lambda^(k div dp) base^(k mod dp) for k < D,
 * pub_k = [k < D] (t^2 ad_k q^-(k+1) + t (e - x delta q^-(k+1))) + [k < base] t^3 x q^-(k+1) / (e + k) and
 * g_off = 2 t^3 (sum_{k<D} q^(k+1) + e sum_{k<D} ad_k - x delta sum_{k<D} ad_k q^-(k+1)) — the ONE multi-scalar multiplication of
 * verify_given_commitment_multiplicands.  G1 points are affine Montgomery words (zero words: the identity), taken as members of the subgroup; scalars are
 * canonical words (any 256-bit value, reduced), or ark-ff Montgomery words when `montgomery` is set (`random` too).
 *
 * dgpu_bpp_range_proofs_verify_each_g1 writes per proof
 *   status[i] = 0   verified
 *   status[i] = 1   the equation failed: the reference's only verdict, WeightedNormLinearArgumentVerificationFailed
 *   status[i] = 2   one of t, r, e + k (k < base) is zero modulo r: the reference unwrap()s an inverse there; no honest transcript produces it
 *
 * dgpu_bpp_range_proofs_verify_batch_g1 gives one verdict under rho = random (non-zero modulo r, else DGPU_E_BADARG): proof i is weighed by rho^i, and *ok = 1
 * iff no proof has status 2 and the weighted sum of the n equations is the identity.  The sum is a polynomial of degree n - 1 in rho whose coefficients are
 * the proofs' sums: an invalid batch passes with probability at most (n - 1) / r over a uniform rho.  rho = 1 is the plain sum of the equations: proofs whose
 * errors cancel (a point moved by +E in one proof and -E in another) pass it; it is accepted for tests, not for use.  An empty batch verifies.
 *
 * n = 0 returns DGPU_OK without looking at anything else (the batch: *ok = 1 when ok is not NULL).  Then a NULL pointer, base outside {2, 4, 8, 16}, num_bits
 * that is no power of two in [bb, 64], m that is no power of two in [1, 8], an NG that is no power of two (base 8 with num_bits >= 32: the reference cannot
 * build such a proof) and n >= 2^31 are DGPU_E_BADARG before the device is looked at; then DGPU_E_NODEVICE; then a handle that is no plain G1 bases handle of
 * 9 + NG points is DGPU_E_BADARG (a handle exists only where a device does, so this check cannot come first).  Never DGPU_E_TOO_SMALL.  Thread-safe; one slot
 * per call.  Chunks: the each call takes min(the many-row kernels' rows for 9 + NG terms, 4096)
 * proofs, the batch call the largest count with rows (m + 4 + 2 K) <= 2^16, at least one; dgpu_set_many_chunk_rows of the development surface cuts both
 * further.  Stage timers bpp.consts, bpp.shared, bpp.stage, bpp.verdict (each), bpp.columns (the batch) beside msm.*. */
int32_t dgpu_bpp_range_proofs_verify_each_g1(uint64_t setup, uint32_t base, uint32_t num_bits, uint32_t m, const uint64_t *values /* n*m*12: V */,
                                             const uint64_t *round_points /* n*4*12: D, M, R, S */, const uint64_t *wnla_points /* n*2K*12: X_0.., R_0.. */,
                                             const uint64_t *l_n /* n*2*4 */, const uint64_t *challenges /* n*(7+K)*4: e, x, y, r, lambda, delta, t, gamma_0.. */,
                                             size_t n, int32_t montgomery, uint8_t *status /* n */);
int32_t dgpu_bpp_range_proofs_verify_batch_g1(uint64_t setup, uint32_t base, uint32_t num_bits, uint32_t m, const uint64_t *values /* n*m*12: V */,
                                              const uint64_t *round_points /* n*4*12: D, M, R, S */, const uint64_t *wnla_points /* n*2K*12: X_0.., R_0.. */,
                                              const uint64_t *l_n /* n*2*4 */, const uint64_t *challenges /* n*(7+K)*4: e, x, y, r, lambda, delta, t, gamma_0.. */,
                                              size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
