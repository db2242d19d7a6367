/* include/dock_gpu_saver.h — SAVER (verifiable encryption) in bulk: the C ABI of crypto_amd/libdock_gpu_saver.so beyond include/dock_gpu.h.
 * Conventions, error codes and DGPU_G2_PREPARED_WORDS: include/dock_gpu.h. */
#ifndef DOCK_GPU_SAVER_H
#define DOCK_GPU_SAVER_H
#include "dock_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- SAVER (verifiable encryption over LegoGroth16) in bulk: decrypt, verify decryptions and commitments (crypto_amd/csrc/dock_saver.hip) ----
 * These seven calls are NOT part of libdock_gpu.so: they are served by libdock_gpu_saver.so, the product's objects plus dock_saver.o and k_saver.o — a library of
 * its own beside the product, as the development twin is, with its own contexts and handle table: bring it up with its own dgpu_init, and use every handle
 * under the library that made it.  It exports everything include/dock_gpu.h declares as well, so a host that needs SAVER links this one INSTEAD of the product.
 * The reference's saver crate for many ciphertexts under one key.  A ciphertext row is [c_0, c_1 .. c_K, psi], (K + 2) * 12 words, in every call (the decryption
 * calls ignore psi); K is the number of chunks of chunk_bit_size = b bits (1 <= K <= 255, 1 <= b <= 16).  Points are affine ABI words, zero words are the
 * identity, and a pair with an identity member contributes one, as everywhere in the library and in arkworks: the verdicts are the reference's.  Points are taken
 * as validated members of the subgroups.
 *
 * dgpu_saver_dk_create makes a decryption key resident: g_i (K G1 points, the generators of the chunks), the G2 points H (EncryptionGens), V_0, V_1[K], V_2[K]
 * (DecryptionKey, keygen.rs:256-299).  The handle keeps on the device the prepared coefficients of the 2 K + 2 G2 points, the table
 * T_j[m] = e(g_j, V_2_j)^m for m = 1 .. 2^b - 1 and j < K in the canonical form (72 words per element: 576 B * K * (2^b - 1), 604 MB at b = 16, K = 16) — the
 * reference's pairing_powers (keygen.rs:211-234), built by doubling rounds of parallel products — and per column a search index of the entries' 64-bit
 * fingerprints sorted with m.  Out of memory is DGPU_E_OOM and leaves nothing behind.  dgpu_saver_dk_free releases it (it waits for calls in flight).
 * dgpu_saver_dk_powers reads entries back: out[k] = T_j[first + k], k < count, i.e. pairing_powers[j][first - 1 + k]; 1 <= first, first + count - 1 <= 2^b - 1.
 *
 * dgpu_saver_decrypt_many is Ciphertext::decrypt_to_chunks_given_pairing_powers (encryption.rs:569-624) for n ciphertexts with the secret key sk = rho:
 * p_ij = e(c_ij, V_2_j) e(-rho c_0_i, V_1_j), chunks[i K + j] = the m with T_j[m] = p_ij (0 when p_ij is one), found by an exact lookup on the device
 * (the fingerprint finds candidates, all 72 words decide); nu_xy[i] = rho c_0_i.  status[i] = 0: decrypted; 1: some chunk has no discrete log in the table
 * (the reference's CouldNotFindDiscreteLog) — that row's chunks are zeros.  -rho c_0_i is the GLV scaling [s] P of dgpu_g1_scale_batch: for points of G1 ONLY.
 * The device copy of rho is zeroed on every return path.
 *
 * dgpu_saver_verify_decryption_each is verify_decryption (encryption.rs:425-469) per row: ok[i] = 1 iff e(-nu_i, H) e(c_0_i, V_0) = 1 and for every j
 * e(c_ij, V_2_j) e(-nu_i, V_1_j) = T_j[m_ij] (one for m_ij = 0) — by bilinearity the reference's e(m_ij g_j - c_ij, V_2_j) e(nu_i, V_1_j) = 1; a chunk of
 * 2^b or more fails the row.  Else the reference returns InvalidDecryption.
 *
 * dgpu_saver_verify_commitment_each is verify_ciphertext_commitment (encryption.rs:367-393) per row against all_pc, the prepared coefficients of
 * [Z_0 .. Z_K, H] in that order ((K + 2) * DGPU_G2_PREPARED_WORDS words; the verifier holds no decryption key): ok[i] = 1 iff
 * e(c_0_i, Z_0) prod_j e(c_ij, Z_j) e(-psi_i, H) = 1.  dgpu_saver_verify_commitments_batch is verify_commitments_in_batch (:395-422, :710-740): K + 2 MSMs over the
 * columns with the caller's r_powers (n scalars) and ONE multi-pairing of K + 2 pairs; *ok = 1 iff it is one (an empty batch verifies).
 *
 * n = 0 returns DGPU_OK without looking at anything else.  Then a NULL argument, b outside 1 .. 16, K outside 1 .. 255, n >= 2^31, and a handle that is not a live
 * SAVER key are DGPU_E_BADARG before the device is looked at; then DGPU_E_NODEVICE.  Chunks: the decryption calls take the largest count of ciphertexts with
 * rows * K <= 4096 two-pair pairing rows, at least one (the V_0 column of the verifier runs over up to 4096 ciphertexts a pass); commitment_each at most 8192 pairs; the batch 65536 rows per MSM;
 * dgpu_set_many_chunk_rows of the development surface cuts all of them.  Stage timers saver.prepare, saver.base_lines, saver.table, saver.index_readback, saver.index_sort,
 * saver.scale, saver.lines (the per-column line launches), saver.lookup, saver.verdict beside bbs.products, bbs.tail, bbs.final_exp. */
int32_t dgpu_saver_dk_create(const uint64_t *g_i /* K*12 */, const uint64_t H[24], const uint64_t V_0[24], const uint64_t *V_1 /* K*24 */, const uint64_t *V_2 /* K*24 */,
                             int32_t chunk_bit_size, size_t K, uint64_t *handle);
int32_t dgpu_saver_dk_free(uint64_t dk);
int32_t dgpu_saver_dk_powers(uint64_t dk, size_t j, size_t first, size_t count, uint64_t *out /* count*72 */);
int32_t dgpu_saver_decrypt_many(uint64_t dk, const uint64_t *ct /* n*(K+2)*12 */, size_t n, const uint64_t sk[4], int32_t montgomery, uint16_t *chunks /* n*K */,
                                uint64_t *nu_xy /* n*12 */, uint8_t *status /* n */);
int32_t dgpu_saver_verify_decryption_each(uint64_t dk, const uint64_t *ct /* n*(K+2)*12 */, size_t n, const uint16_t *chunks /* n*K */, const uint64_t *nu_xy /* n*12 */,
                                          uint8_t *ok /* n */);
int32_t dgpu_saver_verify_commitment_each(const uint64_t *all_pc /* (K+2) * DGPU_G2_PREPARED_WORDS */, size_t K, const uint64_t *ct /* n*(K+2)*12 */, size_t n,
                                          uint8_t *ok /* n */);
int32_t dgpu_saver_verify_commitments_batch(const uint64_t *all_pc /* (K+2) * DGPU_G2_PREPARED_WORDS */, size_t K, const uint64_t *ct /* n*(K+2)*12 */, size_t n,
                                            const uint64_t *r_powers /* n*4 */, int32_t montgomery, int32_t *ok);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
