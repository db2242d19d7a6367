// crypto_amd/csrc/saver_launch.hip.h — host-callable launchers of the SAVER kernels (k_saver.hip, saver_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace saverk {
// How a call is cut.  SAVER_PAIR_ROWS: two-pair pairing rows per chunk of the decryption calls — the one size at which §13-§15 measured
// k_miller_tail and k_final_exp; SAVER_COMMIT_PAIRS: pairs per chunk of dgpu_saver_verify_commitment_each; SAVER_BATCH_CHUNK: rows per MSM of the batch
constexpr size_t SAVER_PAIR_ROWS = 4096, SAVER_COMMIT_PAIRS = 8192, SAVER_BATCH_CHUNK = 65536;
// one doubling round of the table of K columns of E entries (144 u32 each, entry m at (j E + m - 1) 144): T_j[half + k] = T_j[half] T_j[k] for
// k = 1 .. cnt, cnt <= half and half + cnt <= E
void launch_gt_table_extend(hipStream_t s, uint32_t *tab, size_t K, uint32_t E, uint32_t half, uint32_t cnt);
// the index of a key on the device: the table, per column the sorted masked fingerprints with their m, the element one
struct DkDev { const uint32_t *tab; const uint64_t *fps; const uint16_t *ms; const uint32_t *one; uint32_t E; uint64_t mask; };
// p: rows x K pairing values, column-major (value (i, j) at (j rows + i) 144).  at_index: chunks (rows x K, row-major) holds the claimed m, else it
// receives the found one; miss: rows x K bytes
void launch_gt_dlog_lookup(hipStream_t s, const uint32_t *p, size_t rows, size_t K, const DkDev &dk, bool at_index, uint16_t *chunks, uint8_t *miss);
// status[i] = 1 iff a chunk of row i missed (its chunks are zeroed then) or extra[i] == 0 (extra may be nullptr); invert: 1 iff none did
void launch_saver_row_verdict(hipStream_t s, const uint8_t *miss, size_t rows, size_t K, uint16_t *chunks, const uint8_t *extra, bool invert, uint8_t *status);
}  // namespace saverk
