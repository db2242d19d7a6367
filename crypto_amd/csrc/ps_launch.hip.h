// crypto_amd/csrc/ps_launch.hip.h — host-callable launchers of the PS (Coconut) scalar kernels (k_ps.hip, ps_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "bbs_launch.hip.h"
namespace psk {
// How a call is cut.  All of these are UNMEASURED (tests/perf/ps_timing.py reports what they would be tuned from); they are §13's rules:
//   PS_EACH_CHUNK    rows per chunk of dgpu_ps_sign_many_g1 and dgpu_ps_verify_each, at most (and 2^17 / (L + 1), the many-row kernels' rule); MSM rows per chunk
//                    of dgpu_ps_pok_verify_each, which runs two per proof: half as many proofs
//   PS_BATCH_TERMS   scalars of messages per chunk of dgpu_ps_verify_batch (32 MB), PS_BATCH_CHUNK its rows at most
//   PS_COL_RUN       rows per lane of k_ps_col_scalars: the start power costs at most 2 log2(n) products, then one or two per row
constexpr size_t PS_EACH_CHUNK = 4096, PS_BATCH_TERMS = (size_t)1 << 20, PS_BATCH_CHUNK = 65536, PS_COL_RUN = 16;
// out[16 i ..] = r_i, out[16 i + 8 ..] = u_i = r_i (x + sum_j y_j m_ij), canonical words.  sk: (1 + L) x 8 words (x, y_1 .. y_L); r: rows x 8; msgs: rows x L x 8
// packed (mont: ark-ff Montgomery form, else any 256-bit value)
void launch_ps_sign_rows(hipStream_t s, const uint32_t *sk, const uint32_t *r, const uint32_t *msgs, int mont, size_t rows, size_t L, uint32_t *out);
// out_rows: rows x n canonical words-of-8, n = L + 1: row i = (1, m_i1 .. m_iL) — the 2023 BBS row without a multiplier, so k_bbs_rows writes it: ONE fixed
// column, no s, no t (bbs_launch.hip.h)
inline void launch_ps_rows(hipStream_t s, const uint32_t *msgs, int mont, size_t rows, size_t n, uint32_t *out_rows) {
    bbsk::launch_bbs_rows(s, nullptr, msgs, nullptr, mont, rows, n, 1, out_rows);
}
// a chunk's proofs on the device: resp: rows x 8 words (the response over g_tilde), vals: rows x L x 8 words packed, rev: rows x L bytes
struct PokDev { const uint32_t *resp, *vals; const uint8_t *rev; size_t L; int mont; };
// out_rows: 2 rows x (L + 2) canonical words-of-8: the S rows (0, hidden ? z : 0 .., z_r), then the R rows (1, revealed ? m : 0 .., 0)
void launch_ps_pok_rows(hipStream_t s, const PokDev &in, size_t rows, uint32_t *out_rows);
// the chunk [i0, i0 + rows) of a batch: cols[(k * cstride + i) * 8 ..] for k < L + 2 — rho^(i0 + i); rho^(i0 + i) m_i(k-1); -rho^(i0 + i) — canonical words
void launch_ps_col_scalars(hipStream_t s, const uint32_t *msgs, const uint32_t rho_words[8], int mont, size_t rows, size_t L, size_t i0, size_t cstride, uint32_t *cols);
// status[i] of SignaturePoK::verify: got / got_inf: S_i - c_i k_i (rows x 48 words, flags), t: the commitments (rows x 48), sig: [sigma_1' | -sigma_2'] (rows x 24
// words each), pairing: the pairing's verdict bytes
void launch_ps_verdict(hipStream_t s, const uint32_t *got, const uint8_t *got_inf, const uint32_t *t, const uint32_t *sig, const uint8_t *pairing, size_t rows, uint8_t *status);
}  // namespace psk
