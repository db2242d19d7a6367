// crypto_amd/csrc/saver_kernels.hip.h — what SAVER (verifiable encryption, the reference's saver crate) needs beyond the kernels the library has
// (dock_saver.hip drives it):
//   the table    T_j[m] = e(g_j, V_2_j)^m, m = 1 .. E = 2^b - 1, for the K chunk columns j, resident in the ABI form k_final_exp writes (144 u32 per
//                element, entry m at word ((j E + m - 1) 144).  It grows by doubling: round t writes T_j[2^t + k] = T_j[2^t] T_j[k], k = 1 .. 2^t (the last
//                round cut at E), one product per six-lane group (gt_mul, gt_kernels.hip.h), every column in one launch            k_gt_table_extend
//                A GT element has ONE canonical form, so these words are the words of the reference's `cur += g_i_v_i` chain (keygen.rs:211-234).
//   the lookup   the chunk m with T_j[m] = p for a pairing value p (encryption.rs:677-696), exactly: p = one gives 0; else the 64-bit fingerprint of p
//                (its first two ABI words under the key's mask) is binary-searched in the column's sorted index, the run of equal fingerprints is
//                scanned and a candidate counts only if all 144 words agree.  compare-at-index mode: entry m is given, no search   k_gt_dlog_lookup
//   the verdict  the K miss bytes of a ciphertext folded into its status; a missed row's chunks are zeroed                          k_saver_row_verdict
// The lookup and the verdict are ONE host + device function each: tests/native/saver_dev_host_shim.cpp drives the same text over synthetic tables,
// and runs the table's group body under the FP29_CHECK bound tracker.  gt_mul takes class N operands below 16 p and leaves one below 2 p; both
// operands here come out of fp_from_abi (canonical, below p), and gt_put_abi's fp_to_abi reduces to the canonical residue.
#pragma once
#include "gt_kernels.hip.h"

namespace saverk {
using namespace bls29;

constexpr int SAVER_MISS = -1;

// ---- the table: what one group of k_gt_table_extend does -------------------------------------------------------------------------------------------
template <class X> FD void table_extend_group(X &x, const uint32_t *a, const uint32_t *b, uint32_t *dst) {
    const int e = x.lane();
    Fp2 fa, fb, r; gt_get_abi(fa, a, e); gt_get_abi(fb, b, e);
    gt_mul(x, r, fa, fb);
    gt_put_abi(dst, e, r);
}

// ---- the lookup ------------------------------------------------------------------------------------------------------------------------------------
FD bool words_eq(const uint32_t *a, const uint32_t *b) {
    uint32_t d = 0;
    for (int k = 0; k < GT_ABIW; k++) d |= a[k] ^ b[k];
    return d == 0;
}
FD uint64_t fingerprint(const uint32_t *el, uint64_t mask) { return (((uint64_t)el[1] << 32) | el[0]) & mask; }
// the chunk of p in one column, or SAVER_MISS.  tab: the column's E entries; fps / ms: its index, the entries' masked fingerprints in ascending order
// with their m.  at_index: compare with entry m alone (m = 0: with one; m > E: a miss).
FD int dlog_lookup(const uint32_t *p, const uint32_t *one, const uint32_t *tab, const uint64_t *fps, const uint16_t *ms, uint32_t E, uint64_t mask, bool at_index,
                   uint32_t m) {
    if (at_index) {
        if (m > E) return SAVER_MISS;
        if (m == 0) return words_eq(p, one) ? 0 : SAVER_MISS;
        return words_eq(p, tab + (size_t)(m - 1) * GT_ABIW) ? (int)m : SAVER_MISS;
    }
    if (words_eq(p, one)) return 0;
    const uint64_t f = fingerprint(p, mask);
    uint32_t lo = 0, hi = E;                                              // the first k with fps[k] >= f
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (fps[mid] < f) lo = mid + 1; else hi = mid; }
    for (uint32_t k = lo; k < E && fps[k] == f; k++) {
        const uint32_t c = ms[k];
        if (words_eq(p, tab + (size_t)(c - 1) * GT_ABIW)) return (int)c;
    }
    return SAVER_MISS;
}
// status of one ciphertext from its K miss bytes: 0 decrypted, 1 CouldNotFindDiscreteLog (its chunks are zeroed then)
FD uint8_t row_verdict(const uint8_t *miss, size_t K, uint16_t *chunks) {
    uint8_t any = 0;
    for (size_t j = 0; j < K; j++) any |= miss[j];
    if (any) for (size_t j = 0; j < K; j++) chunks[j] = 0;
    return any ? 1 : 0;
}

#ifdef __HIPCC__
// everything the lookup reads of a key
struct DkIndex { const uint32_t *tab; const uint64_t *fps; const uint16_t *ms; const uint32_t *one; uint32_t E; uint64_t mask; };

// pairing value (i, j) of `rows` ciphertexts and K columns sits at p + (j rows + i) 144 (column-major, as the line buffer).  at_index: chunks holds the
// claimed m, else it receives the found one (row-major, i K + j).  miss[i K + j] = 1 where nothing matched.  One lane per value: the search is a
// dozen dependent 8-byte loads, the confirmation 576 bytes of each side.
__global__ void __launch_bounds__(64) k_gt_dlog_lookup(const uint32_t *__restrict__ p, size_t rows, size_t K, DkIndex dk, int at_index, uint16_t *__restrict__ chunks,
                                                       uint8_t *__restrict__ miss) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * K) return;
    const size_t j = t / rows, i = t % rows;
    const size_t off = j * dk.E;
    const int c = dlog_lookup(p + t * GT_ABIW, dk.one, dk.tab + off * GT_ABIW, dk.fps + off, dk.ms + off, dk.E, dk.mask, at_index != 0, at_index ? chunks[i * K + j] : 0u);
    if (!at_index) chunks[i * K + j] = c < 0 ? 0 : (uint16_t)c;
    miss[i * K + j] = c < 0 ? 1 : 0;
}
// status[i] = row_verdict; extra: one more byte per row that must be 1 for the row to hold (the V_0 check of verify_decryption), or nullptr.
// invert: write ok bytes (1 = holds) instead of status bytes
__global__ void __launch_bounds__(64) k_saver_row_verdict(const uint8_t *__restrict__ miss, size_t rows, size_t K, uint16_t *__restrict__ chunks, const uint8_t *__restrict__ extra,
                                                          int invert, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    uint8_t st = row_verdict(miss + i * K, K, chunks + i * K);
    if (extra && !extra[i]) st = 1;
    status[i] = invert ? (st ? 0 : 1) : st;
}
#endif

}  // namespace saverk
