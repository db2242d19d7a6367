// crypto_amd/csrc/setup_kernels.hip.h — the scalar half of LegoGroth16 key generation on gfx950 (dock_setup.hip drives them).
//
// Device side of LibsnarkReduction::instance_map_with_evaluation (/root/reference/legogroth16/src/r1cs_to_qap.rs:105-147) and of the key scalars
// of generate_parameters_and_extra_info_with_qap (legogroth16/src/generator.rs:296-326, r1cs_to_qap.rs:212-223):
//   u_i = Z(t) w^i / (D (t - w^i))        k_lagrange: one Fermat inversion per lane, Montgomery's trick over the lane's strided share
//   a_j = u_{m+j} (j < num_inputs) + sum over A's entries (i, j, v) of u_i v,  b, c likewise over B, C
//        the matrices are row-sorted (CSR); the column sums need them by column: a counting sort of the nnz by column (k_col_count and
//        k_col_scatter with wave-aggregated atomics, a three-pass scan; the scatter forms the product u_i v), then a segmented sum balanced by nnz (k_fold, repeated on its
//        own partials): a column of 2^20 entries (C of the `nconstraints` circuit: every row names variable 0) costs no more than 2^20
//        entries spread over many columns.
//   mix_j = beta a_j + alpha b_j + c_j;  gamma_abc_j = mix_j / gamma (j < n),  l_j = mix_j / delta (j >= n)   k_key_scalars
// Layout as in ntt_kernels.hip.h: limb-major SoA (word l of element i at buf[l * stride + i]); scalars handed on are canonical 8 x u32 words.
#pragma once
#include <hip/hip_runtime.h>
#include "fr29.hip.h"

namespace setupk {
using namespace fr29;

__device__ __forceinline__ void ld(Fr &r, const uint32_t *__restrict__ buf, size_t stride, size_t i) {
#pragma unroll
    for (int l = 0; l < NL; l++) r.l[l] = buf[(size_t)l * stride + i];
}
__device__ __forceinline__ void st(uint32_t *__restrict__ buf, size_t stride, size_t i, const Fr &a) {
#pragma unroll
    for (int l = 0; l < NL; l++) buf[(size_t)l * stride + i] = a.l[l];
}
__device__ __forceinline__ void ld_const(Fr &r, const uint32_t *__restrict__ words) {
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = words[k];
    fr_from_words(r, w, false);
}

// lane g of G owns the elements i = g + k G (k < K, i < D): consecutive lanes touch consecutive elements.  pw: w^i (SoA, stride D);
// consts: t, Z(t) / D (canonical words).  out (SoA, stride D) holds the prefix products, then u_i.
__global__ void __launch_bounds__(256) k_lagrange(const uint32_t *__restrict__ pw, const uint32_t *__restrict__ consts, size_t D, size_t G, uint32_t *__restrict__ out) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const size_t n = (D - g + G - 1) / G;
    Fr t; ld_const(t, consts);
    auto x = [&](size_t k, Fr &v) { Fr w; ld(w, pw, D, g + k * G); fr_sub(v, t, w); fr_norm(v, v); };    // t - w^i: < 514 r, limbs < 2^29 + 8
    auto lo = [&](size_t k, Fr &v) { ld(v, out, D, g + k * G); };
    auto so = [&](size_t k, const Fr &v) { st(out, D, g + k * G, v); };
    fr_batch_inv(n, x, lo, so);
    Fr ztd; ld_const(ztd, consts + 8);
    for (size_t k = 0; k < n; k++) {
        const size_t i = g + k * G;
        Fr v, w; ld(v, out, D, i); ld(w, pw, D, i);
        fr_mul(v, v, w); fr_mul(v, v, ztd);
        st(out, D, i, v);
    }
}
// a_j = u_{m + j} for j < num_inputs, every other entry of a, b, c zero (the sums are added onto these)
__global__ void __launch_bounds__(256) k_im_init(const uint32_t *__restrict__ u, size_t D, size_t m, size_t num_inputs, size_t nv, uint32_t *__restrict__ a, uint32_t *__restrict__ b, uint32_t *__restrict__ c) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nv) return;
    Fr z, v; fr_zero(z); v = z;
    if (j < num_inputs) ld(v, u, D, m + j);
    st(a, nv, j, v); st(b, nv, j, z); st(c, nv, j, z);
}
// ---- counting sort of a CSR matrix's entries by column ----
// old = ctr[key]++ for every lane with `valid`, with the lanes of a wave that share a key served by ONE atomic: a column that holds a large share
// of the entries (C of the `nconstraints` circuit names variable 0 in every row) would otherwise send one same-address atomic per entry to one L2
// channel.  Up to WAGG_ROUNDS rounds each take the lowest pending lane's key and every pending lane that holds it; the lanes still pending after
// that (keys that occur in few lanes) issue their atomics together.  Every lane of the wave must call it (ballots).
constexpr int WAGG_ROUNDS = 4;
__device__ __forceinline__ uint32_t wave_atomic_inc(uint32_t *__restrict__ ctr, uint32_t key, bool valid) {
    const int lane = __lane_id();
    unsigned long long pending = __ballot(valid);
    uint32_t pos = 0;
    for (int round = 0; round < WAGG_ROUNDS && pending; round++) {
        const int leader = __ffsll(pending) - 1;
        const uint32_t lk = __shfl(key, leader);
        const unsigned long long grp = __ballot(valid && key == lk) & pending;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&ctr[lk], (uint32_t)__popcll(grp));
        base = __shfl(base, leader);
        if ((grp >> lane) & 1) pos = base + (uint32_t)__popcll(grp & ((1ull << lane) - 1));
        pending &= ~grp;
    }
    if ((pending >> lane) & 1) pos = atomicAdd(&ctr[key], 1u);
    return pos;
}
__global__ void __launch_bounds__(256) k_col_count(const uint32_t *__restrict__ cols, size_t nnz, uint32_t *__restrict__ cnt) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = k < nnz;
    (void)wave_atomic_inc(cnt, valid ? cols[k] : 0u, valid);
}
// exclusive prefix sum of n counters in place, in three passes: k_scan_tiles (each block sums a tile of SCAN_TILE consecutive counters),
// k_scan_excl over the tile sums (one block), k_scan_apply (each block scans its tile in LDS, starting from its tile's offset)
constexpr int SCAN_B = 256, SCAN_ITEMS = 8, SCAN_TILE = SCAN_B * SCAN_ITEMS;
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *part) {      // SCAN_B threads; returns the exclusive prefix of v
    const int t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (int off = 1; off < SCAN_B; off <<= 1) {
        const uint32_t w = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += w;
        __syncthreads();
    }
    const uint32_t r = part[t] - v;
    __syncthreads();
    return r;
}
__global__ void __launch_bounds__(SCAN_B) k_scan_tiles(const uint32_t *__restrict__ x, size_t n, uint32_t *__restrict__ tile_sum) {
    __shared__ uint32_t part[SCAN_B];
    const size_t lo = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    uint32_t s = 0;
    for (int q = 0; q < SCAN_ITEMS; q++) if (lo + q < n) s += x[lo + q];
    const uint32_t pre = block_excl_scan(s, part);
    if (threadIdx.x == SCAN_B - 1) tile_sum[blockIdx.x] = pre + s;
}
__global__ void __launch_bounds__(SCAN_B) k_scan_apply(uint32_t *__restrict__ x, size_t n, const uint32_t *__restrict__ tile_off) {
    __shared__ uint32_t part[SCAN_B];
    const size_t lo = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS], s = 0;
    for (int q = 0; q < SCAN_ITEMS; q++) { v[q] = lo + q < n ? x[lo + q] : 0u; s += v[q]; }
    uint32_t run = tile_off[blockIdx.x] + block_excl_scan(s, part);
    for (int q = 0; q < SCAN_ITEMS; q++) if (lo + q < n) { x[lo + q] = run; run += v[q]; }
}
// in place: x -> exclusive prefix sum of x over n entries, one block of SCAN_T threads (each scans a contiguous slice, the slice totals are scanned
// in LDS): the middle pass of the scan above, over one word per tile
constexpr int SCAN_T = 1024;
__global__ void __launch_bounds__(SCAN_T) k_scan_excl(uint32_t *__restrict__ x, size_t n) {
    __shared__ uint32_t part[SCAN_T];
    const int t = threadIdx.x;
    const size_t per = (n + SCAN_T - 1) / SCAN_T, lo = min(n, t * per), hi = min(n, lo + per);
    uint32_t s = 0;
    for (size_t i = lo; i < hi; i++) s += x[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < SCAN_T; off <<= 1) {                  // Hillis-Steele over the slice totals
        const uint32_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (size_t i = lo; i < hi; i++) { const uint32_t v = x[i]; x[i] = run; run += v; }
}
// entry k of row i (found by bisection of rowptr: rows of any length cost the same) goes to slot cursor[col]++ of its column, as the key col and
// the value u_i * coeff.  The order inside a column depends on the atomics; the sums do not.
__global__ void __launch_bounds__(256) k_col_scatter(const uint64_t *__restrict__ rowptr, size_t rows, const uint32_t *__restrict__ cols, const uint32_t *__restrict__ vals, size_t vstride, size_t nnz,
                                                     const uint32_t *__restrict__ u, size_t D, uint32_t *__restrict__ cursor, uint32_t *__restrict__ keys, uint32_t *__restrict__ out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = k < nnz;
    const uint32_t col = valid ? cols[k] : 0u;
    const uint32_t pos = wave_atomic_inc(cursor, col, valid);       // (every lane takes part in the ballots)
    if (!valid) return;
    size_t lo = 0, hi = rows;                   // the row i with rowptr[i] <= k < rowptr[i + 1]
    while (hi - lo > 1) { const size_t mid = (lo + hi) >> 1; if (rowptr[mid] <= k) lo = mid; else hi = mid; }
    Fr c, ui, v; ld(c, vals, vstride, k); ld(ui, u, D, lo);
    fr_mul(v, ui, c);
    keys[pos] = col;
    st(out, nnz, pos, v);
}
// one segmented-sum pass over n key-sorted entries in chunks of ch (<= 2^10): runs complete inside a chunk are added onto out[key] (every key
// is completed exactly once over all passes), the first and last runs of each chunk go to the 2 x nchunks partials (fr_fold_chunk)
__global__ void __launch_bounds__(256) k_fold(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, size_t n, size_t ch, int final_pass,
                                              uint32_t *__restrict__ out, size_t nv, uint32_t *__restrict__ pkeys, uint32_t *__restrict__ pvals) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nch = (n + ch - 1) / ch;
    if (c >= nch) return;
    const size_t lo = c * ch, hi = min(n, lo + ch), pn = 2 * nch;
    auto val = [&](size_t k, Fr &v) { ld(v, vals, n, k); };
    auto done = [&](uint32_t key, const Fr &s) { Fr o; ld(o, out, nv, key); fr_add(o, o, s); fr_norm(o, o); st(out, nv, key, o); };
    auto part = [&](int which, uint32_t key, const Fr &s) { pkeys[2 * c + which] = key; st(pvals, pn, 2 * c + which, s); };
    fr_fold_chunk(keys, lo, hi, final_pass != 0, val, done, part);
}
// SoA internal -> 8 x u32 words (mont: x 2^256 mod r, ark-ff's Fr limbs; else canonical)
__global__ void __launch_bounds__(256) k_soa_to_words(const uint32_t *__restrict__ src, size_t n, int mont, uint32_t *__restrict__ words) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr x; ld(x, src, n, i);
    uint32_t w[8]; fr_to_words(w, x, mont != 0);
    uint4 *q = reinterpret_cast<uint4 *>(words + i * 8);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]); q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// the scalars of the queries that depend on a, b, c (canonical words, what k_fb_mul takes): a, b as they are, gamma_abc = mix[..n] / gamma,
// l = mix[n..] / delta.  consts: alpha, beta, 1/gamma, 1/delta (canonical words)
__global__ void __launch_bounds__(256) k_key_scalars(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, const uint32_t *__restrict__ c, size_t nv, size_t n_abc,
                                                     const uint32_t *__restrict__ consts, uint32_t *__restrict__ a_w, uint32_t *__restrict__ b_w, uint32_t *__restrict__ abc_w, uint32_t *__restrict__ l_w) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nv) return;
    Fr al, be, k, x, y, z, m, t;
    ld_const(al, consts); ld_const(be, consts + 8); ld_const(k, consts + (j < n_abc ? 16 : 24));
    ld(x, a, nv, j); ld(y, b, nv, j); ld(z, c, nv, j);             // (values < 4 r, limbs <= 2^29 + 7)
    fr_mul(m, x, be); fr_mul(t, y, al); fr_add(m, m, t); fr_add(m, m, z); fr_norm(m, m);
    fr_mul(m, m, k);
    uint32_t w[8];
    fr_to_words(w, x, false);
#pragma unroll
    for (int q = 0; q < 8; q++) a_w[j * 8 + q] = w[q];
    fr_to_words(w, y, false);
#pragma unroll
    for (int q = 0; q < 8; q++) b_w[j * 8 + q] = w[q];
    fr_to_words(w, m, false);
    uint32_t *dst = j < n_abc ? abc_w + j * 8 : l_w + (j - n_abc) * 8;
#pragma unroll
    for (int q = 0; q < 8; q++) dst[q] = w[q];
}

}  // namespace setupk
