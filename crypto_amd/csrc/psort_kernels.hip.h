// crypto_amd/csrc/psort_kernels.hip.h — two-level partition sort of the (bucket key, term) pairs of an MSM, for wide windows
// (keys of up to 22 bits), where the per-window LDS sweep of sort_kernels.hip.h would re-read every digit column once per bucket range.
//
//   P1 k_ps_count1    tile t of 512 scalars: signed digits -> keys; LDS histogram over the partitions p = key >> 11   -> cnt1[p][t]
//   P2 (scan)         exclusive scan of cnt1 (partition-major, so partition p's pairs end up contiguous)
//   P3 k_ps_scatter1  same digits again; the tile's pairs are staged in LDS grouped by partition and leave as contiguous runs
//   P4 k_ps_bucket    block p owns partition p (2048 buckets): LDS histogram of the low 11 key bits, block scan -> off[] of its buckets
//                     (what k_accumulate needs), then LDS cursors place every term at its bucket's slot -> entries[]
// No global atomics (the order inside a bucket is the arrival order of LDS atomics: any order gives the same group element), each pair is
// written once (8 B) and read twice, the scalars are read twice: ~0.35 GB of traffic at n = 2^20 against 3.3 GB of sweeps at c = 20.
//
// Key / value spelling (so that one set of kernels serves both table layouts):
//   key = w * key_wstride + (|digit| - 1)            key_wstride = 0: all windows share one bucket set (precomputed 2^(c w) P tables)
//   val = (val_base + w * val_wstride + i) | sign << 31     index of the base record the term adds
#pragma once
#include "dyn_chunk.hip.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sort_launch.hip.h"
#include "ps_digits.hip.h"

namespace msm {


// LDS counter increment that survives hot keys (all scalars equal, a witness that is mostly 0 / 1, the few values of the short top window):
// the lanes of a wave that target the SAME counter as its first active lane are served by ONE atomic (that lane adds their population count
// and they take consecutive slots); only the others issue an atomic of their own.  A key that dominates a partition thus costs one LDS
// atomic per wave instead of up to 64 serialised ones on one address.  Must be called by all lanes of the wave (`active` masks the idle
// ones).  Returns the slot.
__device__ __forceinline__ uint32_t lds_inc_agg(uint32_t *cnt, uint32_t bin, bool active) {
    const uint64_t mask = __ballot(active);
    if (mask == 0) return 0;
    const int lane = threadIdx.x & 63, first = __ffsll((long long)mask) - 1;
    const uint32_t fb = (uint32_t)__shfl((int)bin, first, 64);
    const bool same = active && bin == fb;
    const uint64_t smask = __ballot(same);
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(&cnt[fb], (uint32_t)__popcll(smask));
    base = (uint32_t)__shfl((int)base, first, 64);
    if (same) return base + (uint32_t)__popcll(smask & ((1ull << lane) - 1ull));
    return active ? atomicAdd(&cnt[bin], 1u) : 0u;
}

__device__ __forceinline__ bool ps_live(const PsParams &q, size_t i) {
    // q.idflag == nullptr: a sort shared by several tables (dgpu_scalars_sort): identity rows are skipped by the accumulation instead
    return i < q.n && (!q.idflag || q.idflag[(size_t)q.flag_base + i] == 0);
}

__global__ void __launch_bounds__(256) k_id_flags(const uint32_t *__restrict__ bases, int aff_stride, int flag_word, size_t n, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = bases[i * (size_t)aff_stride + flag_word] != 0 ? 1 : 0;
}

// out[i] = 64-bit fingerprint of raw point i as the caller holds it (x at x_off, y at y_off: `words` 64-bit words each; the identity byte inside the
// point and / or in a separate array): what the resident-bases cache (bases_cache.hpp) keeps per record to notice a key whose host memory changed.
// The host computes the same function for the records it samples (rec_fingerprint) — keep the two in step.
__global__ void __launch_bounds__(256) k_raw_record_hash(const uint8_t *__restrict__ raw, size_t stride, size_t x_off, size_t y_off, size_t inf_off, const uint8_t *__restrict__ is_inf,
                                                         int words, size_t n, uint64_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *pt = raw + i * stride;
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int part = 0; part < 2; part++) {
        const uint8_t *src = pt + (part ? y_off : x_off);
        for (int k = 0; k < words; k++) {
            const uint2 v = *reinterpret_cast<const uint2 *>(src + 8 * k);
            h = (h ^ ((uint64_t)v.x | ((uint64_t)v.y << 32))) * 0xff51afd7ed558ccdull;
            h ^= h >> 32;
        }
    }
    uint64_t flag = 0;
    if (is_inf && is_inf[i]) flag = 1;
    if (inf_off != ~(size_t)0 && pt[inf_off]) flag = 1;
    h = (h ^ flag) * 0xc4ceb9fe1a85ec53ull;
    out[i] = h ^ (h >> 29);
}

// block -> tile: workgroup ids go round the eight XCDs, and the cnt1 / off1 words of tile t sit next to those of tile t + 1 (partition-major layout): the
// blocks of one XCD take CONSECUTIVE tiles, so that the sixteen tiles of a 64-byte line meet in one L2 instead of eight
__device__ __forceinline__ uint32_t ps_tile_of_block(uint32_t b, uint32_t ntiles) {
    const uint32_t per = ntiles >> 3;
    return b < (per << 3) ? (b & 7u) * per + (b >> 3) : b;
}

// P1: cnt1[p * ntiles + tile]
template <int CC, int CW>
__global__ void __launch_bounds__(PS_TILE) k_ps_count1(PsParams q, uint32_t *__restrict__ cnt1) {
    extern __shared__ __align__(16) uint32_t lds[];                   // P counters
    for (uint32_t j = threadIdx.x; j < q.P; j += blockDim.x) lds[j] = 0;
    __syncthreads();
    const uint32_t tile = ps_tile_of_block(blockIdx.x, q.ntiles);
    const size_t i = (size_t)tile * PS_TILE + threadIdx.x;
    if (i < q.n && (q.scalars[i * 8 + 7] >> 31)) atomicOr(q.bad, 1u);
    ps_digits<CC, CW>(q, i, ps_live(q, i), [&](int w, uint32_t m1, uint32_t, bool nz) { (void)lds_inc_agg(lds, nz ? ((uint32_t)w * q.key_wstride + m1) >> q.part_log : 0u, nz); });
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < q.P; j += blockDim.x) cnt1[(size_t)j * q.ntiles + tile] = lds[j];
}

// P3: pairs[off1[p * ntiles + tile] + k] = (key, val) of the k-th pair of tile `tile` that falls in partition p
template <int CC, int CW>
__global__ void __launch_bounds__(PS_TILE) k_ps_scatter1(PsParams q, const uint32_t *__restrict__ cnt1, const uint32_t *__restrict__ off1, uint2 *__restrict__ pairs) {
    extern __shared__ __align__(16) uint32_t lds[];
    uint32_t *cnt = lds, *pre = lds + q.P, *cur = lds + 2 * q.P, *goff = lds + 3 * q.P;      // histogram, exclusive prefix, cursors, the tile's first slot in each partition
    uint2 *stage = reinterpret_cast<uint2 *>(lds + 4 * q.P);          // 8-byte aligned (P is a power of two)
    __shared__ uint32_t wave_tot[PS_TILE / 64 + 1];
    // this tile's histogram is what P1 counted (one digit pass less: the digits are extracted twice per scalar, not three times), read back as the
    // differences of the scanned offsets: off1[idx + 1] - off1[idx] = cnt1[idx], one strided access per partition instead of two
    const uint32_t tile = ps_tile_of_block(blockIdx.x, q.ntiles);
    for (uint32_t j = threadIdx.x; j < q.P; j += blockDim.x) { const size_t idx = (size_t)j * q.ntiles + tile; const uint32_t o0 = off1[idx], o1 = off1[idx + 1]; goff[j] = o0; cnt[j] = o1 - o0; }
    const size_t i = (size_t)tile * PS_TILE + threadIdx.x;
    const bool live = ps_live(q, i);
    __syncthreads();
    // exclusive scan of cnt[0..P): every thread takes P / 512 consecutive bins (P is a power of two >= 1; 512 threads)
    {
        const uint32_t per = (q.P + PS_TILE - 1) / PS_TILE;
        const uint32_t b0 = threadIdx.x * per;
        uint32_t sum = 0;
        for (uint32_t k = 0; k < per; k++) if (b0 + k < q.P) sum += cnt[b0 + k];
        // wave scan + cross-wave totals
        uint32_t incl = sum;
        for (int d = 1; d < 64; d <<= 1) { uint32_t t = __shfl_up(incl, d, 64); if ((int)(threadIdx.x & 63) >= d) incl += t; }
        if ((threadIdx.x & 63) == 63) wave_tot[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t base = 0;
        for (uint32_t wv = 0; wv < (threadIdx.x >> 6); wv++) base += wave_tot[wv];
        uint32_t run = base + incl - sum;
        for (uint32_t k = 0; k < per; k++) if (b0 + k < q.P) { pre[b0 + k] = run; cur[b0 + k] = run; run += cnt[b0 + k]; }
    }
    __syncthreads();
    ps_digits<CC, CW>(q, i, live, [&](int w, uint32_t m1, uint32_t neg, bool nz) {
        const uint32_t key = nz ? (uint32_t)w * q.key_wstride + m1 : 0u;
        const uint32_t pos = lds_inc_agg(cur, key >> q.part_log, nz);
        if (nz) stage[pos] = make_uint2(key, (q.val_base + (uint32_t)w * q.val_wstride + (uint32_t)i) | (neg << 31));
    });
    __syncthreads();
    uint32_t total = 0;
    for (uint32_t wv = 0; wv < PS_TILE / 64; wv++) total += wave_tot[wv];
    for (uint32_t k = threadIdx.x; k < total; k += blockDim.x) {
        const uint2 pr = stage[k];
        const uint32_t p = pr.x >> q.part_log;
        pairs[(size_t)goff[p] + (k - pre[p])] = pr;
    }
}

// P4: one block per partition of 2^part_log buckets
// (WC = false: the direct placement keeps 8 pairs in registers: two blocks share a CU; WC = true: 16 staged pairs per thread, one block per CU)
template <bool WC>
__global__ void __launch_bounds__(1024, WC ? 4 : 8) k_ps_bucket(const uint2 *__restrict__ pairs, const uint32_t *__restrict__ off1, uint32_t ntiles, uint32_t P, uint32_t NB, int part_log,
                                                    uint32_t *__restrict__ off, uint32_t *__restrict__ entries,
                                                    uint32_t heavy_thr, uint32_t *__restrict__ heavy, uint32_t heavy_cap, const uint32_t *__restrict__ dyn) {
    if (dyn) heavy_thr = dyn[DYN_HEAVY];
    __shared__ uint32_t cnt[PS_PART];
    __shared__ uint32_t wave_tot[17];
    const uint32_t p = blockIdx.x, PB = 1u << part_log, mask = PB - 1;
    const uint32_t lo = off1[(size_t)p * ntiles], hi = off1[(size_t)(p + 1) * ntiles];
    for (uint32_t j = threadIdx.x; j < PS_PART; j += blockDim.x) cnt[j] = 0;
    __syncthreads();
    constexpr int U = WC ? 4 : 8;                                     // loads in flight per thread
    for (uint32_t base = lo; base < hi; base += U * 1024) {
        uint32_t key[U];
#pragma unroll
        for (int j = 0; j < U; j++) { const uint32_t k = base + j * 1024 + threadIdx.x; key[j] = k < hi ? pairs[k].x : 0xffffffffu; }
#pragma unroll
        for (int j = 0; j < U; j++) (void)lds_inc_agg(cnt, key[j] & mask, key[j] != 0xffffffffu);
    }
    __syncthreads();
    // exclusive scan of the (up to 2048) bins: two per thread
    const uint32_t c0 = cnt[2 * threadIdx.x], c1 = cnt[2 * threadIdx.x + 1];
    const uint32_t sum = c0 + c1;
    uint32_t incl = sum;
    for (int d = 1; d < 64; d <<= 1) { uint32_t t = __shfl_up(incl, d, 64); if ((int)(threadIdx.x & 63) >= d) incl += t; }
    if ((threadIdx.x & 63) == 63) wave_tot[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t basep = lo;
    for (uint32_t wv = 0; wv < (threadIdx.x >> 6); wv++) basep += wave_tot[wv];
    const uint32_t e0 = basep + incl - sum, e1 = e0 + c0;
    __syncthreads();
    cnt[2 * threadIdx.x] = e0; cnt[2 * threadIdx.x + 1] = e1;            // cursors
    const uint32_t j0 = 2 * threadIdx.x, k0 = p * PB + j0;
    if (j0 < PB && k0 < NB) { off[k0] = e0; if (c0 >= heavy_thr) { uint32_t h = atomicAdd(&heavy[0], 1u); if (h < heavy_cap) heavy[1 + h] = k0; } }
    if (j0 + 1 < PB && k0 + 1 < NB) { off[k0 + 1] = e1; if (c1 >= heavy_thr) { uint32_t h = atomicAdd(&heavy[0], 1u); if (h < heavy_cap) heavy[1 + h] = k0 + 1; } }
    if (p == P - 1 && threadIdx.x == 0) off[NB] = hi;
    __syncthreads();
    // Placement.  A partition of a few tens of thousands of pairs (n <= 2^22 at c = 20) keeps its open cache lines — one per bucket cursor — in L2
    // while the block fills them, and every term goes straight to its slot.  Beyond that the resident blocks hold more open lines than the L2s
    // do, lines leave half written and come back (the kernel ran 1.9x worse than linear at n = 2^24): there (wc != 0) the pairs are taken in
    // tiles of PS_WC_TILE, grouped by bucket in LDS, and leave as contiguous runs per bucket (write combining).
    if constexpr (!WC) {
        // the partition's slots are ONE contiguous range of entries[] (its buckets are consecutive): the values are placed in LDS at their slot's
        // distance from the range start and leave as whole wave-wide stores — the direct form issued one 4-byte store per pair, each to a different
        // cache line of the 512 ... 2048 open ones (13.6 M L2 transactions at n = 2^20).  Slots past PS_DIRECT_CAP go straight to memory.
        extern __shared__ __align__(16) uint32_t dv_lds[];
        for (uint32_t base = lo; base < hi; base += U * 1024) {
            uint2 pr[U];
#pragma unroll
            for (int j = 0; j < U; j++) { const uint32_t k = base + j * 1024 + threadIdx.x; pr[j] = k < hi ? pairs[k] : make_uint2(0xffffffffu, 0u); }
#pragma unroll
            for (int j = 0; j < U; j++) {
                const bool on = pr[j].x != 0xffffffffu; const uint32_t pos = lds_inc_agg(cnt, pr[j].x & mask, on);
                if (on) { const uint32_t r = pos - lo; if (r < (uint32_t)PS_DIRECT_CAP) dv_lds[r] = pr[j].y; else entries[pos] = pr[j].y; }
            }
        }
        __syncthreads();
        const uint32_t staged = hi - lo < (uint32_t)PS_DIRECT_CAP ? hi - lo : (uint32_t)PS_DIRECT_CAP;
        for (uint32_t k = threadIdx.x; k < staged; k += 1024) entries[lo + k] = dv_lds[k];
        return;
    } else {
    extern __shared__ __align__(16) uint32_t wc_lds[];
    uint32_t *lcnt = wc_lds, *lpre = wc_lds + PS_PART;           // per tile: pairs per bucket, their exclusive prefix
    uint2 *stage = reinterpret_cast<uint2 *>(wc_lds + 2 * PS_PART);   // PS_WC_TILE x (value, slot in entries[])
    constexpr int V = PS_WC_TILE / 1024;                         // pairs per thread and tile
    for (uint32_t base = lo; base < hi; base += PS_WC_TILE) {
        lcnt[2 * threadIdx.x] = 0; lcnt[2 * threadIdx.x + 1] = 0;
        __syncthreads();
        uint2 pr[V]; uint32_t rank[V];
#pragma unroll
        for (int j = 0; j < V; j++) { const uint32_t k = base + j * 1024 + threadIdx.x; pr[j] = k < hi ? pairs[k] : make_uint2(0xffffffffu, 0u); }
#pragma unroll
        for (int j = 0; j < V; j++) rank[j] = lds_inc_agg(lcnt, pr[j].x & mask, pr[j].x != 0xffffffffu);       // position inside the tile's share of its bucket
        __syncthreads();
        const uint32_t l0 = lcnt[2 * threadIdx.x], l1 = lcnt[2 * threadIdx.x + 1];
        const uint32_t ls = l0 + l1;
        uint32_t li = ls;
        for (int d = 1; d < 64; d <<= 1) { uint32_t t = __shfl_up(li, d, 64); if ((int)(threadIdx.x & 63) >= d) li += t; }
        if ((threadIdx.x & 63) == 63) wave_tot[threadIdx.x >> 6] = li;
        __syncthreads();
        uint32_t lb = 0;
        for (uint32_t wv = 0; wv < (threadIdx.x >> 6); wv++) lb += wave_tot[wv];
        lpre[2 * threadIdx.x] = lb + li - ls; lpre[2 * threadIdx.x + 1] = lb + li - ls + l0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < V; j++)
            if (pr[j].x != 0xffffffffu) { const uint32_t bk = pr[j].x & mask; stage[lpre[bk] + rank[j]] = make_uint2(pr[j].y, cnt[bk] + rank[j]); }
        __syncthreads();
        cnt[2 * threadIdx.x] += l0; cnt[2 * threadIdx.x + 1] += l1;                      // the cursors move past this tile
        const uint32_t tile_n = hi - base < (uint32_t)PS_WC_TILE ? hi - base : (uint32_t)PS_WC_TILE;
        for (uint32_t q = threadIdx.x; q < tile_n; q += 1024) { const uint2 e = stage[q]; entries[e.y] = e.x; }       // neighbours in q are neighbours in a bucket: whole runs per store
        __syncthreads();
    }
    }
}

}  // namespace msm
