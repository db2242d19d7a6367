// crypto_amd/csrc/k_ntt.hip — translation unit of the Fr NTT / witness-map kernels.
#include <atomic>
#include "ntt_kernels.hip.h"
#include "qap_launch.hip.h"
#include "ntt_plan.hpp"
namespace ntt {
static inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
void launch_fr_mont_to_canonical(hipStream_t s, uint32_t *words, size_t n) { hipLaunchKernelGGL(k_fr_mont_to_canonical, grid_for(n), dim3(256), 0, s, words, n); }
void launch_fr_canonical_to_mont(hipStream_t s, uint32_t *words, size_t n) { hipLaunchKernelGGL(k_fr_canonical_to_mont, grid_for(n), dim3(256), 0, s, words, n); }
void launch_fr_load(hipStream_t s, const uint32_t *words, size_t n, int mont, uint32_t *out, size_t D) { hipLaunchKernelGGL(k_fr_load, grid_for(D), dim3(256), 0, s, words, n, mont, out, D); }
void launch_fr_powers(hipStream_t s, const uint32_t *bw, const uint32_t *sw, size_t count, uint32_t *out) { hipLaunchKernelGGL(k_fr_powers, grid_for(count), dim3(256), 0, s, bw, sw, count, out); }
void launch_tw_compact(hipStream_t s, uint32_t *tw, size_t H) {
    if (H > 1) hipLaunchKernelGGL(k_tw_compact, grid_for(H), dim3(256), 0, s, tw, H, 0);
}
void launch_csr_eval(hipStream_t s, const uint64_t *rowptr, const uint32_t *cols, const uint32_t *vals_soa, size_t nnz, const uint32_t *z_words, int z_mont, size_t nvars, size_t rows, size_t extra, uint32_t *out, size_t D) {
    hipLaunchKernelGGL(k_csr_eval, grid_for(D), dim3(256), 0, s, rowptr, cols, vals_soa, nnz, z_words, z_mont, nvars, rows, extra, out, D);
}
// ---- development knob (dgpu_dev_set_ntt / dgpu_dev_get_ntt_last, include/dock_gpu_dev.h; the product never calls the setter, so it runs path 0 and no split) ----
// forced route, forced split of the piped passes (4 bits per entry, DIF order, the count in bits 48-51) and what the last transform ran (the same packing in
// launch order, the route in bits 56-57); read / written on every call
static std::atomic<int> g_path{0};
static std::atomic<uint64_t> g_split{0}, g_last{0};
static inline uint64_t pack_groups(const int *g, int n) { uint64_t w = (uint64_t)n << 48; for (int k = 0; k < n && k < 12; k++) w |= (uint64_t)(g[k] & 15) << (4 * k); return w; }
bool dev_set_ntt(int path, const int32_t *split, int n_split) {
    if (path < 0 || path > 2 || n_split < 0 || n_split > PLAN_PIPE_MAX_GROUPS || (n_split > 0 && !split)) return false;
    int g[PLAN_PIPE_MAX_GROUPS];
    for (int k = 0; k < n_split; k++) { if (split[k] < 1 || split[k] > PLAN_PIPE_TILE_LOG) return false; g[k] = split[k]; }
    g_path = path; g_split = pack_groups(g, n_split);
    return true;
}
int dev_get_ntt_last(int *path, int32_t *groups, int cap) {
    const uint64_t w = g_last.load();
    const int route = (int)(w >> 56) & 3, n = (int)(w >> 48) & 63;
    *path = route;
    for (int k = 0; k < n && k < cap; k++) groups[k] = route == NTT_ROUTE_PER_STAGE ? 1 : (int)(w >> (4 * k)) & 15;      // per stage: log2 D launches of one stage
    return n;
}
static inline void note_last(int route, const int *g, int n) { g_last = (uint64_t)route << 56 | (route == NTT_ROUTE_PER_STAGE ? (uint64_t)n << 48 : pack_groups(g, n)); }
static_assert(PLAN_PIPE_TILE_LOG == PIPE_TILE_LOG && PLAN_PIPE_MAX_LOGN == PIPE_MAX_LOGN && PLAN_FUSE_TILE_LOG == FUSE_TILE_LOG, "ntt_plan.hpp plans for the tiles of ntt_kernels.hip.h");
// in_pointwise: bufs = {a, b, c}, pre = zinv words, the transform runs over a only (see k_ntt_r4); post / out_words: the last pass writes scalars
static bool run_passes(hipStream_t s, uint32_t *const *bufs, int nbuf, int logn, const uint32_t *tw, int dif, const uint32_t *pre, bool in_pointwise, const uint32_t *post, uint32_t *out_words) {
    const size_t D = (size_t)1 << logn, H = D >> 1;
    const int path = g_path.load();
    const bool per_stage = logn < PIPE_TILE_LOG || path == NTT_ROUTE_PER_STAGE;                                                  // tiny domains: one pass per stage
    const bool staged = !per_stage && (logn > PIPE_MAX_LOGN || (path == NTT_ROUTE_STAGED && logn >= FUSE_TILE_LOG));           // (32-bit buffer offsets: arrays beyond 4 GB take the staged kernel)
    if ((in_pointwise || post) && (per_stage || staged)) return false;   // the caller runs the separate kernels
    if (per_stage) {
        for (int b = 0; b < nbuf; b++) {
            if (pre) hipLaunchKernelGGL(k_coset_scale, grid_for(D), dim3(256), 0, s, bufs[b], logn, pre, (uint32_t *)nullptr, 1);
            for (int st = 0; st < logn; st++) hipLaunchKernelGGL(k_ntt_stage, grid_for(H), dim3(256), 0, s, bufs[b], logn, st, tw, dif);
        }
        note_last(NTT_ROUTE_PER_STAGE, nullptr, logn);
        return true;
    }
    if (staged) {
        const size_t lds_bytes = (size_t)NL * (1u << FUSE_TILE_LOG) * 4;      // 80 KB
        // (the attribute belongs to the function ON THE CURRENT DEVICE: a process that drives several GPUs sets it once per device)
        { static std::atomic<uint32_t> done{0}; int dev = 0; (void)hipGetDevice(&dev); const uint32_t bit = 1u << (dev & 31);
          if (!(done.load() & bit)) { (void)hipFuncSetAttribute((const void *)k_ntt_fused, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); done.fetch_or(bit); } }
        int groups[PLAN_FUSE_MAX_GROUPS];
        const int ng = plan_staged(logn, dif, groups);
        const unsigned tiles = (unsigned)(D >> FUSE_TILE_LOG);
        for (int b = 0; b < nbuf; b++) { int s0 = 0; for (int gidx = 0; gidx < ng; gidx++) { hipLaunchKernelGGL(k_ntt_fused, dim3(tiles), dim3(FUSE_THREADS), lds_bytes, s, bufs[b], logn, s0, groups[gidx], tw, dif, gidx == 0 ? pre : (const uint32_t *)nullptr); s0 += groups[gidx]; } }
        note_last(NTT_ROUTE_STAGED, groups, ng);
        return true;
    }
    // Pipelined passes (the schedule: plan_piped, ntt_plan.hpp)
    constexpr int tile_log = PIPE_TILE_LOG;
    int groups[PLAN_PIPE_MAX_GROUPS];
    int ng = plan_piped(logn, dif, groups);
    if (const uint64_t sp = g_split.load()) {            // a forced split, e.g. 6,6,8: strided passes then the flat one (the order is reversed for DIT); only for the domain it sums to
        const int n = (int)(sp >> 48) & 15; int sum = 0;
        for (int k = 0; k < n; k++) sum += (int)(sp >> (4 * k)) & 15;
        if (sum == logn) { ng = n; for (int k = 0; k < n; k++) groups[dif ? k : n - 1 - k] = (int)(sp >> (4 * k)) & 15; }
    }
    const size_t lds_bytes = (size_t)NL * ((size_t)1 << tile_log) * 4;
    { static std::atomic<uint32_t> done{0}; int dev = 0; (void)hipGetDevice(&dev); const uint32_t bit = 1u << (dev & 31);
      if (!(done.load() & bit)) {
          (void)hipFuncSetAttribute((const void *)k_ntt_r4<true, PIPE_TILE_LOG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
          (void)hipFuncSetAttribute((const void *)k_ntt_r4<false, PIPE_TILE_LOG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
          done.fetch_or(bit); } }
    NttBatch B; for (int b = 0; b < 3; b++) B.buf[b] = bufs[b < nbuf ? b : 0];
    const unsigned tiles = (unsigned)(D >> tile_log), total = tiles * (unsigned)(in_pointwise ? 1 : nbuf);
    const dim3 blk(1u << (tile_log - 2));
    int s0 = 0;
    for (int gidx = 0; gidx < ng; gidx++) {
        const uint32_t *pr = gidx == 0 ? pre : (const uint32_t *)nullptr;
        const int im = (gidx == 0 && in_pointwise) ? NTT_IN_POINTWISE : 0, om = (gidx == ng - 1 && post) ? NTT_OUT_WORDS : 0;
        if (dif) hipLaunchKernelGGL((k_ntt_r4<true, PIPE_TILE_LOG>), dim3(total), blk, lds_bytes, s, B, logn, s0, groups[gidx], tw, pr, im, om, post, out_words);
        else hipLaunchKernelGGL((k_ntt_r4<false, PIPE_TILE_LOG>), dim3(total), blk, lds_bytes, s, B, logn, s0, groups[gidx], tw, pr, im, om, post, out_words);
        s0 += groups[gidx];
    }
    note_last(NTT_ROUTE_PIPED, groups, ng);
    return true;
}
void launch_ntt_batch(hipStream_t s, uint32_t *const *bufs, int nbuf, int logn, const uint32_t *tw, int dif, const uint32_t *pre) {
    (void)run_passes(s, bufs, nbuf, logn, tw, dif, pre, false, nullptr, nullptr);
}
// h = coset iFFT of (a b - c) / Z(g), written as canonical scalars in natural order: a <- iDFT((a b - c) zinv) (bit-reversed), out[k] = a[rev k] pw[rev k]
void launch_ntt_final(hipStream_t s, uint32_t *a, uint32_t *b, uint32_t *c, int logn, const uint32_t *tw_i, const uint32_t *zinv_words, const uint32_t *pw_data_order, uint32_t *out_words) {
    uint32_t *bufs[3] = {a, b, c};
    if (run_passes(s, bufs, 3, logn, tw_i, 1, zinv_words, true, pw_data_order, out_words)) return;
    launch_pointwise(s, a, b, c, (size_t)1 << logn, zinv_words);
    launch_ntt(s, a, logn, tw_i, 1);
    launch_coset_scale(s, a, logn, pw_data_order, out_words, 1);
}
void launch_ntt(hipStream_t s, uint32_t *buf, int logn, const uint32_t *tw, int dif, const uint32_t *pre) { uint32_t *b[1] = {buf}; launch_ntt_batch(s, b, 1, logn, tw, dif, pre); }
void launch_coset_scale(hipStream_t s, uint32_t *buf, int logn, const uint32_t *pw, uint32_t *out_words, int pw_in_data_order) { hipLaunchKernelGGL(k_coset_scale, grid_for((size_t)1 << logn), dim3(256), 0, s, buf, logn, pw, out_words, pw_in_data_order); }
void launch_bitrev_table(hipStream_t s, const uint32_t *src, uint32_t *dst, int logn) { hipLaunchKernelGGL(k_bitrev_table, grid_for((size_t)1 << logn), dim3(256), 0, s, src, dst, logn); }
void launch_pointwise(hipStream_t s, uint32_t *a, const uint32_t *b, const uint32_t *c, size_t D, const uint32_t *zinv_words) { hipLaunchKernelGGL(k_pointwise, grid_for(D), dim3(256), 0, s, a, b, c, D, zinv_words); }
}  // namespace ntt
