// crypto_amd/csrc/dock_dev.hip — the DEVELOPMENT surface (include/dock_gpu_dev.h): tuning knobs, stage timers and self-test hooks.  Linked into
// crypto_amd/libdock_gpu_dev.so only (the twin the tests, tools/ and bench.py's stage / roofline leg load); the product library libdock_gpu.so
// exports none of these symbols (tests/test_abi_host.py asserts both) and runs every knob at its default.
#include "msm_driver.hip.h"
#include "acc_launch.hip.h"
#include "qap_launch.hip.h"
#include "selftest_launch.hip.h"
#include "../../include/dock_gpu_dev.h"

using namespace dock;

#include "dev_sort_hooks.hip.h"      // dgpu_selftest_psort, _sort_sweep, _scan, _dyn_chunk, _choose_chunk: the MSM sort stage on its own

extern "C" {

int32_t dgpu_set_window_bits(int32_t c) { if (c != 0 && (c < 7 || c > 22)) return DGPU_E_BADARG; gs.window_bits = c; return DGPU_OK; }
int32_t dgpu_set_chunk(int32_t terms) { if (terms != 0 && (terms < 16 || terms > 4096)) return DGPU_E_BADARG; gs.chunk = terms; return DGPU_OK; }
int32_t dgpu_set_many_chunk_rows(int32_t rows) { if (rows < 0 || rows > 65535) return DGPU_E_BADARG; gs.many_chunk = rows; return DGPU_OK; }
int32_t dgpu_set_msm_segments(int32_t fold, int32_t chunk_terms) { if (fold < 0 || fold > 2 || chunk_terms < 0 || chunk_terms > (1 << 20)) return DGPU_E_BADARG; gs.seg_fold = fold; gs.seg_chunk = chunk_terms; return DGPU_OK; }
int32_t dgpu_set_gt_pow(int32_t groups_per_wave, int32_t bases_per_group, int32_t chunk_elems) {
    if (groups_per_wave < 0 || groups_per_wave > 10 || bases_per_group < 0 || bases_per_group > 8 || chunk_elems < 0 || chunk_elems > 65536) return DGPU_E_BADARG;
    gs.gt_pow_g = groups_per_wave; gs.gt_pow_k = bases_per_group; gs.gt_pow_chunk = chunk_elems; return DGPU_OK;
}
int32_t dgpu_set_wm_many(int32_t chunk_rows, int32_t rows_per_block) {
    if (chunk_rows < 0 || chunk_rows > 4096 || rows_per_block < 0 || rows_per_block > 512) return DGPU_E_BADARG;
    gs.wm_many_chunk = chunk_rows; gs.wm_many_rpb = rows_per_block; return DGPU_OK;
}
int32_t dgpu_dev_set_acc_split(int32_t chunks) { if (chunks < 0 || chunks > (int32_t)acck::ACC_MAX_SPLIT) return DGPU_E_BADARG; gs.acc_split = chunks; return DGPU_OK; }
int32_t dgpu_dev_get_acc_split(void) { return gs.acc_last_split.load(); }
int32_t dgpu_dev_set_acc_d_pass(int32_t entries) { if (entries < 0) return DGPU_E_BADARG; gs.acc_d_pass = entries; return DGPU_OK; }
int32_t dgpu_dev_set_acc_d_unroll(int32_t non_members_per_lane) { if (non_members_per_lane != 0 && non_members_per_lane != 1 && non_members_per_lane != 4) return DGPU_E_BADARG; gs.acc_d_unroll = non_members_per_lane; return DGPU_OK; }
int32_t dgpu_dev_get_acc_d_unroll(void) { return gs.acc_d_last_unroll.load(); }
int32_t dgpu_dev_set_ntt(int32_t path, const int32_t *split, int32_t n_split) { return ntt::dev_set_ntt(path, split, n_split) ? DGPU_OK : DGPU_E_BADARG; }
int32_t dgpu_dev_get_ntt_last(int32_t *path, int32_t *groups, int32_t cap) {
    if (!path || cap < 0 || (cap > 0 && !groups)) return DGPU_E_BADARG;
    int route = 0; const int n = ntt::dev_get_ntt_last(&route, groups, cap);
    *path = route; return n;
}
// the chunking and the heavy-bucket count the last bucket MSM left in its slot's accumulate workspace (sl.dyn, sl.heavy: grow-only, never cleared).  The slots
// are handed out in turn (SlotLock: cx.rr), so with one call at a time the slot of the last call is rr - 1; read only, nothing of the product's state changes
int32_t dgpu_dev_get_acc_last(uint32_t out[6]) {
    if (!out) return DGPU_E_BADARG;
    Ctx &cx = cur();
    if (!cx.ready) return DGPU_E_NODEVICE;
    const unsigned taken = cx.rr.load();
    if (!taken) return DGPU_E_BADARG;                              // no call has taken a slot yet
    Slot &sl = cx.slots[(taken - 1) % N_SLOTS];
    std::lock_guard<std::mutex> lk(sl.mu);
    if (!sl.stream || !sl.dyn.p || !sl.heavy.p || sl.dyn.cap < (size_t)msm::DYN_MULTI * 4 || sl.heavy.cap < 4) return DGPU_E_BADARG;
    HIPCHK(hipSetDevice(cx.device));
    HIPCHK(hipStreamSynchronize(sl.stream));
    uint32_t w[6];
    HIPCHK(hipMemcpy(w, sl.dyn.p, (size_t)msm::DYN_MULTI * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(w + 5, sl.heavy.p, 4, hipMemcpyDeviceToHost));
    const uint32_t ch = w[msm::DYN_CH], E = w[msm::DYN_E];
    // a workspace that was reserved but never used holds whatever the allocation held: k_dyn_chunk's words always satisfy these relations
    if (ch < 16 || w[msm::DYN_HEAVY] != 16u * ch || w[msm::DYN_T] != (uint32_t)(((uint64_t)E + ch - 1) / ch)) return DGPU_E_BADARG;
    out[0] = ch; out[1] = w[msm::DYN_T]; out[2] = w[msm::DYN_HEAVY]; out[3] = E; out[4] = w[msm::DYN_NMULTI]; out[5] = w[5];
    return DGPU_OK;
}
int32_t dgpu_dev_set_saver_fp_bits(int32_t bits) { if (bits < -1 || bits > 63) return DGPU_E_BADARG; gs.saver_fp_bits = bits; return DGPU_OK; }
int32_t dgpu_set_reduce_lanes(int32_t lanes) { if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4) return DGPU_E_BADARG; gs.reduce_lanes = lanes; return DGPU_OK; }
int32_t dgpu_set_reduce_shift(int32_t sh) { if (sh < -1 || sh > 6) return DGPU_E_BADARG; gs.reduce_shift = sh; return DGPU_OK; }
int32_t dgpu_set_miller_pipeline(int32_t mode) {       // bits 0-4: forms; bits 8-13 / 16-21: where the chain is cut (0: default); bits 24-27: slice length of the last piece's products (0: automatic); bits 28-29: log2 of the factor on the block limit of k_line_products3
    if (mode < 0 || (mode & ~0x3F3F3F1F)) return DGPU_E_BADARG;
    const int a = (mode >> 8) & 63, b = (mode >> 16) & 63;
    if ((a || b) && !(a > b && b > 0 && a < 62)) return DGPU_E_BADARG;
    gs.ml_mode = mode; return DGPU_OK;
}

int32_t dgpu_prof_enable(int32_t on) { gs.prof = on != 0; return DGPU_OK; }
int32_t dgpu_prof_reset(void) { std::lock_guard<std::mutex> lk(gs.mu); gs.prof_tab.clear(); gs.allocs_at_reset = g_dev_allocs.load(); gs.alloc_ns_at_reset = g_dev_alloc_ns.load(); return DGPU_OK; }
int32_t dgpu_prof_read(const char **names, double *total_ms, uint64_t *calls, int32_t cap) {
    std::lock_guard<std::mutex> lk(gs.mu);
    int32_t k = 0;
    for (auto &t : gs.prof_tab) { if (k >= cap) break; names[k] = t.name; total_ms[k] = t.ms; calls[k] = t.calls; k++; }
    // device allocations since the last dgpu_prof_reset (counted whether or not the stage timers are enabled): 0 calls in steady state
    if (k < cap) { names[k] = "hipMalloc"; total_ms[k] = (double)(g_dev_alloc_ns.load() - gs.alloc_ns_at_reset) * 1e-6; calls[k] = g_dev_allocs.load() - gs.allocs_at_reset; k++; }
    return k;
}

int32_t dgpu_selftest_fp_mul(const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out) {
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    void *da, *db, *dout;
    HIPCHK(dev_malloc(&da, n * 48 + 16)); HIPCHK(dev_malloc(&db, n * 48 + 16)); HIPCHK(dev_malloc(&dout, n * 48 + 16));
    HIPCHK(hipMemcpy(da, a, n * 48, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(db, b, n * 48, hipMemcpyHostToDevice));
    selftest::launch_selftest_fp_mul(sl.stream, (const uint32_t *)da, (const uint32_t *)db, n, (uint32_t *)dout);
    HIPCHK(hipStreamSynchronize(sl.stream));
    HIPCHK(hipMemcpy(out, dout, n * 48, hipMemcpyDeviceToHost));
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    return DGPU_OK;
}
int32_t dgpu_selftest_g1_sum(const uint64_t *pts, const uint8_t *neg, size_t n, uint64_t out[18]) {
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    void *dp, *dn, *dout, *dinf;
    HIPCHK(dev_malloc(&dp, n * 96 + 16)); HIPCHK(dev_malloc(&dn, n + 16)); HIPCHK(dev_malloc(&dout, 4 * 48)); HIPCHK(dev_malloc(&dinf, 16));
    HIPCHK(hipMemcpy(dp, pts, n * 96, hipMemcpyHostToDevice));
    if (neg) HIPCHK(hipMemcpy(dn, neg, n, hipMemcpyHostToDevice)); else HIPCHK(hipMemsetAsync(dn, 0, n + 16, sl.stream));      // (on the kernel's stream, as below)
    selftest::launch_selftest_g1_sum(sl.stream, (const uint32_t *)dp, (const uint8_t *)dn, n, (uint32_t *)dout, (uint8_t *)dinf);
    HIPCHK(hipStreamSynchronize(sl.stream));
    uint64_t w[24]; uint8_t inf;
    HIPCHK(hipMemcpy(w, dout, 4 * 48, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&inf, dinf, 1, hipMemcpyDeviceToHost));
    (void)hipFree(dp); (void)hipFree(dn); (void)hipFree(dout); (void)hipFree(dinf);
    uint8_t finf = inf;
    host_fold<hostf::Fq>(w, &finf, 1, 1, out);
    return DGPU_OK;
}
// one arithmetic function of the device headers per call (selftest_kernels.hip.h): n rows of in_words u64 in, out_words u64 out
int32_t dgpu_selftest_arith(int32_t op, int32_t stress, const uint64_t *in, size_t in_words, size_t n, uint64_t *out, size_t out_words) {
    size_t iw = 0, ow = 0;
    if (!selftest::selftest_arith_shape(op, stress, &iw, &ow) || iw != in_words || ow != out_words || (n && (!in || !out)) || n > ((size_t)1 << 24)) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    if (!n) return DGPU_OK;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    void *din, *dout;
    HIPCHK(dev_malloc(&din, n * iw * 8 + 16)); HIPCHK(dev_malloc(&dout, n * ow * 8 + 16));
    HIPCHK(hipMemcpy(din, in, n * iw * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(dout, 0, n * ow * 8, sl.stream));      // (on the kernel's stream: the slot streams do not wait for the null stream, and a memset there can land on the kernel's output)
    selftest::launch_selftest_arith(sl.stream, op, stress, (const uint32_t *)din, n, (uint32_t *)dout);
    HIPCHK(hipStreamSynchronize(sl.stream));
    HIPCHK(hipMemcpy(out, dout, n * ow * 8, hipMemcpyDeviceToHost));
    (void)hipFree(din); (void)hipFree(dout);
    return DGPU_OK;
}
// host self-test hook: the GLV split the scaling kernel is fed with (k mod r = k1 + k2 lambda, both < 2^128)
int32_t dgpu_selftest_glv_decompose(const uint64_t k[4], uint64_t k1[2], uint64_t k2[2]) {
    if (!k || !k1 || !k2) return DGPU_E_BADARG;
    hostf::glv_decompose(k, k1, k2);
    return DGPU_OK;
}
// host self-test hook: the GLS split the G2 scaling and fold kernels are fed with (k mod r = d0 + d1 |x| + d2 |x|^2 + d3 |x|^3, d0 .. d2 < |x|)
int32_t dgpu_selftest_gls4_decompose(const uint64_t k[4], uint64_t d[4]) {
    if (!k || !d) return DGPU_E_BADARG;
    hostf::gls4_decompose(k, d);
    return DGPU_OK;
}

}  // extern "C"
