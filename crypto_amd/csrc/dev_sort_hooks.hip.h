// crypto_amd/csrc/dev_sort_hooks.hip.h — self-test hooks of the MSM sort stage (include/dock_gpu_dev.h: dgpu_selftest_psort, _sort_sweep, _scan, _dyn_chunk,
// _choose_chunk).  Included by dock_dev.hip at file scope: the development twin only.  Every device hook takes a slot, allocates buffers of its
// own, fills each output buffer and DGPU_SELFTEST_GUARD words behind it with DGPU_SELFTEST_SENTINEL on the slot's stream, runs the PRODUCT's launchers
// (sort_launch.hip.h) with the geometry the product's drivers compute (msm_driver.hip.h), copies everything back, guards included, and frees its buffers.
// Nothing here is reachable from libdock_gpu.so.

namespace {
constexpr size_t ST_G = DGPU_SELFTEST_GUARD;
struct StDevMem {                        // the hook's allocations: freed when it returns, on every path
    std::vector<void *> all;
    ~StDevMem() { for (void *p : all) (void)hipFree(p); }
    template <class T> hipError_t get(T **p, size_t elems) {
        void *v = nullptr;
        const hipError_t e = dev_malloc(&v, (elems ? elems : 1) * sizeof(T) + 16);
        if (e == hipSuccess) all.push_back(v);
        *p = (T *)v;
        return e;
    }
};
inline hipError_t st_fill(hipStream_t s, uint32_t *p, size_t words) { return hipMemsetD32Async((hipDeviceptr_t)p, (int)DGPU_SELFTEST_SENTINEL, words, s); }
}  // namespace

extern "C" {

int32_t dgpu_selftest_choose_chunk(uint64_t E, int32_t min_chunk, uint64_t max_chunks, int32_t lanes_per_chunk, uint64_t nb_shared) {
    if (min_chunk < 1 || lanes_per_chunk < 1 || lanes_per_chunk > (int32_t)msm::RESIDENT_ACC_LANES) return DGPU_E_BADARG;
    return choose_chunk((size_t)E, min_chunk, (size_t)max_chunks, lanes_per_chunk, (size_t)nb_shared);
}

int32_t dgpu_selftest_dyn_chunk(uint32_t E, uint32_t fixed_ch, uint32_t min_chunk, uint32_t max_chunks, uint32_t lanes_per_chunk, uint32_t T_max, uint32_t nb_shared, uint32_t *dyn) {
    if (!dyn || min_chunk < 1 || lanes_per_chunk < 1 || lanes_per_chunk > msm::RESIDENT_ACC_LANES) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    StDevMem mem; uint32_t *d_tot, *d_dyn;
    HIPCHK(mem.get(&d_tot, 1)); HIPCHK(mem.get(&d_dyn, msm::DYN_MULTI + ST_G));
    HIPCHK(hipMemcpyAsync(d_tot, &E, 4, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(st_fill(sl.stream, d_dyn, msm::DYN_MULTI + ST_G));
    msm::launch_dyn_chunk(sl.stream, d_tot, fixed_ch, min_chunk, max_chunks, lanes_per_chunk, T_max, d_dyn, nb_shared);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sl.stream));
    HIPCHK(hipMemcpy(dyn, d_dyn, (msm::DYN_MULTI + ST_G) * 4, hipMemcpyDeviceToHost));
    return DGPU_OK;
}

int32_t dgpu_selftest_scan(const uint32_t *cnt, size_t NB, int32_t with_cursor, uint32_t *off, uint32_t *cursor) {
    if (!cnt || !off || NB < 1 || NB > ((size_t)1 << 26) || (with_cursor && !cursor)) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    StDevMem mem; uint32_t *d_cnt, *d_off, *d_cur = nullptr, *d_bs;
    const size_t nblk = msm::scan_blocks(NB);
    HIPCHK(mem.get(&d_cnt, NB)); HIPCHK(mem.get(&d_off, NB + 1 + ST_G)); HIPCHK(mem.get(&d_bs, nblk + 2));
    if (with_cursor) HIPCHK(mem.get(&d_cur, NB + ST_G));
    HIPCHK(hipMemcpyAsync(d_cnt, cnt, NB * 4, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(st_fill(sl.stream, d_off, NB + 1 + ST_G));
    if (with_cursor) HIPCHK(st_fill(sl.stream, d_cur, NB + ST_G));
    msm::launch_scan(sl.stream, d_cnt, d_off, d_cur, d_bs, NB);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sl.stream));
    HIPCHK(hipMemcpy(off, d_off, (NB + 1 + ST_G) * 4, hipMemcpyDeviceToHost));
    if (with_cursor) HIPCHK(hipMemcpy(cursor, d_cur, (NB + ST_G) * 4, hipMemcpyDeviceToHost));
    return DGPU_OK;
}

int32_t dgpu_selftest_psort(const uint32_t *scalars, size_t n, int32_t c, int32_t W, uint32_t key_wstride, uint32_t val_base, uint32_t val_wstride,
                            const uint8_t *idflag, uint32_t flag_base, uint32_t heavy_thr, uint32_t heavy_cap, const uint32_t *dyn_args, int32_t place,
                            uint32_t *off, uint32_t *entries, uint32_t *heavy, uint32_t *dyn, uint32_t *bad, int32_t *placed) {
    if (!scalars || !off || !entries || !heavy || !bad || !placed || (dyn_args && !dyn)) return DGPU_E_BADARG;
    if (c < 16 || c > 22 || W != 255 / c + 1 || W > msm::PS_MAX_W || n < 1 || n > ((size_t)1 << 22) || place < 0 || place > 2 || heavy_cap > (1u << 20)) return DGPU_E_BADARG;
    const uint32_t B = 1u << (c - 1);
    if (key_wstride != 0 && key_wstride != B) return DGPU_E_BADARG;
    if ((uint64_t)val_base + (uint64_t)(W - 1) * val_wstride + n > (1ull << 31) || (uint64_t)flag_base + n > (1ull << 31)) return DGPU_E_BADARG;
    if (dyn_args && (dyn_args[1] < 1 || dyn_args[3] < 1 || dyn_args[3] > msm::RESIDENT_ACC_LANES)) return DGPU_E_BADARG;
    // NB, part_log, P, ntiles: as msm_device_ranges (a bucket set per window) and pre_sort (the one set of a table) compute them
    const uint32_t NB = key_wstride ? (uint32_t)W * B : B;
    msm::PsParams q;
    q.n = n; q.flag_base = flag_base; q.c = c; q.W = W; q.key_wstride = key_wstride; q.val_base = val_base; q.val_wstride = val_wstride;
    q.part_log = msm::ps_part_log(NB); q.P = (NB + (1u << q.part_log) - 1) >> q.part_log; q.ntiles = (uint32_t)((n + msm::PS_TILE - 1) / msm::PS_TILE);
    if (msm::ps_scatter_lds_bytes(q.P, W) > msm::PS_SCATTER_LDS_MAX) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    hipStream_t s = sl.stream;
    const size_t n1 = (size_t)q.P * q.ntiles, E = n * (size_t)W;
    StDevMem mem; uint32_t *d_sc, *d_cnt1, *d_off1, *d_bs, *d_off, *d_ent, *d_heavy, *d_dyn = nullptr, *d_bad; uint2 *d_pairs; uint8_t *d_flag = nullptr;
    HIPCHK(mem.get(&d_sc, n * 8)); HIPCHK(mem.get(&d_cnt1, n1 + 1)); HIPCHK(mem.get(&d_off1, n1 + 1 + ST_G)); HIPCHK(mem.get(&d_bs, msm::scan_blocks(n1) + 2));
    HIPCHK(mem.get(&d_pairs, E)); HIPCHK(mem.get(&d_off, (size_t)NB + 1 + ST_G)); HIPCHK(mem.get(&d_ent, E + ST_G));
    HIPCHK(mem.get(&d_heavy, (size_t)1 + heavy_cap + ST_G)); HIPCHK(mem.get(&d_bad, 1 + ST_G));
    if (dyn_args) HIPCHK(mem.get(&d_dyn, msm::DYN_MULTI + ST_G));
    if (idflag) { HIPCHK(mem.get(&d_flag, (size_t)flag_base + n)); HIPCHK(hipMemcpyAsync(d_flag, idflag, (size_t)flag_base + n, hipMemcpyHostToDevice, s)); }
    HIPCHK(hipMemcpyAsync(d_sc, scalars, n * 32, hipMemcpyHostToDevice, s));
    HIPCHK(st_fill(s, d_off, (size_t)NB + 1 + ST_G)); HIPCHK(st_fill(s, d_ent, E + ST_G)); HIPCHK(st_fill(s, d_heavy, (size_t)1 + heavy_cap + ST_G)); HIPCHK(st_fill(s, d_bad, 1 + ST_G));
    if (dyn_args) HIPCHK(st_fill(s, d_dyn, msm::DYN_MULTI + ST_G));
    HIPCHK(hipMemsetAsync(d_heavy, 0, 4, s)); HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));          // the two words the drivers clear before every sort
    q.scalars = d_sc; q.idflag = d_flag; q.bad = d_bad;
    *placed = msm::launch_psort(s, q, NB, d_cnt1, d_off1, d_bs, d_pairs, d_off, d_ent, heavy_thr, d_heavy, heavy_cap, dyn_args, d_dyn, place);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(off, d_off, ((size_t)NB + 1 + ST_G) * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(entries, d_ent, (E + ST_G) * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(heavy, d_heavy, ((size_t)1 + heavy_cap + ST_G) * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(bad, d_bad, (1 + ST_G) * 4, hipMemcpyDeviceToHost));
    if (dyn_args) HIPCHK(hipMemcpy(dyn, d_dyn, (msm::DYN_MULTI + ST_G) * 4, hipMemcpyDeviceToHost));
    return DGPU_OK;
}

}  // extern "C"

template <class C>
static int32_t st_sort_sweep(const uint32_t *scalars, size_t n, int c, const uint32_t *bases, uint32_t fixed_ch, uint32_t heavy_cap,
                             uint32_t *off, uint32_t *cursor, uint32_t *entries, uint32_t *heavy, uint32_t *dyn, uint32_t *bad) {
    PlainGeom g; int32_t rc;
    if ((rc = plain_geometry_at<C>(n, c, g))) return rc;
    const uint32_t NB = g.NB; const int W = g.W; const AccGeom &a = g.acc;
    const uint32_t HEAVY_CAP = heavy_cap ? heavy_cap : a.HEAVY_CAP;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    hipStream_t s = sl.stream;
    const size_t E = n * (size_t)W, code = g.wide ? 4 : 2;
    StDevMem mem; uint32_t *d_sc, *d_bases = nullptr, *d_cnt, *d_off, *d_cur, *d_bs, *d_ent, *d_heavy, *d_dyn, *d_bad; uint8_t *d_dig;
    HIPCHK(mem.get(&d_sc, n * 8)); HIPCHK(mem.get(&d_dig, (size_t)W * g.n_pad * code)); HIPCHK(mem.get(&d_cnt, (size_t)NB + 1)); HIPCHK(mem.get(&d_off, (size_t)NB + 1 + ST_G));
    HIPCHK(mem.get(&d_cur, (size_t)NB + ST_G)); HIPCHK(mem.get(&d_bs, g.nblk + 2)); HIPCHK(mem.get(&d_ent, E + ST_G)); HIPCHK(mem.get(&d_heavy, (size_t)1 + HEAVY_CAP + ST_G));
    HIPCHK(mem.get(&d_dyn, msm::DYN_MULTI + ST_G)); HIPCHK(mem.get(&d_bad, 1 + ST_G));
    if (bases) { HIPCHK(mem.get(&d_bases, n * C::AFF_STRIDE)); HIPCHK(hipMemcpyAsync(d_bases, bases, n * C::AFF_STRIDE * 4, hipMemcpyHostToDevice, s)); }
    HIPCHK(hipMemcpyAsync(d_sc, scalars, n * 32, hipMemcpyHostToDevice, s));
    HIPCHK(st_fill(s, d_off, (size_t)NB + 1 + ST_G)); HIPCHK(st_fill(s, d_cur, (size_t)NB + ST_G)); HIPCHK(st_fill(s, d_ent, E + ST_G));
    HIPCHK(st_fill(s, d_heavy, (size_t)1 + HEAVY_CAP + ST_G)); HIPCHK(st_fill(s, d_dyn, msm::DYN_MULTI + ST_G)); HIPCHK(st_fill(s, d_bad, 1 + ST_G));
    HIPCHK(hipMemsetAsync(d_heavy, 0, 4, s)); HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));          // the two words the drivers clear before every sort
    // the launches of msm_device_ranges' sweep route, in its order
    const uint32_t heavy_thr = 0xffffffffu;
    launch_digit_codes(s, g.wide, d_sc, d_bases, C::AFF_STRIDE, C::FLAGW, n, g.n_pad, c, W, d_dig, d_bad);
    launch_sort_sweep(s, g.wide, false, g.sort_grid, g.lds_bytes, d_dig, n, g.n_pad, W, g.RANGES, g.rb_log, g.B, d_cnt, nullptr, nullptr, heavy_thr, d_heavy, HEAVY_CAP);
    launch_scan(s, d_cnt, d_off, d_cur, d_bs, (size_t)NB);
    launch_dyn_chunk(s, d_off + NB, fixed_ch, a.min_chunk, a.max_chunks, a.lanes_per_chunk, (uint32_t)a.T, d_dyn);
    launch_flag_heavy(s, d_off, NB, d_dyn, d_heavy, HEAVY_CAP);
    launch_sort_sweep(s, g.wide, true, g.sort_grid, g.lds_bytes, d_dig, n, g.n_pad, W, g.RANGES, g.rb_log, g.B, nullptr, d_off, d_ent, heavy_thr, d_heavy, HEAVY_CAP);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(off, d_off, ((size_t)NB + 1 + ST_G) * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(cursor, d_cur, ((size_t)NB + ST_G) * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(entries, d_ent, (E + ST_G) * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(heavy, d_heavy, ((size_t)1 + HEAVY_CAP + ST_G) * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dyn, d_dyn, (msm::DYN_MULTI + ST_G) * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(bad, d_bad, (1 + ST_G) * 4, hipMemcpyDeviceToHost));
    return DGPU_OK;
}
extern "C" int32_t dgpu_selftest_sort_sweep(const uint32_t *scalars, size_t n, int32_t c, int32_t g2, const uint32_t *bases, uint32_t fixed_ch, uint32_t heavy_cap,
                                 uint32_t *off, uint32_t *cursor, uint32_t *entries, uint32_t *heavy, uint32_t *dyn, uint32_t *bad) {
    if (!scalars || !off || !cursor || !entries || !heavy || !dyn || !bad || c < 7 || c > 22 || n < 1 || n > ((size_t)1 << 20) || heavy_cap > (1u << 20)) return DGPU_E_BADARG;
    if (fixed_ch > 4096) return DGPU_E_BADARG;
    return g2 ? st_sort_sweep<msm::G2>(scalars, n, c, bases, fixed_ch, heavy_cap, off, cursor, entries, heavy, dyn, bad)
              : st_sort_sweep<msm::G1>(scalars, n, c, bases, fixed_ch, heavy_cap, off, cursor, entries, heavy, dyn, bad);
}
