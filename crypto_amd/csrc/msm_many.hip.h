// crypto_amd/csrc/msm_many.hip.h — many small MSMs in one call (templated on the curve): rows of scalars over one plain handle, segments over their own bases.
#pragma once
#include <thread>
#include <type_traits>
#include "msm_driver.hip.h"

namespace dock {

// ---- many rows of scalars over one plain handle in one call (many_kernels.hip.h) -----------------------------------------------------------
// rows per launch: 2^17 terms' worth, at most 4096 rows — the scalars, 16 window sums per row and (rows of more than 128 terms) up to 64 partials per
// window stay below ~70 MB of the slot's grow-only buffers whatever m; dgpu_set_many_chunk_rows (development surface) overrides it
inline size_t many_chunk_rows(size_t n) {
    const int forced = gs.many_chunk.load();
    if (forced > 0) return (size_t)forced;
    const size_t r = ((size_t)1 << 17) / std::max<size_t>(n, 1);
    return std::min<size_t>(4096, std::max<size_t>(r, 1));
}
template <class C> int32_t ws_many(Slot &sl, size_t n, size_t rows, const ManyGeom &g) {
    int32_t rc;
    typedef typename C::ACC A;
    constexpr size_t WPS = SMALL_MSM_W / SMALL_MSM_S;
    if ((rc = sl.flags.ensure(64))) return rc;
    if ((rc = sl.in_scalars.ensure(rows * n * 32))) return rc;
    if ((rc = sl.bucket.ensure(rows * WPS * A::XW * 4))) return rc;                      // the window sums and their flags
    if ((rc = sl.bucket_inf.ensure(rows * WPS))) return rc;
    if (g.nblk > 1) {
        if ((rc = sl.head.ensure(rows * WPS * g.nblk * A::XW * 4))) return rc;          // the blocks' partials, their flags, the per-window block counters
        if ((rc = sl.part_inf.ensure(rows * WPS * g.nblk))) return rc;
        if ((rc = sl.cnt.ensure(rows * WPS * 4))) return rc;
    }
    if ((rc = sl.win.ensure(rows * 3 * C::ABI_W * 4))) return rc;                        // the rows' results and their identity flags
    return sl.win_inf.ensure(rows);
}
// one chunk whose canonical scalars are on the device already (rows packed; the workspace is ws_many's): tree, fold.  The rows' normalised Jacobian results
// are left in sl.win, their identity flags in sl.win_inf, *d_bad |= a scalar >= 2^255.  Shared by msm_device_many and RowMsm below,
// whose rows are made on the device.
template <class C>
int32_t many_rows_resident(Slot &sl, const SmallSub &sub, const uint32_t *d_sc, size_t n, size_t rows, const ManyGeom &g, uint32_t *d_bad) {
    hipStream_t s = sl.stream;
    if (g.nblk > 1) HIPCHK(hipMemsetAsync(sl.cnt.p, 0, rows * (SMALL_MSM_W / SMALL_MSM_S) * 4, s));
    {
        StageTimer st(sl, "msm.many_tree");
        launch_many_tree<C>(s, sub.tab, sub.tab_inf, d_sc, n, n, rows, sl.head.as<uint32_t>(), sl.part_inf.as<uint8_t>(), sl.cnt.as<uint32_t>(), sl.bucket.as<uint32_t>(), sl.bucket_inf.as<uint8_t>(), d_bad);
    }
    {
        StageTimer st(sl, "msm.many_fold");
        launch_many_fold<C>(s, sl.bucket.as<uint32_t>(), sl.bucket_inf.as<uint8_t>(), rows, sl.win.as<uint32_t>(), sl.win_inf.as<uint8_t>());
    }
    HIPCHK(hipGetLastError());
    return DGPU_OK;
}
// `rows` rows of L scalars, `stride` scalars apart in the caller's memory, packed on the device: what lies between the caller's rows never crosses
inline int32_t upload_rows_packed(hipStream_t s, void *dst, const uint64_t *src, size_t L, size_t stride, size_t rows) {
    if (stride == L) HIPCHK(hipMemcpyAsync(dst, src, rows * L * 32, hipMemcpyHostToDevice, s));
    else HIPCHK(hipMemcpy2DAsync(dst, L * 32, src, stride * 32, L * 32, rows, hipMemcpyHostToDevice, s));
    return DGPU_OK;
}
// the rows on the device, chunk by chunk: scalars up, tree, fold, results down
template <class C>
int32_t msm_device_many(Slot &sl, const SmallSub &sub, const uint64_t *scalars, size_t row_stride, size_t n, size_t m, bool mont, uint64_t *out, uint8_t *out_inf) {
    int32_t rc;
    constexpr size_t JW = 3 * C::ABI_W / 2;                                               // u64 words per result
    const ManyGeom g = many_geometry(n);
    const size_t chunk = std::min(m, many_chunk_rows(n));
    if ((rc = ensure_workspace(sl, [&](Slot &o) { return ws_many<C>(o, n, chunk, g); }))) return rc;
    hipStream_t s = sl.stream;
    uint32_t *const d_sc = sl.in_scalars.as<uint32_t>(), *const d_bad = sl.flags.as<uint32_t>();
    HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));
    uint32_t *const hbad = (uint32_t *)sl.hpin;
    for (size_t r0 = 0; r0 < m; r0 += chunk) {
        const size_t rows = std::min(chunk, m - r0);
        hipEvent_t ev = sl.copy_ev[sl.ev_next++ % (Slot::N_COPY_EV + 1)];
        if ((rc = upload_rows_packed(sl.cstream, d_sc, scalars + r0 * row_stride * 4, n, row_stride, rows))) return rc;
        HIPCHK(hipEventRecord(ev, sl.cstream));
        HIPCHK(hipStreamWaitEvent(s, ev, 0));
        if (mont) ntt::launch_fr_mont_to_canonical(s, d_sc, rows * n);
        if ((rc = many_rows_resident<C>(sl, sub, d_sc, n, rows, g, d_bad))) return rc;
        HIPCHK(hipMemcpyAsync(out + r0 * JW, sl.win.p, rows * JW * 8, hipMemcpyDeviceToHost, s));
        if (out_inf) HIPCHK(hipMemcpyAsync(out_inf + r0, sl.win_inf.p, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hbad, d_bad, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                  // (the next chunk's scalars overwrite this one's)
        if (gs.prof) prof_flush(sl);
        if (*hbad) return DGPU_E_BADARG;                  // a scalar >= 2^255 somewhere in the block: the whole call is refused
    }
    return DGPU_OK;
}
// Jacobian rows (X, Y, Z: 3 F) -> affine rows (x, y: 2 F) packed in place (2 i + 2 <= 3 i), an identity: zero words, and inf[i] its flag.  F: hostf::Fq (G1:
// 18 -> 12 words) or hostf::Fq2 (G2: 36 -> 24)
template <class F> inline void jac_rows_to_affine(uint64_t *jac, size_t rows, uint8_t *inf) {
    constexpr size_t FW = sizeof(F) / 8;
    for (size_t i = 0; i < rows; i++) {
        const uint64_t *p = jac + 3 * FW * i;
        uint64_t *q = jac + 2 * FW * i;
        inf[i] = jac_is_identity(p, 3 * FW);
        if (inf[i]) { memset(q, 0, 2 * sizeof(F)); continue; }
        F x, y, z; memcpy(&x, p, sizeof(F)); memcpy(&y, p + FW, sizeof(F)); memcpy(&z, p + 2 * FW, sizeof(F));
        const F zi = z.inv(), zi2 = zi * zi;
        x = x * zi2; y = y * zi2 * zi;
        memcpy(q, &x, sizeof(F)); memcpy(q + FW, &y, sizeof(F));
    }
}
// Rows of n scalars made on the device, over one small set of G1 or G2 bases -> affine points and identity flags on the device (dock_bbs.hip: the b_i and P_i over
// the parameters; dock_accumulator.hip: the T_i over omega; dock_ps.hip: the Q_i, S_i, R_i over the public key in G2).  The many-row kernels over the bases' small-path table `sub` where they reach; beyond (rows longer than
// dgpu_set_small_msm_max allows, no memory for the table) the single-row driver over the prepared records `rec`, row by row, normalised on the host.  The caller
// says which, and fills in `sub` or `rec` before points(): a handle's table comes from small_sub_for, a call's own table is built in its workspace.
template <class C> struct RowMsm {
    typedef typename std::conditional<C::NFP == 1, hostf::Fq, hostf::Fq2>::type HF;      // the slow path normalises over the curve's base field
    static constexpr size_t PT = 2 * C::ABI_W * 4;        // bytes of an affine point of the ABI
    bool many; ManyGeom geom; size_t n, chunk;            // terms per row, rows per chunk
    SmallSub sub{nullptr, nullptr}; const uint32_t *rec = nullptr;
    // rows per chunk: the caller's cap, a launch of the many-row kernels, or 64 MB of scalars on the slow path (n = 0: no row is ever run)
    RowMsm(bool many_, size_t n_, size_t rows, size_t cap)
        : many(many_), geom(many_geometry(std::max<size_t>(n_, 1))), n(n_),
          chunk(std::min(rows, std::min(cap, many_ ? many_chunk_rows(n_) : std::max<size_t>(1, ((size_t)1 << 21) / std::max<size_t>(n_, 1))))) {}
    int32_t workspace(Slot &o) const {
        if (many) return ws_many<C>(o, n, chunk, geom);
        int32_t e;
        if ((e = ws_for<C>(o, 2, n, 0, nullptr))) return e;
        if ((e = o.in_scalars.ensure(chunk * n * 32))) return e;
        return o.flags.ensure(64);
    }
    // the rows at d_rows (canonical words, packed) -> dOut (affine words; an identity: zero words) and dInf
    int32_t points(Slot &sl, const uint32_t *d_rows, size_t rows, uint32_t *d_bad, uint8_t *dOut, uint8_t *dInf) const {
        hipStream_t s = sl.stream;
        int32_t rc;
        if (many) {
            if ((rc = many_rows_resident<C>(sl, sub, d_rows, n, rows, geom, d_bad))) return rc;
            // the normalised Jacobian rows (X, Y, 1) -> X and Y of every row, and its identity flag
            HIPCHK(hipMemcpy2DAsync(dOut, PT, sl.win.p, 3 * PT / 2, PT, rows, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(dInf, sl.win_inf.p, rows, hipMemcpyDeviceToDevice, s));
            return DGPU_OK;
        }
        HIPCHK(hipGetLastError());
        constexpr size_t JW = 3 * sizeof(HF) / 8;
        std::vector<uint64_t> jac(rows * JW); std::vector<uint8_t> inf(rows);
        for (size_t i = 0; i < rows; i++)
            if ((rc = msm_device<C, HF>(sl, rec, d_rows + i * n * 8, n, jac.data() + JW * i))) return rc;
        jac_rows_to_affine<HF>(jac.data(), rows, inf.data());
        hipError_t up = hipMemcpyAsync(dOut, jac.data(), rows * PT, hipMemcpyHostToDevice, s);
        if (up == hipSuccess) up = hipMemcpyAsync(dInf, inf.data(), rows, hipMemcpyHostToDevice, s);
        const hipError_t waited = hipStreamSynchronize(s);      // (the host vectors end here, whatever the copies answered)
        HIPCHK(up); HIPCHK(waited);
        return DGPU_OK;
    }
};
// How the rows over a plain bases handle `h` (pinned by the caller) are made: RowMsm over its first nn points, whose small-path table serves the many-row kernels
// where they reach (dock_bbs.hip: the signature parameters in G1; dock_ps.hip: the public key in G2).  group: MSM rows that belong together (dock_ps.hip: the
// two rows of a proof) — the chunk is a whole number of groups and at least one, so a forced chunk that is no multiple of it is rounded down, and up to one group
template <class C> RowMsm<C> param_rows(Slot &sl, uint64_t params, const Handle &h, size_t nn, size_t cap, size_t n, size_t group = 1) {
    SmallSub sub{nullptr, nullptr};
    const bool many = h.n <= SMALL_MSM_MAX_N && nn <= gs.small_max.load() && small_sub_for<C>(sl, params, h, 0, nn, sub, true);
    RowMsm<C> rm(many, nn, n, cap);
    rm.sub = sub; rm.rec = (const uint32_t *)h.p;
    rm.chunk = std::max(group, rm.chunk - rm.chunk % group);
    return rm;
}
template <class C, class HF>
int32_t msm_handle_many(uint64_t bases, size_t offset, const uint64_t *scalars, size_t row_stride, size_t n, size_t m, int mont, uint64_t *out, uint8_t *out_inf, int kind) {
    if (m == 0) return DGPU_OK;
    constexpr size_t JW = 3 * sizeof(HF) / 8;
    if (!out || (n && (!scalars || row_stride < n)) || m >= (1ull << 31) || n >= (1ull << 31) || row_stride >= (1ull << 31)) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;             // (before the size threshold, like the single call)
    if (!tl_no_min && m * n < std::min<size_t>(gs.min_gpu_n, DGPU_MIN_GPU_N_HANDLE)) return DGPU_E_TOO_SMALL;      // the batch is the unit: many one-term rows are device work
    bool served = false;
    int32_t rc = DGPU_OK;
    {
        HandleRef hb(bases);
        if (!hb.ok || (hb.h.kind != kind && hb.h.kind != kind + 9) || offset > hb.h.n || n > hb.h.n - offset) return DGPU_E_BADARG;
        if (n == 0) {                                     // every row is the empty sum
            for (size_t j = 0; j < m; j++) { write_identity<HF>(out + j * JW); if (out_inf) out_inf[j] = 1; }
            return DGPU_OK;
        }
        // the new kernels serve plain handles within the small path's reach; anything else (a precomputed table, more than 8192 bases, the small path switched
        // off, no memory for the table) runs its rows through the single-row driver below
        if (hb.h.kind == kind && hb.h.n <= SMALL_MSM_MAX_N && n <= gs.small_max.load()) {
            CtxScope on_owner(hb.h.ctx);
            SLOT_ACQUIRE(L, sl);
            HIPCHK(hipSetDevice(cur().device));
            SmallSub sub;
            if (small_sub_for<C>(sl, bases, hb.h, offset, n, sub, true)) {
                served = true;
                rc = msm_device_many<C>(sl, sub, scalars, row_stride, n, m, mont != 0, out, out_inf);
                if (rc) drain(sl);
            }
        }
    }
    if (served) return rc;
    for (size_t j = 0; j < m; j++) {
        if ((rc = msm_handle<C, HF>(bases, offset, scalars + 4 * row_stride * j, n, mont, out + j * JW, kind, false))) return rc;
        if (out_inf) out_inf[j] = jac_is_identity(out + j * JW, JW);
    }
    return DGPU_OK;
}

// ---- many small MSMs, each over its own bases, in one call (seg_kernels.hip.h) ----------------------------------------------------------------
// Segments travel in chunks of whole segments: at most SEG_CHUNK_TERMS terms (the table of eight multiples per base is 1.6 KB per G1 base, 3.3 KB per G2
// base: 109 / 218 MB) and SEG_CHUNK_SEGS segments (64 window sums each: 55 / 109 MB) per chunk; dgpu_set_msm_segments (development surface) overrides the
// term limit.  From SEG_DEVICE_FOLD_MIN segments in a chunk on, k_seg_fold folds them on the device; below, the host threads' host_fold does (up to 16 threads per
// chunk through par_run: several calls in flight with few segments each share the host's cores).
constexpr size_t SEG_CHUNK_TERMS = (size_t)1 << 16, SEG_CHUNK_SEGS = 4096;
constexpr size_t SEG_DEVICE_FOLD_MIN = 24;              // PROVISIONAL, not measured: the crossover is what tests/perf/msm_segments_timing.py's fold sweep finds on an MI355X
// what every chunk needs whatever brings its operands: the prepared records, the table of eight multiples per base and its identity flags, the descriptors, the
// window sums and the results with their flags
template <class C> int32_t ws_seg_resident(Slot &sl, size_t terms, size_t nseg, size_t blocks) {
    int32_t rc;
    typedef typename C::ACC A;
    constexpr size_t W = SMALL_MSM_W, WIN_BYTES = std::max<size_t>(A::XW * 4, 4 * C::ABI_W * 4);      // a window sum in either form
    if ((rc = sl.flags.ensure(64))) return rc;
    if ((rc = sl.prepped.ensure(terms * C::AFF_STRIDE * 4))) return rc;
    if ((rc = sl.bucket.ensure(terms * SMALL_MSM_E * A::XW * 4))) return rc;
    if ((rc = sl.bucket_inf.ensure(terms * SMALL_MSM_E))) return rc;
    if ((rc = sl.entries.ensure(blocks * 64 * sizeof(SegDesc)))) return rc;
    if ((rc = sl.l1.ensure(nseg * W * WIN_BYTES))) return rc;
    if ((rc = sl.l1_inf.ensure(nseg * W))) return rc;
    if ((rc = sl.win.ensure(nseg * 3 * C::ABI_W * 4))) return rc;
    return sl.win_inf.ensure(nseg);
}
// ... and what a chunk from the host adds: its scalars, its staged bases, and the partial slots of segments longer than a block
template <class C> int32_t ws_seg(Slot &sl, const RawBases &rb, size_t terms, size_t nseg, size_t blocks, size_t pslots) {
    int32_t rc;
    constexpr size_t W = SMALL_MSM_W;
    if ((rc = ws_seg_resident<C>(sl, terms, nseg, blocks))) return rc;
    if ((rc = sl.in_scalars.ensure(terms * 32))) return rc;
    if ((rc = ws_stage_bases<C>(sl, rb, terms))) return rc;
    if (pslots) {
        if ((rc = sl.head.ensure(pslots * W * C::ACC::XW * 4))) return rc;                  // the blocks' partials, their flags, the per-window block counters
        if ((rc = sl.part_inf.ensure(pslots * W))) return rc;
        if ((rc = sl.cnt.ensure(pslots * W * 4))) return rc;
    }
    return DGPU_OK;
}
// the launches of a chunk of T terms in ns segments whose prepared records are in sl.prepped and whose descriptors are on their way to sl.entries: table, tree,
// and (device_fold) the fold that leaves the normalised Jacobian results in sl.win and their identity flags in sl.win_inf; *d_bad |= a scalar >= 2^255
template <class C>
int32_t seg_launches(Slot &sl, const uint32_t *d_sc, size_t T, size_t ns, const SegLayout &lay, bool device_fold, uint32_t *d_bad) {
    hipStream_t s = sl.stream;
    {
        StageTimer st(sl, "msm.small_table");
        launch_small_table<C>(s, sl.prepped.as<uint32_t>(), T, sl.bucket.as<uint32_t>(), sl.bucket_inf.as<uint8_t>());
    }
    if (lay.pslots) HIPCHK(hipMemsetAsync(sl.cnt.p, 0, lay.pslots * SMALL_MSM_W * 4, s));
    {
        StageTimer st(sl, "msm.seg_tree");
        launch_seg_tree<C>(s, sl.bucket.as<uint32_t>(), sl.bucket_inf.as<uint8_t>(), d_sc, sl.entries.p, lay.blocks, sl.head.as<uint32_t>(), sl.part_inf.as<uint8_t>(), sl.cnt.as<uint32_t>(),
                           sl.l1.as<uint32_t>(), sl.l1_inf.as<uint8_t>(), !device_fold, d_bad);
    }
    if (device_fold) {
        StageTimer st(sl, "msm.seg_fold");
        launch_seg_fold<C>(s, sl.l1.as<uint32_t>(), sl.l1_inf.as<uint8_t>(), ns, sl.win.as<uint32_t>(), sl.win_inf.as<uint8_t>());
    }
    HIPCHK(hipGetLastError());
    return DGPU_OK;
}
// segments [s0, s1) (all within the small path's reach, T > 0 terms in all) on the device: one upload, table, tree, fold (device or host), results down
template <class C, class HF>
int32_t msm_seg_chunk(Slot &sl, const RawBases &rb, const uint64_t *scalars, const uint64_t *seg_end, size_t s0, size_t s1, bool mont, const SegLayout &lay, bool device_fold,
                      std::vector<uint64_t> &hwin, std::vector<uint8_t> &hinf, uint64_t *out, uint8_t *out_inf) {
    constexpr size_t JW = 3 * sizeof(HF) / 8, W = SMALL_MSM_W, WW = 4 * sizeof(HF) / 8;   // u64 words per result / per window sum
    const size_t t0 = s0 ? seg_end[s0 - 1] : 0, T = seg_end[s1 - 1] - t0, ns = s1 - s0;
    hipStream_t s = sl.stream;
    uint32_t *const d_sc = sl.in_scalars.as<uint32_t>(), *const d_bad = sl.flags.as<uint32_t>();
    uint32_t *const hbad = (uint32_t *)sl.hpin;
    int32_t rc;
    HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));
    HIPCHK(hipMemcpyAsync(sl.entries.p, lay.desc.data(), lay.blocks * 64 * sizeof(SegDesc), hipMemcpyHostToDevice, sl.cstream));      // (ordered before the scalars' event)
    if ((rc = stage_scalars(sl, scalars + t0 * 4, T, mont, d_sc))) return rc;
    if ((rc = stage_bases<C>(sl, rb.from(t0), T, sl.prepped.as<uint32_t>()))) return rc;
    if ((rc = seg_launches<C>(sl, d_sc, T, ns, lay, device_fold, d_bad))) return rc;
    if (device_fold) {
        HIPCHK(hipMemcpyAsync(out + s0 * JW, sl.win.p, ns * JW * 8, hipMemcpyDeviceToHost, s));
        if (out_inf) HIPCHK(hipMemcpyAsync(out_inf + s0, sl.win_inf.p, ns, hipMemcpyDeviceToHost, s));
    } else {
        hwin.resize(ns * W * WW); hinf.resize(ns * W);
        HIPCHK(hipMemcpyAsync(hwin.data(), sl.l1.p, ns * W * WW * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hinf.data(), sl.l1_inf.p, ns * W, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(hbad, d_bad, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                      // (the next chunk's operands overwrite this one's)
    if (gs.prof) prof_flush(sl);
    if (*hbad) return DGPU_E_BADARG;                      // a scalar >= 2^255 somewhere in the chunk: the whole call is refused
    if (!device_fold) {
        const size_t TH = std::min<size_t>(std::min<size_t>(ns, 16), std::max<size_t>(1, std::thread::hardware_concurrency()));
        auto tail = [&](size_t g) {
            host_fold<HF>(hwin.data() + g * W * WW, hinf.data() + g * W, (int)W, SMALL_MSM_C, out + (s0 + g) * JW);
            if (out_inf) out_inf[s0 + g] = jac_is_identity(out + (s0 + g) * JW, JW);
        };
        if (TH <= 1) { for (size_t g = 0; g < ns; g++) tail(g); }
        else if ((rc = par_run(TH, [&](size_t k) -> int32_t { for (size_t g = k; g < ns; g += TH) tail(g); return DGPU_OK; }))) return rc;
    }
    return DGPU_OK;
}
// The device-resident entry of a chunk (dock_bbs.hip: proofs of knowledge, whose segments' scalars are made on the device): T raw points on the device (`stride`
// bytes apart, x then y, zero words an identity) and their canonical scalars d_sc, laid out over ns segments by `lay` (no multi-block segment: lay.pslots == 0).
// Table, tree, device fold (seg_launches); the workspace is ws_seg_resident's.
template <class C>
int32_t seg_rows_resident(Slot &sl, const uint8_t *d_raw, size_t stride, const uint32_t *d_sc, size_t T, size_t ns, const SegLayout &lay, uint32_t *d_bad) {
    hipStream_t s = sl.stream;
    if (lay.pslots) return DGPU_E_BADARG;
    HIPCHK(hipMemcpyAsync(sl.entries.p, lay.desc.data(), lay.blocks * 64 * sizeof(SegDesc), hipMemcpyHostToDevice, s));
    {
        StageTimer st(sl, "msm.prep_bases");
        launch_prep_bases_raw<C>(s, d_raw, stride, 0, (size_t)C::ABI_W * 4, msm::NO_INF_OFF, nullptr, T, sl.prepped.as<uint32_t>());
    }
    return seg_launches<C>(sl, d_sc, T, ns, lay, true, d_bad);
}
template <class C, class HF>
int32_t msm_segments(const uint64_t *bases, const uint8_t *is_inf, const uint64_t *scalars, size_t N, const uint64_t *seg_end, size_t nseg, int mont, uint64_t *out, uint8_t *out_inf) {
    if (nseg == 0) return DGPU_OK;
    constexpr size_t JW = 3 * sizeof(HF) / 8;
    if (!bases || !scalars || !out || !seg_end || N >= (1ull << 31)) return DGPU_E_BADARG;
    { uint64_t prev = 0; for (size_t g = 0; g < nseg; g++) { if (seg_end[g] < prev) return DGPU_E_BADARG; prev = seg_end[g]; } if (prev != N) return DGPU_E_BADARG; }
    if (!cur().ready) return DGPU_E_NODEVICE;             // (before the size threshold, like the single call)
    if (!tl_no_min && N < gs.min_gpu_n) return DGPU_E_TOO_SMALL;      // the batch is the unit: many one-term segments are device work
    const RawBases rb = RawBases::packed<C>(bases, is_inf);
    const size_t reach = std::min<size_t>(SMALL_MSM_MAX_N, gs.small_max.load());
    const int forced_terms = gs.seg_chunk.load(), forced_fold = gs.seg_fold.load();
    const size_t chunk_terms = forced_terms > 0 ? (size_t)forced_terms : SEG_CHUNK_TERMS;
    auto len = [&](size_t g) { return (size_t)(seg_end[g] - (g ? seg_end[g - 1] : 0)); };
    // the chunks: runs of whole segments within the small path's reach; a longer segment ends the run and goes through the single-call driver afterwards
    struct Chunk { size_t s0, s1; };
    std::vector<Chunk> chunks; std::vector<size_t> slow;
    for (size_t g = 0; g < nseg;) {
        if (len(g) > reach) { slow.push_back(g++); continue; }
        size_t e = g, terms = 0;
        while (e < nseg && len(e) <= reach && e - g < SEG_CHUNK_SEGS && (e == g || terms + len(e) <= chunk_terms)) terms += len(e++);
        chunks.push_back(Chunk{g, e});
        g = e;
    }
    if (!chunks.empty()) {
        SLOT_ACQUIRE(L, sl);
        HIPCHK(hipSetDevice(cur().device));
        // one pass over the layouts for the workspace (grow-only; a shape already seen allocates nothing), one more to run them
        SegLayout lay;
        size_t mt = 0, ms = 0, mb = 0, mp = 0;
        for (const Chunk &c : chunks) {
            const size_t T = seg_end[c.s1 - 1] - (c.s0 ? seg_end[c.s0 - 1] : 0);
            if (T == 0) continue;
            seg_layout(seg_end, c.s0, c.s1, lay);
            mt = std::max(mt, T); ms = std::max(ms, c.s1 - c.s0); mb = std::max(mb, lay.blocks); mp = std::max(mp, lay.pslots);
        }
        int32_t rc;
        if (mt && (rc = ensure_workspace(sl, [&](Slot &o) { return ws_seg<C>(o, rb, mt, ms, mb, mp); }))) return rc;
        std::vector<uint64_t> hwin; std::vector<uint8_t> hinf;
        for (const Chunk &c : chunks) {
            const size_t T = seg_end[c.s1 - 1] - (c.s0 ? seg_end[c.s0 - 1] : 0), ns = c.s1 - c.s0;
            if (T == 0) {                                 // nothing but empty segments
                for (size_t g = c.s0; g < c.s1; g++) { write_identity<HF>(out + g * JW); if (out_inf) out_inf[g] = 1; }
                continue;
            }
            seg_layout(seg_end, c.s0, c.s1, lay);
            const bool device_fold = forced_fold == 2 || (forced_fold != 1 && ns >= SEG_DEVICE_FOLD_MIN);
            rc = msm_seg_chunk<C, HF>(sl, rb, scalars, seg_end, c.s0, c.s1, mont != 0, lay, device_fold, hwin, hinf, out, out_inf);
            if (rc) { drain(sl); return rc; }
        }
    }
    // segments beyond the small path's reach: the single-call driver, one after the other (the slot is released: that driver takes its own)
    for (size_t g : slow) {
        const size_t lo = g ? seg_end[g - 1] : 0;
        const int32_t rc = msm_oneshot_ctx<C, HF>(rb.from(lo), scalars + lo * 4, len(g), mont != 0, out + g * JW);
        if (rc) return rc;
        if (out_inf) out_inf[g] = jac_is_identity(out + g * JW, JW);
    }
    return DGPU_OK;
}

}  // namespace dock
