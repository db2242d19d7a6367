// crypto_amd/csrc/dock_serde_dev.hip — point decoding and validation on the device (include/dock_gpu.h: dgpu_g*_deserialize_device,
// dgpu_bases_upload_g*_serialized, dgpu_g*_validate_batch).  The kernels are serde_kernels.hip.h (k_serde.hip); this unit stages the bytes and
// collects the verdicts.  Same verdicts and words as the host forms in dock_serde.cpp, which stay as they are.
#include "msm_driver.hip.h"
#include "serde_launch.hip.h"
using namespace dock;

namespace dock {
namespace {
constexpr uint32_t NONE_BAD = 0xffffffffu;

// The encoded points cross PCIe in pieces on the slot's copy stream; piece k's decoding runs on the compute stream once it has landed, under the
// copy of piece k + 1 (the pattern of stage_bases).  Accepted points: ABI words in sl.prepped, flags in sl.in_inf; *sl.flags = lowest refused index
// or NONE_BAD.  Nothing is waited for here.
template <class C>
int32_t decode_queue(Slot &sl, const uint8_t *in, size_t n, int32_t mode) {
    const bool comp = (mode & 1) != 0, validate = !(mode & DGPU_SERDE_NO_VALIDATE);
    const size_t sz = (comp ? 48 : 96) * (size_t)C::NFP, wb = (size_t)2 * C::ABI_W * 4;
    int32_t rc;
    if ((rc = sl.in_bases.ensure(n * sz + 16)) || (rc = sl.prepped.ensure(n * wb + 16)) || (rc = sl.in_inf.ensure(n + 16)) || (rc = sl.flags.ensure(16))) return rc;
    uint8_t *draw = sl.in_bases.as<uint8_t>();
    HIPCHK(hipMemsetAsync(sl.flags.p, 0xff, 4, sl.stream));
    const size_t per = std::max<size_t>(1, STAGE_CHUNK_BYTES / sz);
    const size_t pieces = std::min<size_t>((n + per - 1) / per, 6), len = (n + pieces - 1) / pieces;
    StageTimer st(sl, "serde.decode");
    for (size_t lo = 0; lo < n; lo += len) {
        const size_t hi = std::min(n, lo + len);
        hipEvent_t ev = sl.copy_ev[sl.ev_next++ % (Slot::N_COPY_EV + 1)];
        HIPCHK(hipMemcpyAsync(draw + lo * sz, in + lo * sz, (hi - lo) * sz, hipMemcpyHostToDevice, sl.cstream));
        HIPCHK(hipEventRecord(ev, sl.cstream));
        HIPCHK(hipStreamWaitEvent(sl.stream, ev, 0));
        serde::launch_deserialize(sl.stream, C::NFP, comp, validate, (const uint32_t *)draw, lo, hi, sl.prepped.as<uint32_t>(), sl.in_inf.as<uint8_t>(), sl.flags.as<uint32_t>());
    }
    HIPCHK(hipGetLastError());
    return DGPU_OK;
}
// both streams drained (nothing of ours may still read the caller's buffers); the first error wins
inline int32_t drain(Slot &sl, int32_t rc) {
    if (hipStreamSynchronize(sl.cstream) != hipSuccess || hipStreamSynchronize(sl.stream) != hipSuccess) { (void)hipGetLastError(); if (!rc) rc = DGPU_E_HIP; }
    if (gs.prof) prof_flush(sl);
    return rc;
}
// the verdict and (when asked for) the decoded words back to the host
template <class C>
int32_t decode_collect(Slot &sl, size_t n, uint64_t *xy, uint8_t *is_inf, uint32_t &bad) {
    HIPCHK(hipMemcpyAsync(&bad, sl.flags.p, 4, hipMemcpyDeviceToHost, sl.stream));
    if (xy) HIPCHK(hipMemcpyAsync(xy, sl.prepped.p, n * 2 * C::ABI_W * 4, hipMemcpyDeviceToHost, sl.stream));
    if (is_inf) HIPCHK(hipMemcpyAsync(is_inf, sl.in_inf.p, n, hipMemcpyDeviceToHost, sl.stream));
    return DGPU_OK;
}

template <class C>
int32_t deserialize_device(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy, uint8_t *is_inf, size_t *first_bad) {
    if (n && (!in || !xy || !is_inf)) return DGPU_E_BADARG;
    if (n >= (1ull << 31)) return DGPU_E_BADARG;
    if (n == 0) { if (first_bad) *first_bad = 0; return DGPU_OK; }
    if (!cur().ready) return DGPU_E_NODEVICE;
    uint32_t bad = NONE_BAD;
    int32_t rc;
    {
        SLOT_ACQUIRE(L, sl);
        HIPCHK(hipSetDevice(cur().device));
        rc = decode_queue<C>(sl, in, n, mode);
        if (!rc) rc = decode_collect<C>(sl, n, xy, is_inf, bad);
        rc = drain(sl, rc);
    }
    if (rc) return rc;
    if (first_bad) *first_bad = bad == NONE_BAD ? n : bad;
    return bad == NONE_BAD ? DGPU_OK : DGPU_E_BADARG;
}

// bytes -> a plain resident handle: the decoded words go through the conversion bases_upload uses (k_prep_bases) straight from the workspace.
// The handle's memory is taken only once every point is accepted, so a refused key leaves nothing behind.
template <class C>
int32_t upload_serialized(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy, uint8_t *is_inf, uint64_t *handle, size_t *first_bad, int kind) {
    if (!handle || (n && !in) || n >= (1ull << 31)) return DGPU_E_BADARG;
    if (n == 0) {
        const int32_t rc = bases_upload<C>(RawBases::packed<C>(nullptr, nullptr), 0, handle, kind);
        if (!rc && first_bad) *first_bad = 0;
        return rc;
    }
    if (!cur().ready) return DGPU_E_NODEVICE;
    uint32_t bad = NONE_BAD;
    void *p = nullptr;
    int32_t rc;
    {
        SLOT_ACQUIRE(L, sl);
        HIPCHK(hipSetDevice(cur().device));
        rc = decode_queue<C>(sl, in, n, mode);
        if (!rc) rc = decode_collect<C>(sl, n, xy, is_inf, bad);
        rc = drain(sl, rc);
        if (!rc && bad == NONE_BAD) {
            if (dev_malloc(&p, n * C::AFF_STRIDE * 4) != hipSuccess) { (void)hipGetLastError(); p = nullptr; rc = DGPU_E_OOM; }
            if (!rc) {
                launch_prep_bases<C>(sl.stream, sl.prepped.as<uint32_t>(), sl.in_inf.as<uint8_t>(), n, (uint32_t *)p);
                if (hipGetLastError() != hipSuccess) rc = DGPU_E_HIP;
                rc = drain(sl, rc);
            }
            if (rc && p) { (void)hipFree(p); p = nullptr; }
        }
    }
    if (rc) return rc;
    if (first_bad) *first_bad = bad == NONE_BAD ? n : bad;
    if (bad != NONE_BAD) return DGPU_E_BADARG;
    bases_register<C>(p, n, handle, kind);
    return DGPU_OK;
}

template <class C>
int32_t validate_batch(const uint64_t *xy, const uint8_t *is_inf, size_t n, uint8_t *ok) {
    if (n && (!xy || !ok)) return DGPU_E_BADARG;
    if (n >= (1ull << 31)) return DGPU_E_BADARG;
    if (n == 0) return DGPU_OK;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t wb = (size_t)2 * C::ABI_W * 4;
    int32_t rc;
    if ((rc = sl.prepped.ensure(n * wb + 16)) || (rc = sl.in_inf.ensure(n + 16)) || (rc = sl.digits.ensure(n + 16))) return rc;
    const uint8_t *dinf = nullptr;
    if (is_inf) { HIPCHK(hipMemcpyAsync(sl.in_inf.p, is_inf, n, hipMemcpyHostToDevice, sl.cstream)); dinf = sl.in_inf.as<uint8_t>(); }
    const size_t per = std::max<size_t>(1, STAGE_CHUNK_BYTES / wb);
    const size_t pieces = std::min<size_t>((n + per - 1) / per, 6), len = (n + pieces - 1) / pieces;
    {
        StageTimer st(sl, "serde.validate");
        for (size_t lo = 0; lo < n && !rc; lo += len) {
            const size_t hi = std::min(n, lo + len);
            hipEvent_t ev = sl.copy_ev[sl.ev_next++ % (Slot::N_COPY_EV + 1)];
            if (hipMemcpyAsync(sl.prepped.as<uint8_t>() + lo * wb, (const uint8_t *)xy + lo * wb, (hi - lo) * wb, hipMemcpyHostToDevice, sl.cstream) != hipSuccess ||
                hipEventRecord(ev, sl.cstream) != hipSuccess || hipStreamWaitEvent(sl.stream, ev, 0) != hipSuccess) { rc = DGPU_E_HIP; break; }
            serde::launch_validate_words(sl.stream, C::NFP, sl.prepped.as<uint32_t>(), dinf, lo, hi, sl.digits.as<uint8_t>());
        }
    }
    if (!rc && (hipGetLastError() != hipSuccess || hipMemcpyAsync(ok, sl.digits.p, n, hipMemcpyDeviceToHost, sl.stream) != hipSuccess)) rc = DGPU_E_HIP;
    return drain(sl, rc);
}
}  // namespace
}  // namespace dock

extern "C" {
int32_t dgpu_g1_deserialize_device(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy, uint8_t *is_inf, size_t *first_bad) { return deserialize_device<G1>(in, n, mode, xy, is_inf, first_bad); }
int32_t dgpu_g2_deserialize_device(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy, uint8_t *is_inf, size_t *first_bad) { return deserialize_device<G2>(in, n, mode, xy, is_inf, first_bad); }
int32_t dgpu_bases_upload_g1_serialized(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy, uint8_t *is_inf, uint64_t *handle, size_t *first_bad) {
    return upload_serialized<G1>(in, n, mode, xy, is_inf, handle, first_bad, 1); }
int32_t dgpu_bases_upload_g2_serialized(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy, uint8_t *is_inf, uint64_t *handle, size_t *first_bad) {
    return upload_serialized<G2>(in, n, mode, xy, is_inf, handle, first_bad, 2); }
int32_t dgpu_g1_validate_batch(const uint64_t *xy, const uint8_t *is_inf, size_t n, uint8_t *ok) { return validate_batch<G1>(xy, is_inf, n, ok); }
int32_t dgpu_g2_validate_batch(const uint64_t *xy, const uint8_t *is_inf, size_t n, uint8_t *ok) { return validate_batch<G2>(xy, is_inf, n, ok); }
}  // extern "C"
