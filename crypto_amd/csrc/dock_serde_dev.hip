// crypto_amd/csrc/dock_serde_dev.hip — point decoding, validation and encoding on the device (include/dock_gpu.h: dgpu_g*_deserialize_device,
// dgpu_bases_upload_g*_serialized, dgpu_g*_validate_batch, dgpu_g*_serialize_device, dgpu_bases_read_g*, dgpu_bases_serialize_g*).  The kernels are
// serde_kernels.hip.h (k_serde.hip); this unit stages the bytes and collects the verdicts.  Same verdicts, words and bytes as the host forms in
// dock_serde.cpp, which stay as they are.
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

// ---- encoding ---------------------------------------------------------------------------------------------------------------------------------
// decode_queue run backwards: piece k is encoded on the compute stream and copied to the host on the copy stream while piece k + 1 encodes.
// stage_in(lo, hi) queues a piece's inputs on the copy stream (has_in; the handle forms read resident records and have none), encode(lo, hi)
// launches on the compute stream, copy_out(lo, hi) queues the piece's results to the host on the copy stream.  bpp: bytes a point sends to the host.
// Nothing is waited for here.
template <class In, class Enc, class Out>
int32_t encode_queue(Slot &sl, size_t n, size_t bpp, bool has_in, In stage_in, Enc encode, Out copy_out) {
    const size_t per = std::max<size_t>(1, STAGE_CHUNK_BYTES / bpp);
    const size_t pieces = std::min<size_t>((n + per - 1) / per, 6), len = (n + pieces - 1) / pieces;
    auto mark = [&](hipStream_t s, hipEvent_t &ev) { ev = sl.copy_ev[sl.ev_next++ % (Slot::N_COPY_EV + 1)]; return hipEventRecord(ev, s) == hipSuccess; };
    StageTimer st(sl, "serde.encode");
    hipEvent_t landed = nullptr, done = nullptr;
    int32_t rc = DGPU_OK;
    if (has_in && (stage_in(0, std::min(n, len)) || !mark(sl.cstream, landed))) rc = DGPU_E_HIP;
    for (size_t lo = 0; lo < n && !rc; lo += len) {
        const size_t hi = std::min(n, lo + len);
        if (has_in && hipStreamWaitEvent(sl.stream, landed, 0) != hipSuccess) { rc = DGPU_E_HIP; break; }
        encode(lo, hi);
        if (has_in && hi < n && (stage_in(hi, std::min(n, hi + len)) || !mark(sl.cstream, landed))) { rc = DGPU_E_HIP; break; }     // under this piece's encoding
        if (!mark(sl.stream, done) || hipStreamWaitEvent(sl.cstream, done, 0) != hipSuccess || copy_out(lo, hi)) { rc = DGPU_E_HIP; break; }
    }
    hipEvent_t all = nullptr;                       // (the timer covers the last copy)
    if (!rc && (hipGetLastError() != hipSuccess || !mark(sl.cstream, all) || hipStreamWaitEvent(sl.stream, all, 0) != hipSuccess)) rc = DGPU_E_HIP;
    return rc;
}

template <class C>
int32_t serialize_device(const uint64_t *xy, const uint8_t *is_inf, size_t n, int32_t compressed, uint8_t *out) {
    if (n && (!xy || !out)) return DGPU_E_BADARG;
    if (n >= (1ull << 31)) return DGPU_E_BADARG;
    if (n == 0) return DGPU_OK;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    const bool comp = compressed != 0;
    const size_t wb = (size_t)2 * C::ABI_W * 4, sz = (comp ? 48 : 96) * (size_t)C::NFP;
    int32_t rc;
    if ((rc = sl.prepped.ensure(n * wb + 16)) || (rc = sl.in_bases.ensure(n * sz + 16)) || (is_inf && (rc = sl.in_inf.ensure(n + 16)))) return rc;
    uint8_t *dw = sl.prepped.as<uint8_t>(), *dout = sl.in_bases.as<uint8_t>(), *dinf = is_inf ? sl.in_inf.as<uint8_t>() : nullptr;
    auto in = [&](size_t lo, size_t hi) {
        return hipMemcpyAsync(dw + lo * wb, (const uint8_t *)xy + lo * wb, (hi - lo) * wb, hipMemcpyHostToDevice, sl.cstream) != hipSuccess ||
               (dinf && hipMemcpyAsync(dinf + lo, is_inf + lo, hi - lo, hipMemcpyHostToDevice, sl.cstream) != hipSuccess);
    };
    auto enc = [&](size_t lo, size_t hi) { serde::launch_serialize_words(sl.stream, C::NFP, comp, (const uint32_t *)dw, dinf, lo, hi, (uint32_t *)dout); };
    auto copy = [&](size_t lo, size_t hi) { return hipMemcpyAsync(out + lo * sz, dout + lo * sz, (hi - lo) * sz, hipMemcpyDeviceToHost, sl.cstream) != hipSuccess; };
    rc = encode_queue(sl, n, sz, true, in, enc, copy);
    return drain(sl, rc);
}

// Points [offset, offset + n) of a resident bases handle of the curve (kind: plain 1 / 2; its precomputed table kind + 9, whose row 0 holds the
// points' own records; a sharded set kind + 6, every part on its own context) -> enc = 0: ABI words into xy and / or flags into is_inf; enc = 1 / 2:
// the compressed / uncompressed encoding into out.  The handle is pinned for the call, which runs on the context that owns it.
template <class C>
int32_t bases_encode(uint64_t handle, size_t offset, size_t n, int enc, uint64_t *xy, uint8_t *is_inf, uint8_t *out, int kind) {
    if (n && (enc ? !out : (!xy && !is_inf))) return DGPU_E_BADARG;
    HandleRef hb(handle);
    const int k = hb.ok ? hb.h.kind : 0;
    if ((k != kind && k != kind + 6 && k != kind + 9) || offset > hb.h.n || n > hb.h.n - offset) return DGPU_E_BADARG;
    if (n == 0) return DGPU_OK;
    const size_t wb = (size_t)2 * C::ABI_W * 4, sz = (enc == 1 ? 48 : 96) * (size_t)C::NFP;
    if (k == kind + 6) {                             // every part that overlaps the range, in global index order
        const ShardSet &ss = *(const ShardSet *)hb.h.p;
        return run_shards(ss.sub.size(), [&](size_t s) -> int32_t {
            const size_t lo = std::max(ss.lo[s], offset), hi = std::min(ss.lo[s + 1], offset + n);
            if (lo >= hi) return DGPU_OK;
            const size_t at = lo - offset;
            return bases_encode<C>(ss.sub[s], lo - ss.lo[s], hi - lo, enc, xy ? xy + at * (wb / 8) : nullptr, is_inf ? is_inf + at : nullptr, out ? out + at * sz : nullptr, kind);
        });
    }
    CtxScope on_owner(hb.h.ctx);
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    const uint32_t *recs = (const uint32_t *)(k == kind + 9 ? ((const PreTable *)hb.h.p)->tab : hb.h.p) + offset * C::AFF_STRIDE;
    int32_t rc;
    if (enc) {
        if ((rc = sl.in_bases.ensure(n * sz + 16))) return rc;
        uint8_t *dout = sl.in_bases.as<uint8_t>();
        auto run = [&](size_t lo, size_t hi) { serde::launch_read_records(sl.stream, C::NFP, enc, recs, lo, hi, nullptr, nullptr, (uint32_t *)dout); };
        auto copy = [&](size_t lo, size_t hi) { return hipMemcpyAsync(out + lo * sz, dout + lo * sz, (hi - lo) * sz, hipMemcpyDeviceToHost, sl.cstream) != hipSuccess; };
        rc = encode_queue(sl, n, sz, false, [](size_t, size_t) { return false; }, run, copy);
    } else {
        if ((xy && (rc = sl.prepped.ensure(n * wb + 16))) || (is_inf && (rc = sl.in_inf.ensure(n + 16)))) return rc;
        uint8_t *dw = xy ? sl.prepped.as<uint8_t>() : nullptr, *dinf = is_inf ? sl.in_inf.as<uint8_t>() : nullptr;
        auto run = [&](size_t lo, size_t hi) { serde::launch_read_records(sl.stream, C::NFP, 0, recs, lo, hi, (uint32_t *)dw, dinf, nullptr); };
        auto copy = [&](size_t lo, size_t hi) {
            return (dw && hipMemcpyAsync((uint8_t *)xy + lo * wb, dw + lo * wb, (hi - lo) * wb, hipMemcpyDeviceToHost, sl.cstream) != hipSuccess) ||
                   (dinf && hipMemcpyAsync(is_inf + lo, dinf + lo, hi - lo, hipMemcpyDeviceToHost, sl.cstream) != hipSuccess);
        };
        rc = encode_queue(sl, n, (xy ? wb : 0) + (is_inf ? 1 : 0), false, [](size_t, size_t) { return false; }, run, copy);
    }
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
int32_t dgpu_g1_serialize_device(const uint64_t *xy, const uint8_t *is_inf, size_t n, int32_t compressed, uint8_t *out) { return serialize_device<G1>(xy, is_inf, n, compressed, out); }
int32_t dgpu_g2_serialize_device(const uint64_t *xy, const uint8_t *is_inf, size_t n, int32_t compressed, uint8_t *out) { return serialize_device<G2>(xy, is_inf, n, compressed, out); }
int32_t dgpu_bases_read_g1(uint64_t handle, size_t offset, size_t n, uint64_t *xy, uint8_t *is_inf) { return bases_encode<G1>(handle, offset, n, 0, xy, is_inf, nullptr, 1); }
int32_t dgpu_bases_read_g2(uint64_t handle, size_t offset, size_t n, uint64_t *xy, uint8_t *is_inf) { return bases_encode<G2>(handle, offset, n, 0, xy, is_inf, nullptr, 2); }
int32_t dgpu_bases_serialize_g1(uint64_t handle, size_t offset, size_t n, int32_t compressed, uint8_t *out) {
    return bases_encode<G1>(handle, offset, n, compressed ? 1 : 2, nullptr, nullptr, out, 1); }
int32_t dgpu_bases_serialize_g2(uint64_t handle, size_t offset, size_t n, int32_t compressed, uint8_t *out) {
    return bases_encode<G2>(handle, offset, n, compressed ? 1 : 2, nullptr, nullptr, out, 2); }
}  // extern "C"
