// crypto_amd/csrc/dock_gt_dev.hip — GT on the device over many elements (include/dock_gpu.h): dgpu_fp12_pow_batch (`PairingOutput::mul_bigint` per
// element), dgpu_fp12_multi_pow_device (prod a_i^{e_i}: what RandomizedPairingChecker folds per equation, utils/src/randomized_pairing_check.rs:136)
// and dgpu_gt_in_subgroup_device (`Valid::check` of every GT member of a deserialised proof).  Kernels: k_gt_pow.hip, lane functions:
// gt_kernels.hip.h.  The host entry points of dock_gt.cpp stay what every caller inside the library uses; nothing is routed here by size.
//
// One slot per call, the slot's grow-only buffers: ml_out (bases in, results out: ABI), in_scalars (exponents), ml_partial (the power tables:
// 8 entries x 672 B per base), ml_state (products between fold levels, chunk results), flags (verdict bytes).  Chunks of GT_POW_CHUNK elements
// bound the table: 16384 x 5.4 KB = 88 MB, 9.4 MB of elements each way.
#include "dock_ctx.hpp"
#include "gt_launch.hip.h"

using namespace dock;

namespace {
constexpr size_t GT_POW_CHUNK = 16384;
constexpr size_t ELW = 168 * 4, ABIB = 576;       // bytes of an element in the internal form (gt_kernels.hip.h) and in the ABI form

size_t chunk_elems(size_t n) { const size_t c = gs.gt_pow_chunk.load() ? (size_t)gs.gt_pow_chunk.load() : GT_POW_CHUNK; return std::min(n, c); }
size_t fold_out(size_t m) { return (m + 7) / 8; }
// elements of the two regions fold_to_one alternates between for m inputs: the first takes levels 1, 3, .., the second levels 2, 4, ..
size_t fold_a(size_t m) { return fold_out(m) + 1; }
size_t fold_b(size_t m) { return fold_out(fold_out(m)) + 1; }
// workspace of a call over chunks of ch elements, nch chunks (what: 1 powers, 2 product of powers, 3 membership)
int32_t gt_ws(Slot &sl, int what, size_t ch, size_t nch) {
    int32_t rc;
    if ((rc = sl.ml_out.ensure(ch * ABIB * 2))) return rc;
    if (what == 3) return sl.flags.ensure(ch);
    if ((rc = sl.in_scalars.ensure(ch * 32))) return rc;
    if ((rc = sl.ml_partial.ensure(gtk::pow_table_words(ch) * 4))) return rc;
    if (what == 2 && (rc = sl.ml_state.ensure((ch + fold_a(ch) + fold_b(ch) + nch + fold_a(nch) + fold_b(nch)) * ELW))) return rc;
    return DGPU_OK;
}
// in (internal form, m elements) folded level by level; the last level writes ONE element to `last` (ABI if last_abi).  a / b: two scratch regions
// of fold_a(m) and fold_b(m) elements.  m == 1 still runs one level (a copy, converting the form).
void fold_to_one(hipStream_t s, const uint32_t *in, size_t m, uint32_t *a, uint32_t *b, uint32_t *last, bool last_abi) {
    const uint32_t *cur_in = in;
    for (;;) {
        const bool fin = m <= 8;
        uint32_t *dst = fin ? last : a;
        m = gtk::launch_gt_fold(s, cur_in, false, m, 0, dst, fin && last_abi);
        if (fin) return;
        cur_in = dst; std::swap(a, b);
    }
}
}  // namespace

extern "C" {

int32_t dgpu_fp12_pow_batch(const uint64_t *a, const uint64_t *e, size_t e_stride, size_t n, uint64_t *out) {
    if ((n && (!a || !e || !out)) || (e_stride != 0 && e_stride != 4)) return DGPU_E_BADARG;
    if (n == 0) return DGPU_OK;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    const size_t ch = chunk_elems(n);
    const uint64_t allocs0 = g_dev_allocs.load();
    if ((rc = gt_ws(sl, 1, ch, 1))) return rc;
    const bool grew = g_dev_allocs.load() != allocs0;
    hipStream_t s = sl.stream;
    uint32_t *din = sl.ml_out.as<uint32_t>(), *dout = din + ch * 144, *dexp = sl.in_scalars.as<uint32_t>();
    if (!e_stride) HIPCHK(hipMemcpyAsync(dexp, e, 32, hipMemcpyHostToDevice, s));
    for (size_t lo = 0; lo < n; lo += ch) {
        const size_t m = std::min(ch, n - lo);
        HIPCHK(hipMemcpyAsync(din, a + lo * 72, m * ABIB, hipMemcpyHostToDevice, s));
        if (e_stride) HIPCHK(hipMemcpyAsync(dexp, e + lo * 4, m * 32, hipMemcpyHostToDevice, s));
        { StageTimer st(sl, "gt.pow"); gtk::launch_gt_pow(s, din, dexp, e_stride ? 8 : 0, m, gs.gt_pow_g.load(), 1, sl.ml_partial.as<uint32_t>(), dout, true); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + lo * 72, dout, m * ABIB, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (gs.prof) prof_flush(sl);
    if (grew) reserve_idle_slots(&sl, [&](Slot &o) { return gt_ws(o, 1, ch, 1); });      // (the caller's other host threads come with the same shape next)
    return DGPU_OK;
}

int32_t dgpu_fp12_multi_pow_device(const uint64_t *a, const uint64_t *e, size_t n, uint64_t out[72]) {
    if (!out || (n && (!a || !e))) return DGPU_E_BADARG;
    if (n == 0) return dgpu_fp12_multi_pow(nullptr, nullptr, 0, out);          // the element one, no device
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    const size_t ch = chunk_elems(n), nch = (n + ch - 1) / ch;
    const uint64_t allocs0 = g_dev_allocs.load();
    if ((rc = gt_ws(sl, 2, ch, nch))) return rc;
    const bool grew = g_dev_allocs.load() != allocs0;
    hipStream_t s = sl.stream;
    uint32_t *din = sl.ml_out.as<uint32_t>(), *dout = din + ch * 144, *dexp = sl.in_scalars.as<uint32_t>();
    // ml_state: the groups' products | fold scratch a, b | the chunk results | their fold scratch
    uint32_t *prod = sl.ml_state.as<uint32_t>(), *fa = prod + ch * 168, *fb = fa + fold_a(ch) * 168, *cres = fb + fold_b(ch) * 168,
             *ca = cres + nch * 168, *cb = ca + fold_a(nch) * 168;
    const int kset = gs.gt_pow_k.load();
    for (size_t c = 0, lo = 0; lo < n; lo += ch, c++) {
        const size_t m = std::min(ch, n - lo);
        const int k = kset ? kset : gtk::bases_per_group(m);
        HIPCHK(hipMemcpyAsync(din, a + lo * 72, m * ABIB, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dexp, e + lo * 4, m * 32, hipMemcpyHostToDevice, s));
        { StageTimer st(sl, "gt.multi_pow"); gtk::launch_gt_pow(s, din, dexp, 8, m, gs.gt_pow_g.load(), k, sl.ml_partial.as<uint32_t>(), prod, false); }
        { StageTimer st(sl, "gt.fold"); fold_to_one(s, prod, (m + k - 1) / k, fa, fb, nch == 1 ? dout : cres + c * 168, nch == 1); }
        HIPCHK(hipGetLastError());
    }
    if (nch > 1) { StageTimer st(sl, "gt.fold"); fold_to_one(s, cres, nch, ca, cb, dout, true); HIPCHK(hipGetLastError()); }
    HIPCHK(hipMemcpyAsync(out, dout, ABIB, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (gs.prof) prof_flush(sl);
    if (grew) reserve_idle_slots(&sl, [&](Slot &o) { return gt_ws(o, 2, ch, nch); });
    return DGPU_OK;
}

int32_t dgpu_gt_in_subgroup_device(const uint64_t *a, size_t n, uint8_t *ok) {
    if (n && (!a || !ok)) return DGPU_E_BADARG;
    if (n == 0) return DGPU_OK;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    const size_t ch = chunk_elems(n);
    const uint64_t allocs0 = g_dev_allocs.load();
    if ((rc = gt_ws(sl, 3, ch, 1))) return rc;
    const bool grew = g_dev_allocs.load() != allocs0;
    hipStream_t s = sl.stream;
    uint32_t *din = sl.ml_out.as<uint32_t>();
    for (size_t lo = 0; lo < n; lo += ch) {
        const size_t m = std::min(ch, n - lo);
        HIPCHK(hipMemcpyAsync(din, a + lo * 72, m * ABIB, hipMemcpyHostToDevice, s));
        { StageTimer st(sl, "gt.in_subgroup"); gtk::launch_gt_in_subgroup(s, din, m, gs.gt_pow_g.load(), sl.flags.as<uint8_t>()); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ok + lo, sl.flags.p, m, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (gs.prof) prof_flush(sl);
    if (grew) reserve_idle_slots(&sl, [&](Slot &o) { return gt_ws(o, 3, ch, 1); });
    return DGPU_OK;
}

}  // extern "C"
