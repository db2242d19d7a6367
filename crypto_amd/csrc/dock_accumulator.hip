// crypto_amd/csrc/dock_accumulator.hip — the accumulator manager's batch witness update (include/dock_gpu.h: dgpu_accumulator_update_factors,
// dgpu_accumulator_update_witnesses_g1).  Replaces Witness::compute_update_using_secret_key_after_batch_updates and its additions-only / removals-only
// forms (vb_accumulator/src/witness.rs:165-285) with the polynomial evaluations of vb_accumulator/src/batch_utils.rs:81-470 in front:
//   host    F_s, G_s, Phi from the secret key (O(|A| + |D|), one inversion); alpha never leaves the host
//   device  f_i = d_A(y_i) / d_D(y_i), g_i = v_AD(y_i) / d_D(y_i)                 k_acc_prep, k_acc_eval [, k_acc_combine]   (acc_kernels.hip.h)
//   host    the GLV split of every f_i (the caller gets f anyway: 64 bytes per holder come back)
//   device  T_i = g_i V from a window table of V (k_fb_mul), C_i' = T_i + f_i C_i (k_g1_scale_quad with T as the addend)
// The device copy of the tables is zeroed before the slot is released; nothing of a call is kept.
#include <chrono>
#include "msm_driver.hip.h"
#include "fixed_launch.hip.h"
#include "acc_launch.hip.h"
#include "acc_host_tables.hpp"
using namespace dock;
using namespace acch;

namespace {

// zeroes the device copy of the tables on every return path, before the slot goes back
struct DeviceWipe {
    Slot &sl; void *p = nullptr; size_t bytes = 0;
    explicit DeviceWipe(Slot &s) : sl(s) {}
    ~DeviceWipe() { if (p) { (void)hipMemsetAsync(p, 0, bytes, sl.stream); (void)hipStreamSynchronize(sl.stream); } }
};
double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

bool bad_sizes(size_t na, size_t nr, size_t m) { return m >= (1ull << 31) || na >= (1ull << 31) || nr >= (1ull << 31) || na + nr >= (1ull << 31); }

// f, g of every element: canonical words on the device (sl.q[3]: f, then g) and in fg_host (2 m x 4 words).  The slot is the caller's.
int32_t factors_on_slot(Slot &sl, const Tables &t, size_t na, size_t nr, const uint64_t *elements, size_t m, bool mont, std::vector<uint64_t> &fg_host) {
    const size_t ne = acck::acc_table_entries(na, nr), words_b = (ne * 32 + 255) & ~(size_t)255, tab_b = (ne * 40 + 255) & ~(size_t)255;
    const acck::AccShape sh = acck::acc_shape(m, na, nr, gs.acc_split.load());
    gs.acc_last_split = (int)sh.K;
    int32_t rc;
    // q[0]: the tables (words | internal form), q[1]: chunk results, q[2]: scratch slots, q[3]: f | g, q[4]: the elements
    if ((rc = sl.q[0].ensure(words_b + tab_b))) return rc;
    if ((rc = sl.q[1].ensure(acck::acc_part_bytes(m, sh) + 256))) return rc;
    if ((rc = sl.q[2].ensure(acck::acc_scratch_bytes(m)))) return rc;
    if ((rc = sl.q[3].ensure(2 * m * 32))) return rc;
    if ((rc = sl.q[4].ensure(m * 32))) return rc;
    hipStream_t s = sl.stream;
    DeviceWipe dw(sl); dw.p = sl.q[0].p; dw.bytes = words_b + tab_b;
    uint32_t *d_words = sl.q[0].as<uint32_t>(), *d_tab = (uint32_t *)(sl.q[0].as<uint8_t>() + words_b);
    HIPCHK(hipMemcpyAsync(d_words, t.w.data(), ne * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[4].p, elements, m * 32, hipMemcpyHostToDevice, s));
    { StageTimer st(sl, "acc.prep"); acck::launch_acc_prep(s, d_words, ne, d_tab); }
    { StageTimer st(sl, "acc.factors");
      acck::launch_acc_factors(s, d_tab, na, nr, sl.q[4].as<uint32_t>(), mont ? 1 : 0, m, sh, sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), sl.q[3].as<uint32_t>()); }
    HIPCHK(hipGetLastError());
    fg_host.resize(2 * m * 4);
    HIPCHK(hipMemcpyAsync(fg_host.data(), sl.q[3].p, 2 * m * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return DGPU_OK;
}
// canonical words -> what the caller asked for
void factors_out(const uint64_t *canon, size_t m, bool mont, uint64_t *out) {
    if (!mont) { memcpy(out, canon, m * 32); return; }
    for (size_t i = 0; i < m; i++) { const FrH x = fr_in(canon + 4 * i, false); memcpy(out + 4 * i, x.l, 32); }
}

int32_t update_factors(const uint64_t *additions, size_t na, const uint64_t *removals, size_t nr, const uint64_t *alpha, const uint64_t *elements, size_t m, bool mont,
                       uint64_t *f, uint64_t *g) {
    if (m == 0) return DGPU_OK;
    if ((na && !additions) || (nr && !removals) || !alpha || !elements || !f || !g || bad_sizes(na, nr, m)) return DGPU_E_BADARG;
    Tables t;
    int32_t rc = build_tables(additions, na, removals, nr, alpha, mont, t);
    if (rc) return rc;
    if (!cur().ready) return DGPU_E_NODEVICE;
    std::vector<uint64_t> fg;
    {
        SLOT_ACQUIRE(L, sl);
        HIPCHK(hipSetDevice(cur().device));
        rc = factors_on_slot(sl, t, na, nr, elements, m, mont, fg);
        if (gs.prof) prof_flush(sl);
    }
    if (rc) return rc;
    factors_out(fg.data(), m, mont, f); factors_out(fg.data() + 4 * m, m, mont, g);
    return DGPU_OK;
}

int32_t update_witnesses(const uint64_t *additions, size_t na, const uint64_t *removals, size_t nr, const uint64_t *alpha, const uint64_t *elements, const uint64_t *witnesses, size_t m,
                         const uint64_t *accumulator, bool mont, uint64_t *d_factors, uint64_t *out, uint8_t *out_inf) {
    if (m == 0) return DGPU_OK;
    if ((na && !additions) || (nr && !removals) || !alpha || !elements || !witnesses || !accumulator || !d_factors || !out || !out_inf || bad_sizes(na, nr, m)) return DGPU_E_BADARG;
    Tables t;
    auto t0 = std::chrono::steady_clock::now();
    int32_t rc = build_tables(additions, na, removals, nr, alpha, mont, t);
    if (rc) return rc;
    if (!cur().ready) return DGPU_E_NODEVICE;
    if (gs.prof) prof_add_host("acc.host_tables", ms_since(t0));
    // the window table of V, built on a slot of its own before this call takes one (two slots held at once by every caller could starve each other)
    uint64_t table = 0;
    if ((rc = dgpu_window_table_g1(accumulator, &table))) return rc;
    struct TableFree { uint64_t h; ~TableFree() { (void)dgpu_window_table_free(h); } } table_free{table};
    HandleRef tref(table);
    if (!tref.ok) return DGPU_E_BADARG;
    CtxScope on_owner(tref.h.ctx);
    std::vector<uint64_t> fg;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    if ((rc = factors_on_slot(sl, t, na, nr, elements, m, mont, fg))) { if (gs.prof) prof_flush(sl); return rc; }
    const size_t pt = 96;
    // in_bases: [witnesses | T], in_inf: T's identity flags, in_scalars: the split f, prepped: [out | out_inf]
    if ((rc = sl.in_bases.ensure(2 * m * pt))) return rc;
    if ((rc = sl.in_inf.ensure(m))) return rc;
    if ((rc = sl.in_scalars.ensure(m * 32))) return rc;
    if ((rc = sl.prepped.ensure(m * pt + m))) return rc;
    hipStream_t s = sl.stream;
    uint8_t *dC = sl.in_bases.as<uint8_t>(), *dT = dC + m * pt, *dTinf = sl.in_inf.as<uint8_t>(), *dout_inf = sl.prepped.as<uint8_t>() + m * pt;
    HIPCHK(hipMemcpyAsync(dC, witnesses, m * pt, hipMemcpyHostToDevice, s));
    { StageTimer st(sl, "acc.table_mul");          // runs under the host's split of f
      msm::launch_fb_mul<msm::G1>(s, (const uint32_t *)tref.h.p, sl.q[3].as<uint32_t>() + m * 8, m, (uint32_t *)dT, dTinf); }
    HIPCHK(hipGetLastError());
    t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> split(m * 4);
    const size_t parts = std::min<size_t>(16, (m + 4095) / 4096);
    rc = par_run(parts, [&](size_t k) {
        const size_t lo = m * k / parts, hi = m * (k + 1) / parts;
        for (size_t i = lo; i < hi; i++) hostf::glv_decompose(fg.data() + 4 * i, &split[4 * i], &split[4 * i + 2]);
        return (int32_t)DGPU_OK;
    });
    if (gs.prof) prof_add_host("acc.glv_split", ms_since(t0));
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    HIPCHK(hipMemcpyAsync(sl.in_scalars.p, split.data(), m * 32, hipMemcpyHostToDevice, s));
    { StageTimer st(sl, "acc.scale");
      msm::launch_g1_scale_quad(s, (const uint32_t *)dC, nullptr, sl.in_scalars.as<uint32_t>(), 8, nullptr, m, sl.prepped.as<uint32_t>(), dout_inf, (const uint32_t *)dT, dTinf); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, sl.prepped.p, m * pt, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_inf, dout_inf, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (gs.prof) prof_flush(sl);
    factors_out(fg.data(), m, mont, d_factors);
    return DGPU_OK;
}

}  // namespace

extern "C" {
int32_t dgpu_accumulator_update_factors(const uint64_t *additions, size_t n_add, const uint64_t *removals, size_t n_rem, const uint64_t alpha[4], const uint64_t *elements, size_t m,
                                        int32_t montgomery, uint64_t *f, uint64_t *g) {
    return abi_guard([&] { return update_factors(additions, n_add, removals, n_rem, alpha, elements, m, montgomery != 0, f, g); });
}
int32_t dgpu_accumulator_update_witnesses_g1(const uint64_t *additions, size_t n_add, const uint64_t *removals, size_t n_rem, const uint64_t alpha[4], const uint64_t *elements,
                                             const uint64_t *witnesses_xy, size_t m, const uint64_t accumulator_xy[12], int32_t montgomery, uint64_t *d_factors, uint64_t *out_xy, uint8_t *out_inf) {
    return abi_guard([&] { return update_witnesses(additions, n_add, removals, n_rem, alpha, elements, witnesses_xy, m, accumulator_xy, montgomery != 0, d_factors, out_xy, out_inf); });
}
}  // extern "C"
