// crypto_amd/csrc/dock_accumulator.hip — the accumulator's batch witness updates (include/dock_gpu.h: dgpu_accumulator_update_factors,
// dgpu_accumulator_update_witnesses_g1 with the secret key; dgpu_accumulator_omega_g1 and dgpu_accumulator_update_witnesses_public_g1, the two halves of
// the update from public information, further down; dgpu_accumulator_d_for_batch[_resident] and the two calls that issue witnesses at the end).  Replaces Witness::compute_update_using_secret_key_after_batch_updates and its additions-only / removals-only
// forms (vb_accumulator/src/witness.rs:165-285) with the polynomial evaluations of vb_accumulator/src/batch_utils.rs:81-470 in front:
//   host    F_s, G_s, Phi from the secret key (O(|A| + |D|), one inversion); alpha never leaves the host
//   device  f_i = d_A(y_i) / d_D(y_i), g_i = v_AD(y_i) / d_D(y_i)                 k_acc_prep, k_acc_eval [, k_acc_combine]   (acc_kernels.hip.h)
//   host    the GLV split of every f_i (the caller gets f anyway: 64 bytes per holder come back)
//   device  T_i = g_i V from a window table of V (k_fb_mul), C_i' = T_i + f_i C_i (k_g1_scale_quad with T as the addend)
// The device copy of the tables is zeroed before the slot is released; nothing of a call is kept.
#include "msm_many.hip.h"
#include "qap_launch.hip.h"
#include "fixed_launch.hip.h"
#include "acc_launch.hip.h"
#include "acc_host_tables.hpp"
using namespace dock;
using namespace acch;

namespace {

constexpr size_t PT = 96;                 // bytes of an affine G1 point of the ABI

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
    DeviceWipe dw(sl); dw.add(sl.q[0].p, words_b + tab_b);
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
    // in_bases: [witnesses | T], in_inf: T's identity flags, in_scalars: the split f, prepped: [out | out_inf]
    if ((rc = sl.in_bases.ensure(2 * m * PT))) return rc;
    if ((rc = sl.in_inf.ensure(m))) return rc;
    if ((rc = sl.in_scalars.ensure(m * 32))) return rc;
    if ((rc = sl.prepped.ensure(m * PT + m))) return rc;
    hipStream_t s = sl.stream;
    uint8_t *dC = sl.in_bases.as<uint8_t>(), *dT = dC + m * PT, *dTinf = sl.in_inf.as<uint8_t>(), *dout_inf = sl.prepped.as<uint8_t>() + m * PT;
    HIPCHK(hipMemcpyAsync(dC, witnesses, m * PT, hipMemcpyHostToDevice, s));
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
    HIPCHK(hipMemcpyAsync(out, sl.prepped.p, m * PT, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_inf, dout_inf, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (gs.prof) prof_flush(sl);
    factors_out(fg.data(), m, mont, d_factors);
    return DGPU_OK;
}

// ---- the update from public information (section 4.1 of the paper) ------------------------------------------------------------------------------------
// The manager's half, Omega::new (vb_accumulator/src/batch_utils.rs:498-509) without polynomial arithmetic: v_AD has L = max(|A|, |D|) coefficients, so
//   device  the N-th roots of unity, N = 2^logn >= L                                                       k_fr_powers
//   device  v_AD = v_A - Phi v_D at each of them: the passes of the witness update, another finishing         k_acc_prep, k_acc_omega_eval [, k_acc_omega_combine]
//   device  ONE inverse transform of size N over the context's cached domain (N <= 2: in the next kernel)     launch_ntt
//   device  / N, un-reversal, canonical words, a non-zero flag per coefficient                                 k_acc_omega_coeffs
//   device  c_j V from a window table of V, the coefficients still on the device                               k_fb_mul
// The window table is built into the slot's own workspace (window_table_g1_on_slot, queued on the call's stream), not through dgpu_window_table_g1: a steady-state
// call allocates nothing and waits for the device once.
constexpr size_t OMEGA_MAX = DGPU_ACC_OMEGA_MAX;

int32_t omega_g1(const uint64_t *additions, size_t na, const uint64_t *removals, size_t nr, const uint64_t *alpha, const uint64_t *accumulator, bool mont,
                 uint64_t *out, uint8_t *out_inf, size_t *out_len) {
    if ((na && !additions) || (nr && !removals) || !alpha || !accumulator || !out_len || na >= (1ull << 31) || nr >= (1ull << 31)) return DGPU_E_BADARG;
    const size_t L = std::max(na, nr);
    if (L > OMEGA_MAX || (L && (!out || !out_inf))) return DGPU_E_BADARG;
    if (L == 0) { *out_len = 0; return DGPU_OK; }
    Tables t;
    auto t0 = std::chrono::steady_clock::now();
    int32_t rc = build_tables(additions, na, removals, nr, alpha, mont, t);
    if (rc) return rc;
    if (!cur().ready) return DGPU_E_NODEVICE;
    if (gs.prof) prof_add_host("acc.host_tables", ms_since(t0));
    int logn = 0; while (((size_t)1 << logn) < L) logn++;
    const size_t N = (size_t)1 << logn;
    uint64_t consts[3][4];                                    // the generator of the N-th roots of unity, one, 1 / N: canonical
    FrH::root_of_unity(logn).to_canonical(consts[0]); FrH::from_u64(1).to_canonical(consts[1]); FrH::from_u64(N).inv().to_canonical(consts[2]);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    NttDomain dom;
    if (logn >= 2 && (rc = get_domain(sl, logn, dom))) return rc;
    const size_t ne = acck::acc_table_entries(na, nr), words_b = (ne * 32 + 255) & ~(size_t)255, tab_b = (ne * 40 + 255) & ~(size_t)255, esz = ntt::FR_WORDS * 4;
    const acck::AccShape sh = acck::acc_shape(N, na, nr, gs.acc_split.load());
    gs.acc_last_split = (int)sh.K;
    // q[0]: the tables (words | internal form), q[1]: chunk results, q[3]: the coefficients, q[5]: the constants, q[6]: the roots, q[7]: the evaluations,
    // q[8]: the non-zero flags, q[9]: the window table of V, q[10]: [c_j V | identity flags]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure(words_b + tab_b))) return e;
        if ((e = o.q[1].ensure(acck::acc_part_bytes(N, sh) + 256))) return e;
        if ((e = o.q[3].ensure(L * 32))) return e;
        if ((e = o.q[5].ensure(256))) return e;
        if ((e = o.q[6].ensure(N * esz))) return e;
        if ((e = o.q[7].ensure(N * esz))) return e;
        if ((e = o.q[8].ensure(L))) return e;
        if ((e = o.q[9].ensure(window_table_g1_bytes()))) return e;
        if ((e = o.q[10].ensure(L * PT + L))) return e;
        if ((e = o.prepped.ensure(32 * G1::AFF_STRIDE * 4))) return e;                  // (the window table's scratch)
        return o.in_bases.ensure(32 * 2 * G1::ABI_W * 4 + 16);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<uint64_t> window_bases;                       // (host words of the table's upload: they live until the call's synchronisation)
    std::vector<uint8_t> nz(L);
    DrainUnlessDone guard(sl);
    if ((rc = window_table_g1_on_slot(sl, accumulator, sl.q[9].p, window_bases))) return rc;
    DeviceWipe dw(sl);
    dw.add(sl.q[0].p, words_b + tab_b); dw.add(sl.q[1].p, acck::acc_part_bytes(N, sh)); dw.add(sl.q[7].p, N * esz); dw.add(sl.q[3].p, L * 32); dw.add(sl.q[8].p, L);
    uint32_t *d_words = sl.q[0].as<uint32_t>(), *d_tab = (uint32_t *)(sl.q[0].as<uint8_t>() + words_b), *d_c = sl.q[5].as<uint32_t>(), *d_ev = sl.q[7].as<uint32_t>();
    uint8_t *d_out = sl.q[10].as<uint8_t>(), *d_inf = d_out + L * PT;
    HIPCHK(hipMemcpyAsync(d_words, t.w.data(), ne * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_c, consts, sizeof consts, hipMemcpyHostToDevice, s));
    { StageTimer st(sl, "acc.prep"); acck::launch_acc_prep(s, d_words, ne, d_tab); ntt::launch_fr_powers(s, d_c, d_c + 8, N, sl.q[6].as<uint32_t>()); }
    { StageTimer st(sl, "acc.omega_eval"); acck::launch_acc_omega_eval(s, d_tab, na, nr, sl.q[6].as<uint32_t>(), N, sh, sl.q[1].as<uint32_t>(), d_ev); }
    { StageTimer st(sl, "acc.omega_intt");
      if (logn >= 2) ntt::launch_ntt(s, d_ev, logn, (const uint32_t *)dom.tw_i, 1);
      acck::launch_acc_omega_coeffs(s, d_ev, logn, (const uint32_t *)consts[2], L, sl.q[3].as<uint32_t>(), sl.q[8].as<uint8_t>()); }
    { StageTimer st(sl, "acc.omega_mul"); msm::launch_fb_mul<msm::G1>(s, sl.q[9].as<uint32_t>(), sl.q[3].as<uint32_t>(), L, (uint32_t *)d_out, d_inf); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, L * PT, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_inf, d_inf, L, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(nz.data(), sl.q[8].p, L, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    guard.done = true;
    if (gs.prof) prof_flush(sl);
    // ark-poly drops trailing zero coefficients; a zero coefficient below the last non-zero one, and every entry of an identity accumulator, is an identity
    size_t len = L; while (len && !nz[len - 1]) len--;
    for (size_t j = 0; j < L; j++) if (j >= len || !nz[j] || out_inf[j]) { memset(out + 12 * j, 0, PT); out_inf[j] = 1; }
    *out_len = len;
    return DGPU_OK;
}

// The holders' half, m times Witness::compute_update_using_public_info_after_batch_updates (witness.rs:292-314) with Omega::evaluate (batch_utils.rs:664-691):
//   device  f_i = d_A(y_i) / d_D(y_i), s_i = 1 / d_D(y_i)                                  k_acc_prep, k_acc_pub_factors [, k_acc_pub_combine]
//   device  row i = [s_i, s_i y_i, ..] straight into the many-row MSM's scalar buffer      k_acc_pub_rows
//   device  T_i = <row_i, omega> over the small-path table of omega                        k_many_tree, k_many_fold (msm_many.hip.h RowMsm)
//   host    the GLV split of every f_i, under the MSM
//   device  C_i' = T_i + f_i C_i                                                           k_g1_scale_quad
// omega's prepared records and their table live in the slot's workspace for the call (no handle, so nothing to free and no allocation in steady state).  Beyond
// the many-row kernels' reach a row runs through the single-row driver with its scalars where k_acc_pub_rows left them.
int32_t public_on_slot(Slot &sl, const uint64_t *additions, size_t na, const uint64_t *removals, size_t nr, const uint64_t *omega, const uint8_t *oinf, size_t n,
                       const uint64_t *elements, const uint64_t *witnesses, size_t m, bool mont, uint64_t *d_factors, uint64_t *out, uint8_t *out_inf, uint8_t *ok) {
    const size_t nl = na + nr, words_b = (std::max<size_t>(nl, 1) * 32 + 255) & ~(size_t)255, lists_b = (std::max<size_t>(nl, 1) * 40 + 255) & ~(size_t)255;
    const size_t reach = std::min<size_t>(SMALL_MSM_MAX_N, gs.small_max.load());
    const bool many = n && n <= reach;
    const acck::AccShape sh = acck::acc_shape(m, na, nr, gs.acc_split.load());
    gs.acc_last_split = (int)sh.K;
    int32_t rc;
    // q[0]: the lists (words | internal form), q[1]: chunk results, q[2]: scratch slots, q[3]: f | s, q[4]: the elements, q[5]: the split f, q[6]: [witnesses | T],
    // q[7]: [out | out_inf], q[8]: [T's identity flags | ok], q[9]: omega's prepared records, q[10]: their small-path table
    const RawBases rb = RawBases::packed<G1>(omega, oinf);
    RowMsm<G1> tm(many, n, m, ~(size_t)0);                       // the T_i: omega's records are staged into q[9], their table (many) is built in q[10]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure(words_b + lists_b))) return e;
        if ((e = o.q[1].ensure(acck::acc_part_bytes(m, sh) + 256))) return e;
        if ((e = o.q[2].ensure(acck::acc_scratch_bytes(m)))) return e;
        if ((e = o.q[3].ensure(2 * m * 32))) return e;
        if ((e = o.q[4].ensure(m * 32))) return e;
        if ((e = o.q[5].ensure(m * 32))) return e;
        if ((e = o.q[6].ensure(2 * m * PT))) return e;
        if ((e = o.q[7].ensure(m * PT + m))) return e;
        if ((e = o.q[8].ensure(2 * m))) return e;
        if ((e = o.q[9].ensure(std::max<size_t>(n, 1) * G1::AFF_STRIDE * 4))) return e;
        if (!n) return DGPU_OK;
        if ((e = ws_stage_bases<G1>(o, rb, n))) return e;
        if (many && (e = o.q[10].ensure(small_sub_bytes<G1>(n)))) return e;
        return tm.workspace(o);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<uint64_t> f_host(m * 4), split(m * 4);                                        // targets and sources of asynchronous copies ...
    DrainUnlessDone guard(sl);                                                                // ... so an early return waits for them
    uint32_t *d_words = sl.q[0].as<uint32_t>(), *d_lists = (uint32_t *)(sl.q[0].as<uint8_t>() + words_b), *d_fs = sl.q[3].as<uint32_t>(), *d_el = sl.q[4].as<uint32_t>();
    uint8_t *dC = sl.q[6].as<uint8_t>(), *dT = dC + m * PT, *dTinf = sl.q[8].as<uint8_t>(), *d_ok = dTinf + m, *dout_inf = sl.q[7].as<uint8_t>() + m * PT;
    if (na) HIPCHK(hipMemcpyAsync(d_words, additions, na * 32, hipMemcpyHostToDevice, s));
    if (nr) HIPCHK(hipMemcpyAsync(d_words + na * 8, removals, nr * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_el, elements, m * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dC, witnesses, m * PT, hipMemcpyHostToDevice, s));
    if (nl) { StageTimer st(sl, "acc.prep"); acck::launch_acc_prep(s, d_words, nl, d_lists, mont ? 1 : 0); }
    { StageTimer st(sl, "acc.pub_factors");
      acck::launch_acc_pub_factors(s, d_lists, na, nr, d_el, mont ? 1 : 0, m, sh, sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), d_fs, d_ok); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(f_host.data(), d_fs, m * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ok, d_ok, m, hipMemcpyDeviceToHost, s));
    hipEvent_t have_f = ev_get(sl);
    if (!have_f) return DGPU_E_HIP;
    struct EvBack { Slot &sl; hipEvent_t e; ~EvBack() { sl.ev_pool.push_back(e); } } ev_back{sl, have_f};
    HIPCHK(hipEventRecord(have_f, s));
    // T_i = <row_i, omega>
    if (n == 0) HIPCHK(hipMemsetAsync(dTinf, 1, m, s));
    else {
        uint32_t *d_rec = sl.q[9].as<uint32_t>(), *d_rows = sl.in_scalars.as<uint32_t>(), *d_bad = sl.flags.as<uint32_t>();
        if ((rc = stage_bases<G1>(sl, rb, n, d_rec))) return rc;
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                  // (rows are canonical: the flag stays clear)
        tm.rec = d_rec;
        if (many) {
            tm.sub = SmallSub{sl.q[10].as<uint32_t>(), sl.q[10].as<uint8_t>() + small_sub_tab_bytes<G1>(n)};
            StageTimer st(sl, "msm.small_subtable");
            launch_small_subtable<G1>(s, d_rec, n, sl.q[10].as<uint32_t>(), sl.q[10].as<uint8_t>() + small_sub_tab_bytes<G1>(n));
        }
        for (size_t r0 = 0; r0 < m; r0 += tm.chunk) {
            const size_t rows = std::min(tm.chunk, m - r0);
            { StageTimer st(sl, "acc.pub_rows"); acck::launch_acc_pub_rows(s, d_el + r0 * 8, mont ? 1 : 0, d_fs + (m + r0) * 8, rows, n, d_rows); }
            if ((rc = tm.points(sl, d_rows, rows, d_bad, dT + r0 * PT, dTinf + r0))) return rc;
        }
    }
    HIPCHK(hipEventSynchronize(have_f));
    auto t0 = std::chrono::steady_clock::now();
    const size_t parts = std::min<size_t>(16, (m + 4095) / 4096);
    rc = par_run(parts, [&](size_t k) {
        const size_t lo = m * k / parts, hi = m * (k + 1) / parts;
        for (size_t i = lo; i < hi; i++) hostf::glv_decompose(f_host.data() + 4 * i, &split[4 * i], &split[4 * i + 2]);
        return (int32_t)DGPU_OK;
    });
    if (gs.prof) prof_add_host("acc.glv_split", ms_since(t0));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(sl.q[5].p, split.data(), m * 32, hipMemcpyHostToDevice, s));
    { StageTimer st(sl, "acc.scale");
      msm::launch_g1_scale_quad(s, (const uint32_t *)dC, nullptr, sl.q[5].as<uint32_t>(), 8, nullptr, m, sl.q[7].as<uint32_t>(), dout_inf, (const uint32_t *)dT, dTinf); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, sl.q[7].p, m * PT, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_inf, dout_inf, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    guard.done = true;
    // a zero d_D is the reference's Err(CannotBeZero) for that holder alone: ok = 0, a zero factor, the identity
    for (size_t i = 0; i < m; i++) {
        if (!ok[i]) { memset(f_host.data() + 4 * i, 0, 32); out_inf[i] = 1; }
        if (out_inf[i]) memset(out + 12 * i, 0, PT);
    }
    factors_out(f_host.data(), m, mont, d_factors);
    return DGPU_OK;
}

int32_t update_witnesses_public(const uint64_t *additions, size_t na, const uint64_t *removals, size_t nr, const uint64_t *omega, const uint8_t *omega_inf, size_t n,
                                const uint64_t *elements, const uint64_t *witnesses, size_t m, bool mont, uint64_t *d_factors, uint64_t *out, uint8_t *out_inf, uint8_t *ok) {
    if (m == 0) return DGPU_OK;
    if ((na && !additions) || (nr && !removals) || (n && !omega) || !elements || !witnesses || !d_factors || !out || !out_inf || !ok || bad_sizes(na, nr, m) || n >= (1ull << 31))
        return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    // an identity entry of omega: its flag, or zero words (the convention of the points this library writes)
    std::vector<uint8_t> oinf(n);
    for (size_t j = 0; j < n; j++) {
        uint64_t any = 0; for (int k = 0; k < 12; k++) any |= omega[12 * j + k];
        oinf[j] = ((omega_inf && omega_inf[j]) || !any) ? 1 : 0;
    }
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    const int32_t rc = public_on_slot(sl, additions, na, removals, nr, omega, oinf.data(), n, elements, witnesses, m, mont, d_factors, out, out_inf, ok);
    if (rc) drain(sl);                                           // nothing of ours still reads the caller's memory
    if (gs.prof) prof_flush(sl);
    return rc;
}

// ---- issuing witnesses (universal.rs:461-583, positive.rs:369-381) ---------------------------------------------------------------------------------------
// d_i = d_in_i prod_j (member_j - y_i) over ALL members of the accumulator: m n products for a batch of m against an accumulator of n, n the large number.
//   device  the members of one pass (at most ACC_D_PASS; from the host, or straight out of a resident scalars handle) -> internal form     k_acc_prep
//   device  every lane walks the pass once for the one or four non-members it owns, in K chunks when the lanes alone do not fill the device   k_acc_d [, k_acc_d_combine]
// The running products stay on the device in internal form between the passes; the last pass writes words.  Nothing here is secret: nothing is wiped.
int32_t d_on_slot(Slot &sl, const uint64_t *members, const uint32_t *resident, size_t n, const uint64_t *non_members, size_t m, bool mont, const uint64_t *d_in,
                  uint64_t *d_out, uint8_t *nonzero) {
    const size_t forced_pass = (size_t)gs.acc_d_pass.load(), pass = forced_pass ? forced_pass : acck::ACC_D_PASS, longest = std::min(n, pass);
    const int forced = gs.acc_split.load(), U = acck::acc_d_unroll(m, longest, gs.acc_d_unroll.load(), forced);
    const size_t G = acck::acc_d_lanes(m, U);
    const uint32_t K0 = acck::acc_shape(G, longest, 0, forced).K;                 // (a shorter last pass never has more chunks)
    gs.acc_last_split = (int)K0; gs.acc_d_last_unroll = U;
    const size_t words_b = resident ? 0 : (std::max<size_t>(longest, 1) * 32 + 255) & ~(size_t)255, tab_b = (std::max<size_t>(longest, 1) * 40 + 255) & ~(size_t)255;
    // q[0]: the members of a pass (words | internal form), q[1]: chunk products, q[2]: the running products, q[3]: d, q[4]: the non-members, q[5]: d_in, q[8]: non-zero flags
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure(words_b + tab_b))) return e;
        if ((e = o.q[1].ensure(acck::acc_d_part_bytes(m, K0) + 256))) return e;
        if ((e = o.q[2].ensure(acck::acc_d_run_bytes(m)))) return e;
        if ((e = o.q[3].ensure(m * 32))) return e;
        if ((e = o.q[4].ensure(m * 32))) return e;
        if ((e = o.q[5].ensure(m * 32))) return e;
        return o.q[8].ensure(m);
    };
    int32_t rc;
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_words = sl.q[0].as<uint32_t>(), *d_tab = (uint32_t *)(sl.q[0].as<uint8_t>() + words_b), *d_el = sl.q[4].as<uint32_t>();
    const uint32_t *d_din = d_in ? sl.q[5].as<uint32_t>() : nullptr;
    HIPCHK(hipMemcpyAsync(d_el, non_members, m * 32, hipMemcpyHostToDevice, s));
    if (d_in) HIPCHK(hipMemcpyAsync(sl.q[5].p, d_in, m * 32, hipMemcpyHostToDevice, s));
    for (size_t lo = 0;; lo += pass) {
        const size_t len = std::min(pass, n - lo);
        const bool first = lo == 0, last = lo + len >= n;
        if (len) {
            if (!resident) HIPCHK(hipMemcpyAsync(d_words, members + 4 * lo, len * 32, hipMemcpyHostToDevice, s));      // (queued behind the pass before: its prep has read the words)
            StageTimer st(sl, "acc.d_prep");
            acck::launch_acc_prep(s, resident ? resident + lo * 8 : d_words, len, d_tab, resident ? 0 : (mont ? 1 : 0));
        }
        { StageTimer st(sl, "acc.d_eval");
          acck::launch_acc_d(s, d_tab, len, d_el, mont ? 1 : 0, m, U, acck::acc_shape(G, len, 0, forced).K, d_din, first, last, sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(),
                             sl.q[3].as<uint32_t>(), sl.q[8].as<uint8_t>()); }
        if (last) break;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d_out, sl.q[3].p, m * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(nonzero, sl.q[8].p, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    guard.done = true;
    return DGPU_OK;
}
// members: the host's words, or (resident) the handle of a resident scalar vector whose entries [offset, offset + n) are read where they lie
int32_t d_for_batch(const uint64_t *members, bool resident, uint64_t handle, size_t offset, size_t n, const uint64_t *non_members, size_t m, bool mont, const uint64_t *d_in,
                    uint64_t *d_out, uint8_t *nonzero) {
    if (m == 0) return DGPU_OK;
    if ((!resident && n && !members) || !non_members || !d_out || !nonzero || m >= (1ull << 31) || n >= (1ull << 31)) return DGPU_E_BADARG;
    HandleRef hs;
    if (resident && (!hs.acquire(handle) || hs.h.kind != 3 || hs.h.ctx != cur_index() || offset > hs.h.n || n > hs.h.n - offset)) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    const int32_t rc = d_on_slot(sl, members, resident ? (const uint32_t *)hs.h.p + offset * 8 : nullptr, n, non_members, m, mont, d_in, d_out, nonzero);
    if (gs.prof) prof_flush(sl);
    return rc;
}

// C_i = s_i B with s_i = (f_V - d_i) / (y_i + alpha), B = params_gen for non-membership witnesses (compute_non_membership_witnesses_for_batch_given_d,
// universal.rs:499-535) and s_i = 1 / (y_i + alpha), B = V for membership witnesses (compute_membership_witnesses_for_batch, positive.rs:369-381):
//   host    t_i = 1 / (y_i + alpha): one batch inversion per share of the host threads; alpha never leaves the host
//   device  s_i as canonical words straight into the multiplication's scalar buffer, and the zero-d flags        k_acc_issue_scalars
//   device  s_i B from a window table of B built in the slot's workspace, normalised affine points              k_fb_table, k_fb_mul
// The device copies of t, the scalars and the table are zeroed on every return path, the host copy of t too.
int32_t issue_witnesses(bool with_d, const uint64_t *d, const uint64_t *ys, size_t m, const uint64_t *f_V, const uint64_t *alpha, const uint64_t *base, bool mont,
                        uint64_t *out, uint8_t *out_inf, uint8_t *ok) {
    if (m == 0) return DGPU_OK;
    if (!ys || !alpha || !base || !out || !out_inf || (with_d && (!d || !f_V || !ok)) || m >= (1ull << 31)) return DGPU_E_BADARG;
    SecretWords t;
    t.w.assign(m * 4, 0);
    auto t0 = std::chrono::steady_clock::now();
    const size_t parts = std::min<size_t>(16, (m + 1023) / 1024);
    int32_t rc = par_run(parts, [&](size_t k) { return issue_inverses(ys, m * k / parts, m * (k + 1) / parts, alpha, mont, t.w.data()); });
    if (rc) return rc;
    if (!cur().ready) return DGPU_E_NODEVICE;
    if (gs.prof) prof_add_host("acc.host_inverses", ms_since(t0));
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    // q[0]: t, q[3]: the scalars, q[4]: d, q[8]: the zero-d flags, q[9]: the window table of B, q[10]: [s_i B | identity flags]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure(m * 32))) return e;
        if ((e = o.q[3].ensure(m * 32))) return e;
        if ((e = o.q[4].ensure(m * 32))) return e;
        if ((e = o.q[8].ensure(m))) return e;
        if ((e = o.q[9].ensure(window_table_g1_bytes()))) return e;
        if ((e = o.q[10].ensure(m * PT + m))) return e;
        if ((e = o.prepped.ensure(32 * G1::AFF_STRIDE * 4))) return e;                  // (the window table's scratch)
        return o.in_bases.ensure(32 * 2 * G1::ABI_W * 4 + 16);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<uint64_t> window_bases;                       // (host words of the table's upload: they live until the call's synchronisation)
    std::vector<uint8_t> zero(m);
    DrainUnlessDone guard(sl);
    DeviceWipe dw(sl);
    dw.add(sl.q[0].p, m * 32); dw.add(sl.q[3].p, m * 32); dw.add(sl.q[9].p, window_table_g1_bytes());
    if ((rc = window_table_g1_on_slot(sl, base, sl.q[9].p, window_bases))) return rc;
    uint8_t *d_out = sl.q[10].as<uint8_t>(), *d_inf = d_out + m * PT;
    HIPCHK(hipMemcpyAsync(sl.q[0].p, t.w.data(), m * 32, hipMemcpyHostToDevice, s));
    if (with_d) HIPCHK(hipMemcpyAsync(sl.q[4].p, d, m * 32, hipMemcpyHostToDevice, s));
    { StageTimer st(sl, "acc.issue_scalars");
      acck::launch_acc_issue_scalars(s, with_d ? sl.q[4].as<uint32_t>() : nullptr, sl.q[0].as<uint32_t>(), (const uint32_t *)f_V, mont ? 1 : 0, m, sl.q[3].as<uint32_t>(), sl.q[8].as<uint8_t>()); }
    { StageTimer st(sl, "acc.table_mul"); msm::launch_fb_mul<msm::G1>(s, sl.q[9].as<uint32_t>(), sl.q[3].as<uint32_t>(), m, (uint32_t *)d_out, d_inf); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, m * PT, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_inf, d_inf, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(zero.data(), sl.q[8].p, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    guard.done = true;
    if (gs.prof) prof_flush(sl);
    // a zero d is the reference's Err(CannotBeZero) for that entry alone: ok = 0 and the identity; an identity (a zero scalar, an identity base) is zero words
    for (size_t i = 0; i < m; i++) {
        if (with_d) ok[i] = zero[i] ? 0 : 1;
        if (zero[i] || out_inf[i]) { memset(out + 12 * i, 0, PT); out_inf[i] = 1; }
    }
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
int32_t dgpu_accumulator_omega_g1(const uint64_t *additions, size_t n_add, const uint64_t *removals, size_t n_rem, const uint64_t alpha[4], const uint64_t accumulator_xy[12],
                                  int32_t montgomery, uint64_t *omega_xy, uint8_t *omega_inf, size_t *omega_len) {
    return abi_guard([&] { return omega_g1(additions, n_add, removals, n_rem, alpha, accumulator_xy, montgomery != 0, omega_xy, omega_inf, omega_len); });
}
int32_t dgpu_accumulator_update_witnesses_public_g1(const uint64_t *additions, size_t n_add, const uint64_t *removals, size_t n_rem, const uint64_t *omega_xy, const uint8_t *omega_inf,
                                                    size_t n_omega, const uint64_t *elements, const uint64_t *witnesses_xy, size_t m, int32_t montgomery, uint64_t *d_factors, uint64_t *out_xy,
                                                    uint8_t *out_inf, uint8_t *ok) {
    return abi_guard([&] {
        return update_witnesses_public(additions, n_add, removals, n_rem, omega_xy, omega_inf, n_omega, elements, witnesses_xy, m, montgomery != 0, d_factors, out_xy, out_inf, ok);
    });
}
int32_t dgpu_accumulator_d_for_batch(const uint64_t *members, size_t n, const uint64_t *non_members, size_t m, int32_t montgomery, const uint64_t *d_in, uint64_t *d_out, uint8_t *nonzero) {
    return abi_guard([&] { return d_for_batch(members, false, 0, 0, n, non_members, m, montgomery != 0, d_in, d_out, nonzero); });
}
int32_t dgpu_accumulator_d_for_batch_resident(uint64_t members, size_t offset, size_t n, const uint64_t *non_members, size_t m, int32_t montgomery, const uint64_t *d_in, uint64_t *d_out,
                                              uint8_t *nonzero) {
    return abi_guard([&] { return d_for_batch(nullptr, true, members, offset, n, non_members, m, montgomery != 0, d_in, d_out, nonzero); });
}
int32_t dgpu_accumulator_non_membership_witnesses_g1(const uint64_t *d, const uint64_t *non_members, size_t m, const uint64_t f_V[4], const uint64_t alpha[4], const uint64_t params_gen_xy[12],
                                                     int32_t montgomery, uint64_t *out_xy, uint8_t *out_inf, uint8_t *ok) {
    return abi_guard([&] { return issue_witnesses(true, d, non_members, m, f_V, alpha, params_gen_xy, montgomery != 0, out_xy, out_inf, ok); });
}
int32_t dgpu_accumulator_membership_witnesses_g1(const uint64_t *members, size_t m, const uint64_t alpha[4], const uint64_t accumulator_xy[12], int32_t montgomery, uint64_t *out_xy,
                                                 uint8_t *out_inf) {
    return abi_guard([&] { return issue_witnesses(false, nullptr, members, m, nullptr, alpha, accumulator_xy, montgomery != 0, out_xy, out_inf, nullptr); });
}
}  // extern "C"
