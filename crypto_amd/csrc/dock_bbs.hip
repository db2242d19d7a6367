// crypto_amd/csrc/dock_bbs.hip — BBS+ signatures in bulk (include/dock_gpu.h: dgpu_bbs_plus_sign_many_g1, dgpu_bbs_plus_verify_each_g1,
// dgpu_bbs_plus_verify_batch_g1): SignatureG1::new and SignatureG1::verify (bbs_plus/src/signature.rs:138-211, 272-296) for many signatures of one key, each
// call ONE device pipeline per chunk of rows.  The signature parameters are a plain G1 bases handle [g1, h_0, h_1 .. h_L]; b_i = g1 + s_i h_0 + sum_j m_ij h_j
// (bbs_plus/src/setup.rs:128-146) is the small MSM of the row (1, s_i, m_i1 .. m_iL) over its small-path table.
//   sign     host    t_i = 1 / (x + e_i): one batch inversion per share of the host threads (acc_host_tables.hpp issue_inverses); x never leaves the host
//            device  row i = t_i (1, s_i, m_i ..) as canonical words                                     k_bbs_rows
//            device  A_i = <row_i, params>, normalised                                                    k_many_tree, k_many_fold (msm_many.hip.h many_rows_resident)
//   each     host    the GLV split of -e_i (an input: nothing of the device is waited for)
//            device  row i = (1, s_i, m_i ..), b_i = <row_i, params>                                      k_bbs_rows, k_many_tree, k_many_fold
//            device  d_i = -((-e_i) A_i + b_i) = e_i A_i - b_i: the kernel's negation of its result, free  k_g1_scale_quad
//            device  e(A_i, w) e(d_i, g2): lines of the two prepared points shared by every row, the products of every slice (i, i + m), the loop's tail, the
//                    final exponentiation compared with one                                                k_lines_from_prepared x 2, k_line_products, k_miller_tail, k_final_exp
//   batch    device  c_k = sum_i rho^i row_ik, rho^i, rho^i e_i                                           k_bbs_col_sums, k_col_finish
//            device  P1 = sum rho^i A_i, P2 = sum (rho^i e_i) A_i + sum (-c_k) H_k: two MSMs per chunk over the A_i, ONE over the parameters; the host adds the
//                    chunks' points
//            device  e(P1, w) e(P2, g2) against one, as above with one slice
// Proofs of knowledge of a signature (dgpu_bbs_plus_pok_verify_each_g1, dgpu_bbs_plus_pok_verify_batch_g1): PoKOfSignatureG1Proof::verify (bbs_plus/src/proof.rs:529-611)
// for many proofs under one key; the verifier sees no e, s or hidden message, so none of the above serves it.
//   pok each   device  row i = (c_i, z4_i, y_i ..), the own-point scalars (z1, z2, -c, c, -1 | z3, -1)         k_bbs_pok_rows, k_bbs_pok_own
//              device  the bases of the row's two segments, A' and -Abar for the pairing                          k_bbs_pok_stage
//              device  P_i = <row_i, params>                                                                      k_many_tree, k_many_fold
//              device  [A', h_0, Abar, d, T1] . (z1, z2, -c, c, -1) and z3 d - T2 per row                         k_small_table, k_seg_tree, k_seg_fold (seg_rows_resident)
//              device  e(A'_i, w) e(-Abar_i, g2), as above; the four checks into a status byte                    .., k_bbs_pok_verdict
//   pok batch  device  C_k, the weights over the own points, +-rho^i                                              k_bbs_pok_col_sums, k_col_finish
//              device  one MSM over the chunk's 5 n own points, one each over the A' and the Abar; ONE over the parameters; the host adds the chunks' points
//              device  e(sum rho^i A'_i, w) e(-sum rho^i Abar_i, g2) against one
// The 2023 scheme (dgpu_bbs23_*: bbs_plus/src/signature_23.rs, proof_23_cdl.rs, proof_23_ietf.rs): parameters [g1, h_1 .. h_L], no s, no h_0.
//   sign / each / batch   the three drivers above with ONE fixed column (Rows::fixed = 1): row i = mult_i (1, m_i ..), the same kernels
//   pok each   device  row i = (c_i, y_i ..), the own scalars (z1, z2, -c, -1 | z3, -1) (CDL) or (z_a, z_b, -1) (IETF)   k_bbs23_rows, k_bbs23_own
//              device  the bases [Abar, d, Bbar, T1 | d, T2] or [Abar, Bbar, T], Abar and -Bbar for the pairing             k_bbs23_stage
//              device  P_i, the segments, the pairing as above; the checks into a status byte                              .., k_bbs23_verdict
//   pok batch  device  C_k, the weights over the own points, +-rho^i                                                        k_bbs23_col_sums, k_col_finish
//              device  one MSM over the chunk's 5 n or 3 n own points, one each over the Abar and the Bbar; ONE over the parameters; the pairing as above
// Only verdict bytes (each, batch) or the signatures (sign) come back.  The device copies of the inverses and of the rows that carry them are zeroed on every return
// path before the slot is released, the host copy too.
#include "msm_many.hip.h"
#include "qap_launch.hip.h"
#include "fixed_launch.hip.h"
#include "pairing_launch.hip.h"
#include "gt_launch.hip.h"
#include "bbs_launch.hip.h"
#include "bbs_pok_launch.hip.h"
#include "bbs23_launch.hip.h"
#include "acc_host_tables.hpp"
#include "pair_check.hip.h"             // PT, row_layout, prep_g1, msm_add, params_msm, zero_words, ws_check, coeffs_up, launch_check, merged_pair_verdict: shared with the other bulk drivers
using namespace dock;
using namespace acch;
using namespace mlk;

namespace {

constexpr size_t NPTS = 5;                // points of a proof of knowledge: A', Abar, d, T1, T2

// what the three calls share: the rows' inputs and how they are cut.  fixed: the columns in front of the messages — 2 for BBS+ (1, s_i), parameters
// [g1, h_0, h ..]; 1 for the 2023 scheme (1), parameters [g1, h ..], s = NULL
struct Rows {
    const uint64_t *messages, *e, *s; size_t L, stride, n; bool mont; size_t fixed;
    size_t nn() const { return L + fixed; }
};
// the argument checks that come before the device is looked at (n > 0)
bool bad_rows(const Rows &r) {
    return r.L == 0 || !r.messages || !r.e || (r.fixed == 2 && !r.s) || r.stride < r.L || r.n >= (1ull << 31) || r.L >= (1ull << 31) - 2 || r.stride >= (1ull << 31);
}
// the parameters: a plain G1 bases handle of exactly nn = L + 2 (2023: L + 1) points, pinned for the call
bool params_ok(const HandleRef &hb, size_t nn) { return hb.ok && hb.h.kind == 1 && hb.h.n == nn; }

// (how the b_i, the P_i of a proof, of a chunk are made: param_rows<G1>, msm_many.hip.h)
// s (BBS+) and the messages of the rows [r0, r0 + rows) to the device: the messages packed (what lies between the caller's rows never crosses)
int32_t rows_up(Slot &sl, const Rows &r, size_t r0, size_t rows, void *d_s, void *d_m) {
    hipStream_t s = sl.stream;
    if (r.fixed == 2) HIPCHK(hipMemcpyAsync(d_s, r.s + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
    return upload_rows_packed(s, d_m, r.messages + r0 * r.stride * 4, r.L, r.stride, rows);
}

// ---- SignatureG1::new for n rows (signature.rs:138-211): A_i = (x + e_i)^-1 b_i with the caller's e_i, s_i -------------------------------------------------
int32_t sign_many(uint64_t params, const uint64_t *sk, const Rows &r, uint64_t *out_a, uint8_t *bad) {
    if (r.n == 0) return DGPU_OK;
    if (bad_rows(r) || !sk || !out_a || !bad) return DGPU_E_BADARG;
    const size_t n = r.n, nn = r.nn();
    SecretWords t;
    t.w.assign(n * 4, 0);
    std::vector<uint8_t> zero(n), binf(n);
    auto t0 = std::chrono::steady_clock::now();
    const size_t parts = std::min<size_t>(16, (n + 1023) / 1024);
    int32_t rc = par_run(parts, [&](size_t k) { return issue_inverses(r.e, n * k / parts, n * (k + 1) / parts, sk, r.mont, t.w.data(), zero.data()); });
    if (rc) return rc;
    if (!cur().ready) return DGPU_E_NODEVICE;
    if (gs.prof) prof_add_host("bbs.host_inverses", ms_since(t0));
    HandleRef hb(params);
    if (!params_ok(hb, nn)) return DGPU_E_BADARG;
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const RowMsm<G1> bp = param_rows<G1>(sl, params, hb.h, nn, ~(size_t)0, n);
    const size_t chunk = bp.chunk;
    // q[0]: t, q[1]: s, q[2]: the messages, q[4]: [A | identity flags]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure(chunk * 32))) return e;
        if ((e = o.q[1].ensure(chunk * 32))) return e;
        if ((e = o.q[2].ensure(chunk * r.L * 32))) return e;
        if ((e = o.q[4].ensure(chunk * PT + chunk))) return e;
        return bp.workspace(o);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    DeviceWipe dw(sl);
    dw.add(sl.q[0].p, chunk * 32); dw.add(sl.in_scalars.p, chunk * nn * 32);
    uint32_t *d_rows = sl.in_scalars.as<uint32_t>(), *d_bad = sl.flags.as<uint32_t>();
    uint8_t *dA = sl.q[4].as<uint8_t>(), *dAinf = dA + chunk * PT;
    HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                              // (rows are canonical: the flag stays clear)
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        HIPCHK(hipMemcpyAsync(sl.q[0].p, t.w.data() + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
        if ((rc = rows_up(sl, r, r0, rows, sl.q[1].p, sl.q[2].p))) return rc;
        { StageTimer st(sl, "bbs.rows"); bbsk::launch_bbs_rows(s, sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), sl.q[0].as<uint32_t>(), r.mont ? 1 : 0, rows, nn, r.fixed, d_rows); }
        if ((rc = bp.points(sl, d_rows, rows, d_bad, dA, dAinf))) return rc;
        HIPCHK(hipMemcpyAsync(out_a + 12 * r0, dA, rows * PT, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(binf.data() + r0, dAinf, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    // no signature: x + e_i = 0 (the reference draws e again there), or b_i — and with it A_i — the identity
    for (size_t i = 0; i < n; i++) {
        bad[i] = (zero[i] || binf[i]) ? 1 : 0;
        if (bad[i]) memset(out_a + 12 * i, 0, PT);
    }
    return DGPU_OK;
}

// (the pairing check of a chunk's rows — ws_check, coeffs_up, launch_check — is pair_check.hip.h's)

// (k1 | k2) of -e mod r: the scalar of the kernel that returns -((-e) A + b)
void neg_split(const uint64_t *e, bool mont, uint64_t *out) {
    uint64_t c[4];
    fr_in(e, mont).to_canonical(c);
    if (c[0] | c[1] | c[2] | c[3]) {
        uint64_t br = 0;
        for (int i = 0; i < 4; i++) { u128 d = (u128)FrH::MOD[i] - c[i] - br; c[i] = (uint64_t)d; br = (uint64_t)(d >> 64) & 1; }
    }
    hostf::glv_decompose(c, out, out + 2);
}

// ---- SignatureG1::verify for n rows (signature.rs:272-296), a verdict per row --------------------------------------------------------------------------------------
int32_t verify_each(uint64_t params, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a, const Rows &r, uint8_t *ok) {
    if (r.n == 0) return DGPU_OK;
    if (bad_rows(r) || !pk_pc || !g2_pc || !sig_a || !ok) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = r.n, nn = r.nn();
    HandleRef hb(params);
    if (!params_ok(hb, nn)) return DGPU_E_BADARG;
    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> split(n * 4);
    std::vector<uint8_t> ainf(n);
    const size_t parts = std::min<size_t>(16, (n + 4095) / 4096);
    int32_t rc = par_run(parts, [&](size_t k) {
        for (size_t i = n * k / parts; i < n * (k + 1) / parts; i++) { neg_split(r.e + 4 * i, r.mont, &split[4 * i]); ainf[i] = zero_words(sig_a + 12 * i, 12) ? 1 : 0; }
        return (int32_t)DGPU_OK;
    });
    if (rc) return rc;
    if (gs.prof) prof_add_host("bbs.glv_split", ms_since(t0));
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const RowMsm<G1> bp = param_rows<G1>(sl, params, hb.h, nn, bbsk::BBS_EACH_CHUNK, n);
    const size_t chunk = bp.chunk;
    // q[0]: the split -e, q[1]: s, q[2]: the messages, q[3]: A, q[4]: [b | identity flags], q[5]: d, q[6]: [skip flags of (A, d) | ones]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure(chunk * 32))) return e;
        if ((e = o.q[1].ensure(chunk * 32))) return e;
        if ((e = o.q[2].ensure(chunk * r.L * 32))) return e;
        if ((e = o.q[3].ensure(chunk * PT))) return e;
        if ((e = o.q[4].ensure(chunk * PT + chunk))) return e;
        if ((e = o.q[5].ensure(chunk * PT))) return e;
        if ((e = o.q[6].ensure(3 * chunk))) return e;
        if ((e = ws_check(o, chunk))) return e;
        return bp.workspace(o);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_rows = sl.in_scalars.as<uint32_t>(), *d_bad = sl.flags.as<uint32_t>();
    uint8_t *dA = sl.q[3].as<uint8_t>(), *dB = sl.q[4].as<uint8_t>(), *dBinf = dB + chunk * PT, *dD = sl.q[5].as<uint8_t>(), *dsk = sl.q[6].as<uint8_t>(), *dones = dsk + 2 * chunk;
    HIPCHK(hipMemsetAsync(dones, 1, chunk, s));
    if ((rc = coeffs_up(sl, pk_pc, g2_pc, chunk))) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                          // (rows are canonical: the flag stays clear; sl.flags takes the verdicts afterwards)
        HIPCHK(hipMemcpyAsync(sl.q[0].p, &split[4 * r0], rows * 32, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dA, sig_a + 12 * r0, rows * PT, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dsk, ainf.data() + r0, rows, hipMemcpyHostToDevice, s));
        if ((rc = rows_up(sl, r, r0, rows, sl.q[1].p, sl.q[2].p))) return rc;
        { StageTimer st(sl, "bbs.rows"); bbsk::launch_bbs_rows(s, sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), nullptr, r.mont ? 1 : 0, rows, nn, r.fixed, d_rows); }
        if ((rc = bp.points(sl, d_rows, rows, d_bad, dB, dBinf))) return rc;
        // d_i = -((-e_i) A_i + b_i); its identity flag is the second pair's skip flag
        { StageTimer st(sl, "bbs.scale");
          msm::launch_g1_scale_quad(s, (const uint32_t *)dA, dsk, sl.q[0].as<uint32_t>(), 8, dones, rows, (uint32_t *)dD, dsk + rows, (const uint32_t *)dB, dBinf); }
        launch_check(sl, (const uint32_t *)dA, (const uint32_t *)dD, dsk, rows, chunk);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ok + r0, sl.flags.p, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    for (size_t i = 0; i < n; i++) if (ainf[i]) ok[i] = 0;               // ZeroSignature (signature.rs:280-282)
    return DGPU_OK;
}

// ---- one verdict for n rows: the random linear combination RandomizedPairingChecker forms (utils/src/randomized_pairing_check.rs), merged before the pairing
// (HPoint, add_jac and merged_pair_verdict: pair_check.hip.h) ----------
// rows per chunk of the batch calls: their kernels' cap and BBS_BATCH_TERMS scalars (dgpu_set_many_chunk_rows of the development surface cuts these calls' rows too)
size_t batch_chunk(size_t n, size_t L, size_t cap) {
    const int forced = gs.many_chunk.load();
    return std::min(n, forced > 0 ? (size_t)forced : std::min(cap, std::max<size_t>(1, bbsk::BBS_BATCH_TERMS / L)));
}
int32_t verify_batch(uint64_t params, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a, const Rows &r, const uint64_t *random, int32_t *ok) {
    if (r.n == 0) { if (ok) *ok = 1; return DGPU_OK; }
    if (bad_rows(r) || !pk_pc || !g2_pc || !sig_a || !random || !ok) return DGPU_E_BADARG;
    if (fr_is_zero(fr_in(random, r.mont))) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = r.n, nn = r.nn();
    HandleRef hb(params);
    if (!params_ok(hb, nn)) return DGPU_E_BADARG;
    for (size_t i = 0; i < n; i++) if (zero_words(sig_a + 12 * i, 12)) { *ok = 0; return DGPU_OK; }      // ZeroSignature
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = batch_chunk(n, r.L, bbsk::BBS_BATCH_CHUNK);
    const RawBases rb = RawBases::packed<G1>(sig_a, nullptr);
    int32_t rc;
    // q[0]: e, q[1]: s, q[2]: the messages, q[3]: [P1 | P2] and their skip flags, q[7]: the blocks' partial sums, q[8]: [-c | the running sums], q[9]: [rho^i | rho^i e_i],
    // q[10]: the prepared records of the A_i
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure(chunk * 32))) return e;
        if ((e = o.q[1].ensure(chunk * 32))) return e;
        if ((e = o.q[2].ensure(chunk * r.L * 32))) return e;
        if ((e = o.q[3].ensure(2 * PT + 64))) return e;
        if ((e = o.q[7].ensure(colk::col_part_words(chunk, nn) * 4))) return e;
        if ((e = o.q[8].ensure(nn * 40 + nn * 32 + 64))) return e;
        if ((e = o.q[9].ensure(2 * chunk * 32))) return e;
        if ((e = o.q[10].ensure(chunk * G1::AFF_STRIDE * 4))) return e;
        if ((e = ws_stage_bases<G1>(o, rb, chunk))) return e;
        if ((e = ws_for<G1>(o, 2, std::max(chunk, nn), 0, nullptr))) return e;
        if (chunk != nn && (e = ws_for<G1>(o, 2, std::min(chunk, nn), 0, nullptr))) return e;
        return ws_check(o, 1);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_c = sl.q[8].as<uint32_t>(), *d_run = d_c + nn * 8, *d_w = sl.q[9].as<uint32_t>(), *d_we = d_w + chunk * 8, *d_rec = sl.q[10].as<uint32_t>();
    HPoint P1 = HPoint::identity(), P2 = HPoint::identity();
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        HIPCHK(hipMemcpyAsync(sl.q[0].p, r.e + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
        if ((rc = rows_up(sl, r, r0, rows, sl.q[1].p, sl.q[2].p))) return rc;
        if ((rc = stage_bases<G1>(sl, rb.from(r0), rows, d_rec))) return rc;
        { StageTimer st(sl, "bbs.columns");
          bbsk::launch_bbs_columns(s, sl.q[0].as<uint32_t>(), sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), (const uint32_t *)random, r.mont ? 1 : 0, rows, nn, r.fixed, r0, r0 == 0,
                                   sl.q[7].as<uint32_t>(), d_run, d_w, d_we, d_c); }
        HIPCHK(hipGetLastError());
        if ((rc = msm_add(sl, d_rec, d_w, rows, P1))) return rc;
        if ((rc = msm_add(sl, d_rec, d_we, rows, P2))) return rc;
        if (gs.prof) prof_flush(sl);
    }
    if ((rc = params_msm(sl, params, hb.h, d_c, nn, P2))) return rc;       // - sum_k c_k H_k
    if ((rc = merged_pair_verdict(sl, P1, P2, pk_pc, g2_pc, sl.q[3], ok))) return rc;
    guard.done = true;
    return DGPU_OK;
}

// ---- PoKOfSignatureG1Proof::verify for n proofs (proof.rs:529-611) -------------------------------------------------------------------------------------------------
struct Proofs {
    const uint64_t *h0, *points, *fixed, *values; const uint8_t *revealed; const uint64_t *challenge; size_t L, stride, n; bool mont;
    size_t nn() const { return L + 2; }
};
bool bad_proofs(const Proofs &p) {
    return p.L == 0 || !p.h0 || !p.points || !p.fixed || !p.values || !p.revealed || !p.challenge || p.stride < p.L || p.n >= (1ull << 31) || p.L >= (1ull << 31) - 2 ||
           p.stride >= (1ull << 31);
}
// q[0]: the challenges, q[1]: z1 .. z4, q[2]: the values, q[3]: the mask, q[5]: the points of the rows [r0, r0 + rows); the values packed
int32_t ws_proofs(Slot &o, const Proofs &p, size_t chunk) {
    int32_t e;
    if ((e = o.q[0].ensure(chunk * 32))) return e;
    if ((e = o.q[1].ensure(chunk * 4 * 32))) return e;
    if ((e = o.q[2].ensure(chunk * p.L * 32))) return e;
    if ((e = o.q[3].ensure(chunk * p.L))) return e;
    return o.q[5].ensure(chunk * NPTS * PT);
}
int32_t proofs_up(Slot &sl, const Proofs &p, size_t r0, size_t rows, bbspk::PokDev &dev) {
    hipStream_t s = sl.stream;
    HIPCHK(hipMemcpyAsync(sl.q[0].p, p.challenge + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[1].p, p.fixed + 16 * r0, rows * 4 * 32, hipMemcpyHostToDevice, s));
    int32_t rc;
    if ((rc = upload_rows_packed(s, sl.q[2].p, p.values + r0 * p.stride * 4, p.L, p.stride, rows))) return rc;
    HIPCHK(hipMemcpyAsync(sl.q[3].p, p.revealed + r0 * p.L, rows * p.L, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[5].p, p.points + r0 * NPTS * 12, rows * NPTS * PT, hipMemcpyHostToDevice, s));
    dev = bbspk::PokDev{sl.q[0].as<uint32_t>(), sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), sl.q[3].as<uint8_t>(), p.L, p.mont ? 1 : 0};
    return DGPU_OK;
}

int32_t pok_verify_each(uint64_t params, const uint64_t *pk_pc, const uint64_t *g2_pc, const Proofs &p, uint8_t *status) {
    if (p.n == 0) return DGPU_OK;
    if (bad_proofs(p) || !pk_pc || !g2_pc || !status) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n, nn = p.nn();
    HandleRef hb(params);
    if (!params_ok(hb, nn)) return DGPU_E_BADARG;
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const RowMsm<G1> bp = param_rows<G1>(sl, params, hb.h, nn, bbspk::POK_EACH_CHUNK, n);
    const size_t chunk = bp.chunk;
    int32_t rc;
    SegLayout lay, lay_tail;
    row_layout(chunk, 7, 5, lay);                                        // the two segments of every row, 5 and 2 terms
    if (n % chunk) row_layout(n % chunk, 7, 5, lay_tail);
    // q[0 .. 3], q[5]: the proofs (ws_proofs); q[4]: [P | identity flags], q[6]: the own-point scalars, q[7]: the own points in segment order, q[8]: [A' | -Abar],
    // q[9]: [skip flags of (A', -Abar) | status]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, p, chunk))) return e;
        if ((e = o.q[4].ensure(chunk * PT + chunk))) return e;
        if ((e = o.q[6].ensure(chunk * 7 * 32))) return e;
        if ((e = o.q[7].ensure(chunk * 7 * PT))) return e;
        if ((e = o.q[8].ensure(2 * chunk * PT))) return e;
        if ((e = o.q[9].ensure(3 * chunk))) return e;
        if ((e = ws_check(o, chunk))) return e;
        if ((e = ws_seg_resident<G1>(o, 7 * chunk, 2 * chunk, lay.blocks))) return e;
        return bp.workspace(o);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_rows = sl.in_scalars.as<uint32_t>(), *d_bad = sl.flags.as<uint32_t>(), *d_own = sl.q[6].as<uint32_t>(), *d_opts = sl.q[7].as<uint32_t>();
    uint32_t *dPa = sl.q[8].as<uint32_t>(), *dPb = dPa + chunk * (PT / 4);
    uint8_t *dB = sl.q[4].as<uint8_t>(), *dBinf = dB + chunk * PT, *dsk = sl.q[9].as<uint8_t>(), *dstatus = dsk + 2 * chunk;
    if ((rc = coeffs_up(sl, pk_pc, g2_pc, chunk))) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        bbspk::PokDev dev;
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                          // (rows are canonical: the flag stays clear; sl.flags takes the pairing's verdicts afterwards)
        if ((rc = proofs_up(sl, p, r0, rows, dev))) return rc;
        { StageTimer st(sl, "bbs.pok_rows"); bbspk::launch_pok_rows(s, dev, rows, d_rows, d_own); }
        { StageTimer st(sl, "bbs.pok_stage"); bbspk::launch_pok_stage(s, sl.q[5].as<uint32_t>(), (const uint32_t *)p.h0, rows, d_opts, dPa, dPb, dsk); }
        if ((rc = bp.points(sl, d_rows, rows, d_bad, dB, dBinf))) return rc;
        if ((rc = seg_rows_resident<G1>(sl, (const uint8_t *)d_opts, PT, d_own, 7 * rows, 2 * rows, rows == chunk ? lay : lay_tail, d_bad))) return rc;
        launch_check(sl, dPa, dPb, dsk, rows, chunk);
        { StageTimer st(sl, "bbs.pok_verdict");
          bbspk::launch_pok_verdict(s, sl.win.as<uint32_t>(), sl.win_inf.as<uint8_t>(), (const uint32_t *)dB, dBinf, sl.flags.as<uint8_t>(), dsk, rows, dstatus); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(status + r0, dstatus, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    return DGPU_OK;
}

// one verdict for n proofs: row i weighs its first Schnorr check with u_i = rho^(2 i), its second with v_i = rho^(2 i + 1), its pairing with t_i = rho^i
int32_t pok_verify_batch(uint64_t params, const uint64_t *pk_pc, const uint64_t *g2_pc, const Proofs &p, const uint64_t *random, int32_t *ok) {
    if (p.n == 0) { if (ok) *ok = 1; return DGPU_OK; }
    if (bad_proofs(p) || !pk_pc || !g2_pc || !random || !ok) return DGPU_E_BADARG;
    if (fr_is_zero(fr_in(random, p.mont))) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n, nn = p.nn();
    HandleRef hb(params);
    if (!params_ok(hb, nn)) return DGPU_E_BADARG;
    for (size_t i = 0; i < n; i++) if (zero_words(p.points + NPTS * 12 * i, 12)) { *ok = 0; return DGPU_OK; }      // ZeroSignature
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = batch_chunk(n, p.L, bbspk::POK_BATCH_CHUNK);
    int32_t rc;
    // q[0 .. 3], q[5]: the proofs (ws_proofs); q[4]: [P1 | P2] and their skip flags, q[6]: the weights over the own points, q[7]: the blocks' partial sums,
    // q[8]: [C | the running sums], q[9]: [rho^i | -rho^i], q[10]: the prepared records of the own points, q[11]: those of [the A' | the Abar]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, p, chunk))) return e;
        if ((e = o.q[4].ensure(2 * PT + 64))) return e;
        if ((e = o.q[6].ensure(chunk * NPTS * 32))) return e;
        if ((e = o.q[7].ensure(colk::col_part_words(chunk, nn) * 4))) return e;
        if ((e = o.q[8].ensure(nn * 40 + nn * 32 + 64))) return e;
        if ((e = o.q[9].ensure(2 * chunk * 32))) return e;
        if ((e = o.q[10].ensure(chunk * NPTS * G1::AFF_STRIDE * 4))) return e;
        if ((e = o.q[11].ensure(2 * chunk * G1::AFF_STRIDE * 4))) return e;
        for (size_t terms : {NPTS * chunk, chunk, nn}) if ((e = ws_for<G1>(o, 2, terms, 0, nullptr))) return e;
        return ws_check(o, 1);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_c = sl.q[8].as<uint32_t>(), *d_run = d_c + nn * 8, *d_w5 = sl.q[6].as<uint32_t>(), *d_tp = sl.q[9].as<uint32_t>(), *d_tn = d_tp + chunk * 8;
    uint32_t *d_rec = sl.q[10].as<uint32_t>(), *d_reca = sl.q[11].as<uint32_t>(), *d_recb = d_reca + chunk * G1::AFF_STRIDE;
    HPoint Gsum = HPoint::identity(), P1 = HPoint::identity(), P2 = HPoint::identity();
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        bbspk::PokDev dev;
        if ((rc = proofs_up(sl, p, r0, rows, dev))) return rc;
        const uint8_t *raw = sl.q[5].as<uint8_t>();
        { StageTimer st(sl, "msm.prep_bases");
          prep_g1(s, raw, PT, NPTS * rows, d_rec);
          prep_g1(s, raw, NPTS * PT, rows, d_reca);
          prep_g1(s, raw + PT, NPTS * PT, rows, d_recb); }
        { StageTimer st(sl, "bbs.pok_columns");
          bbspk::launch_pok_columns(s, dev, (const uint32_t *)random, rows, r0, r0 == 0, sl.q[7].as<uint32_t>(), d_run, d_w5, d_tp, d_tn, d_c); }
        HIPCHK(hipGetLastError());
        if ((rc = msm_add(sl, d_rec, d_w5, NPTS * rows, Gsum))) return rc;
        if ((rc = msm_add(sl, d_reca, d_tp, rows, P1))) return rc;
        if ((rc = msm_add(sl, d_recb, d_tn, rows, P2))) return rc;
        if (gs.prof) prof_flush(sl);
    }
    if ((rc = params_msm(sl, params, hb.h, d_c, nn, Gsum))) return rc;     // sum_k C_k H_k
    if (!Gsum.inf) { HIPCHK(hipStreamSynchronize(s)); guard.done = true; *ok = 0; return DGPU_OK; }      // the G1 equation fails: the pairing cannot mend it
    if ((rc = merged_pair_verdict(sl, P1, P2, pk_pc, g2_pc, sl.q[4], ok))) return rc;
    guard.done = true;
    return DGPU_OK;
}

// ---- the 2023 scheme's two PoKOfSignature23G1Proof::verify for n proofs (proof_23_cdl.rs:302-549, proof_23_ietf.rs:244-479) ---------------------------------------------
// The signature calls of that scheme are sign_many / verify_each / verify_batch above with Rows::fixed = 1.  KIND: bbs23k::KIND_CDL / KIND_IETF
struct Proofs23 {
    const uint64_t *points, *fixed, *values; const uint8_t *revealed; const uint64_t *challenge; size_t L, stride, n; bool mont;
    size_t nn() const { return L + 1; }
};
bool bad_proofs23(const Proofs23 &p) {
    return p.L == 0 || !p.points || !p.fixed || !p.values || !p.revealed || !p.challenge || p.stride < p.L || p.n >= (1ull << 31) || p.L >= (1ull << 31) - 2 ||
           p.stride >= (1ull << 31);
}
// q[0]: the challenges, q[1]: the fixed responses, q[2]: the values, q[3]: the mask, q[5]: the points of the rows [r0, r0 + rows); the values packed
int32_t ws_proofs23(Slot &o, const Proofs23 &p, const bbs23k::KindShape &ks, size_t chunk) {
    int32_t e;
    if ((e = o.q[0].ensure(chunk * 32))) return e;
    if ((e = o.q[1].ensure(chunk * ks.resp * 32))) return e;
    if ((e = o.q[2].ensure(chunk * p.L * 32))) return e;
    if ((e = o.q[3].ensure(chunk * p.L))) return e;
    return o.q[5].ensure(chunk * ks.pts * PT);
}
int32_t proofs23_up(Slot &sl, const Proofs23 &p, int kind, const bbs23k::KindShape &ks, size_t r0, size_t rows, bbs23k::ProofDev &dev) {
    hipStream_t s = sl.stream;
    HIPCHK(hipMemcpyAsync(sl.q[0].p, p.challenge + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[1].p, p.fixed + 4 * ks.resp * r0, rows * ks.resp * 32, hipMemcpyHostToDevice, s));
    int32_t rc;
    if ((rc = upload_rows_packed(s, sl.q[2].p, p.values + r0 * p.stride * 4, p.L, p.stride, rows))) return rc;
    HIPCHK(hipMemcpyAsync(sl.q[3].p, p.revealed + r0 * p.L, rows * p.L, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[5].p, p.points + r0 * ks.pts * 12, rows * ks.pts * PT, hipMemcpyHostToDevice, s));
    dev = bbs23k::ProofDev{sl.q[0].as<uint32_t>(), sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), sl.q[3].as<uint8_t>(), p.L, kind, p.mont ? 1 : 0};
    return DGPU_OK;
}
// the segments of every row of a chunk — CDL: 4 and 2 terms, IETF: 3
void own_layout23(const bbs23k::KindShape &ks, size_t rows, SegLayout &lay) { row_layout(rows, (size_t)ks.own, ks.segs == 2 ? 4 : 0, lay); }

int32_t pok23_verify_each(int kind, uint64_t params, const uint64_t *pk_pc, const uint64_t *g2_pc, const Proofs23 &p, uint8_t *status) {
    if (p.n == 0) return DGPU_OK;
    if (bad_proofs23(p) || !pk_pc || !g2_pc || !status) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n, nn = p.nn();
    HandleRef hb(params);
    if (!params_ok(hb, nn)) return DGPU_E_BADARG;
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const bbs23k::KindShape ks = bbs23k::kind_shape(kind);
    const size_t own = ks.own, segs = ks.segs;
    const RowMsm<G1> bp = param_rows<G1>(sl, params, hb.h, nn, bbs23k::BBS23_EACH_CHUNK, n);
    const size_t chunk = bp.chunk;
    int32_t rc;
    SegLayout lay, lay_tail;
    own_layout23(ks, chunk, lay);
    if (n % chunk) own_layout23(ks, n % chunk, lay_tail);
    // q[0 .. 3], q[5]: the proofs (ws_proofs23); q[4]: [P | identity flags], q[6]: the own scalars, q[7]: the own points in segment order, q[8]: [Abar | -Bbar],
    // q[9]: [skip flags of (Abar, -Bbar) | status]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs23(o, p, ks, chunk))) return e;
        if ((e = o.q[4].ensure(chunk * PT + chunk))) return e;
        if ((e = o.q[6].ensure(chunk * own * 32))) return e;
        if ((e = o.q[7].ensure(chunk * own * PT))) return e;
        if ((e = o.q[8].ensure(2 * chunk * PT))) return e;
        if ((e = o.q[9].ensure(3 * chunk))) return e;
        if ((e = ws_check(o, chunk))) return e;
        if ((e = ws_seg_resident<G1>(o, own * chunk, segs * chunk, lay.blocks))) return e;
        return bp.workspace(o);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_rows = sl.in_scalars.as<uint32_t>(), *d_bad = sl.flags.as<uint32_t>(), *d_own = sl.q[6].as<uint32_t>(), *d_opts = sl.q[7].as<uint32_t>();
    uint32_t *dPa = sl.q[8].as<uint32_t>(), *dPb = dPa + chunk * (PT / 4);
    uint8_t *dB = sl.q[4].as<uint8_t>(), *dBinf = dB + chunk * PT, *dsk = sl.q[9].as<uint8_t>(), *dstatus = dsk + 2 * chunk;
    if ((rc = coeffs_up(sl, pk_pc, g2_pc, chunk))) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        bbs23k::ProofDev dev;
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                          // (rows are canonical: the flag stays clear; sl.flags takes the pairing's verdicts afterwards)
        if ((rc = proofs23_up(sl, p, kind, ks, r0, rows, dev))) return rc;
        { StageTimer st(sl, "bbs23.pok_rows"); bbs23k::launch_bbs23_rows(s, dev, rows, d_rows, d_own); }
        { StageTimer st(sl, "bbs23.pok_stage"); bbs23k::launch_bbs23_stage(s, sl.q[5].as<uint32_t>(), kind, rows, d_opts, dPa, dPb, dsk); }
        if ((rc = bp.points(sl, d_rows, rows, d_bad, dB, dBinf))) return rc;
        if ((rc = seg_rows_resident<G1>(sl, (const uint8_t *)d_opts, PT, d_own, own * rows, segs * rows, rows == chunk ? lay : lay_tail, d_bad))) return rc;
        launch_check(sl, dPa, dPb, dsk, rows, chunk);
        { StageTimer st(sl, "bbs23.pok_verdict");
          bbs23k::launch_bbs23_verdict(s, sl.win.as<uint32_t>(), sl.win_inf.as<uint8_t>(), (const uint32_t *)dB, dBinf, sl.flags.as<uint8_t>(), dsk, kind, rows, dstatus); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(status + r0, dstatus, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    return DGPU_OK;
}

// one verdict for n proofs — CDL: row i weighs its first Schnorr check with u_i = rho^(2 i), its second with v_i = rho^(2 i + 1), its pairing with t_i = rho^i;
// IETF: its one Schnorr check and its pairing with rho^i
int32_t pok23_verify_batch(int kind, uint64_t params, const uint64_t *pk_pc, const uint64_t *g2_pc, const Proofs23 &p, const uint64_t *random, int32_t *ok) {
    if (p.n == 0) { if (ok) *ok = 1; return DGPU_OK; }
    if (bad_proofs23(p) || !pk_pc || !g2_pc || !random || !ok) return DGPU_E_BADARG;
    if (fr_is_zero(fr_in(random, p.mont))) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n, nn = p.nn();
    HandleRef hb(params);
    if (!params_ok(hb, nn)) return DGPU_E_BADARG;
    const bbs23k::KindShape ks = bbs23k::kind_shape(kind);
    const size_t npts = ks.pts;
    for (size_t i = 0; i < n; i++) if (zero_words(p.points + npts * 12 * i, 12)) { *ok = 0; return DGPU_OK; }      // ZeroSignature
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = batch_chunk(n, p.L, bbs23k::BBS23_BATCH_CHUNK);
    int32_t rc;
    // q[0 .. 3], q[5]: the proofs (ws_proofs23); q[4]: [P1 | P2] and their skip flags, q[6]: the weights over the own points, q[7]: the blocks' partial sums,
    // q[8]: [C | the running sums], q[9]: [rho^i | -rho^i], q[10]: the prepared records of the own points, q[11]: those of [the Abar | the Bbar]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs23(o, p, ks, chunk))) return e;
        if ((e = o.q[4].ensure(2 * PT + 64))) return e;
        if ((e = o.q[6].ensure(chunk * npts * 32))) return e;
        if ((e = o.q[7].ensure(colk::col_part_words(chunk, nn) * 4))) return e;
        if ((e = o.q[8].ensure(nn * 40 + nn * 32 + 64))) return e;
        if ((e = o.q[9].ensure(2 * chunk * 32))) return e;
        if ((e = o.q[10].ensure(chunk * npts * G1::AFF_STRIDE * 4))) return e;
        if ((e = o.q[11].ensure(2 * chunk * G1::AFF_STRIDE * 4))) return e;
        for (size_t terms : {npts * chunk, chunk, nn}) if ((e = ws_for<G1>(o, 2, terms, 0, nullptr))) return e;
        return ws_check(o, 1);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_c = sl.q[8].as<uint32_t>(), *d_run = d_c + nn * 8, *d_wts = sl.q[6].as<uint32_t>(), *d_tp = sl.q[9].as<uint32_t>(), *d_tn = d_tp + chunk * 8;
    uint32_t *d_rec = sl.q[10].as<uint32_t>(), *d_reca = sl.q[11].as<uint32_t>(), *d_recb = d_reca + chunk * G1::AFF_STRIDE;
    HPoint Gsum = HPoint::identity(), P1 = HPoint::identity(), P2 = HPoint::identity();
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        bbs23k::ProofDev dev;
        if ((rc = proofs23_up(sl, p, kind, ks, r0, rows, dev))) return rc;
        const uint8_t *raw = sl.q[5].as<uint8_t>();
        { StageTimer st(sl, "msm.prep_bases");
          prep_g1(s, raw, PT, npts * rows, d_rec);
          prep_g1(s, raw, npts * PT, rows, d_reca);
          prep_g1(s, raw + PT, npts * PT, rows, d_recb); }
        { StageTimer st(sl, "bbs23.pok_columns");
          bbs23k::launch_bbs23_columns(s, dev, (const uint32_t *)random, rows, r0, r0 == 0, sl.q[7].as<uint32_t>(), d_run, d_wts, d_tp, d_tn, d_c); }
        HIPCHK(hipGetLastError());
        if ((rc = msm_add(sl, d_rec, d_wts, npts * rows, Gsum))) return rc;
        if ((rc = msm_add(sl, d_reca, d_tp, rows, P1))) return rc;
        if ((rc = msm_add(sl, d_recb, d_tn, rows, P2))) return rc;
        if (gs.prof) prof_flush(sl);
    }
    if ((rc = params_msm(sl, params, hb.h, d_c, nn, Gsum))) return rc;     // sum_k C_k H_k
    if (!Gsum.inf) { HIPCHK(hipStreamSynchronize(s)); guard.done = true; *ok = 0; return DGPU_OK; }      // the G1 equation fails: the pairing cannot mend it
    if ((rc = merged_pair_verdict(sl, P1, P2, pk_pc, g2_pc, sl.q[4], ok))) return rc;
    guard.done = true;
    return DGPU_OK;
}

}  // namespace

extern "C" {
int32_t dgpu_bbs23_sign_many_g1(uint64_t params, size_t L, const uint64_t sk[4], const uint64_t *messages, size_t row_stride, const uint64_t *e, size_t n, int32_t montgomery,
                                uint64_t *out_a, uint8_t *bad) {
    return abi_guard([&] { return sign_many(params, sk, Rows{messages, e, nullptr, L, row_stride, n, montgomery != 0, 1}, out_a, bad); });
}
int32_t dgpu_bbs23_verify_each_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a, const uint64_t *e, const uint64_t *messages,
                                  size_t row_stride, size_t n, int32_t montgomery, uint8_t *ok) {
    return abi_guard([&] { return verify_each(params, pk_pc, g2_pc, sig_a, Rows{messages, e, nullptr, L, row_stride, n, montgomery != 0, 1}, ok); });
}
int32_t dgpu_bbs23_verify_batch_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a, const uint64_t *e, const uint64_t *messages,
                                   size_t row_stride, size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] { return verify_batch(params, pk_pc, g2_pc, sig_a, Rows{messages, e, nullptr, L, row_stride, n, montgomery != 0, 1}, random, ok); });
}
int32_t dgpu_bbs23_pok_verify_each_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points, const uint64_t *resp_fixed,
                                      const uint64_t *values, size_t row_stride, const uint8_t *revealed, const uint64_t *challenge, size_t n, int32_t montgomery, uint8_t *status) {
    return abi_guard([&] {
        return pok23_verify_each(bbs23k::KIND_CDL, params, pk_pc, g2_pc, Proofs23{points, resp_fixed, values, revealed, challenge, L, row_stride, n, montgomery != 0}, status);
    });
}
int32_t dgpu_bbs23_pok_verify_batch_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points, const uint64_t *resp_fixed,
                                       const uint64_t *values, size_t row_stride, const uint8_t *revealed, const uint64_t *challenge, size_t n, int32_t montgomery,
                                       const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] {
        return pok23_verify_batch(bbs23k::KIND_CDL, params, pk_pc, g2_pc, Proofs23{points, resp_fixed, values, revealed, challenge, L, row_stride, n, montgomery != 0}, random, ok);
    });
}
int32_t dgpu_bbs23_pok_ietf_verify_each_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points, const uint64_t *resp_fixed,
                                           const uint64_t *values, size_t row_stride, const uint8_t *revealed, const uint64_t *challenge, size_t n, int32_t montgomery,
                                           uint8_t *status) {
    return abi_guard([&] {
        return pok23_verify_each(bbs23k::KIND_IETF, params, pk_pc, g2_pc, Proofs23{points, resp_fixed, values, revealed, challenge, L, row_stride, n, montgomery != 0}, status);
    });
}
int32_t dgpu_bbs23_pok_ietf_verify_batch_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points, const uint64_t *resp_fixed,
                                            const uint64_t *values, size_t row_stride, const uint8_t *revealed, const uint64_t *challenge, size_t n, int32_t montgomery,
                                            const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] {
        return pok23_verify_batch(bbs23k::KIND_IETF, params, pk_pc, g2_pc, Proofs23{points, resp_fixed, values, revealed, challenge, L, row_stride, n, montgomery != 0}, random, ok);
    });
}
int32_t dgpu_bbs_plus_sign_many_g1(uint64_t params, size_t L, const uint64_t sk[4], const uint64_t *messages, size_t row_stride, const uint64_t *e, const uint64_t *s, size_t n,
                                   int32_t montgomery, uint64_t *out_a, uint8_t *bad) {
    return abi_guard([&] { return sign_many(params, sk, Rows{messages, e, s, L, row_stride, n, montgomery != 0, 2}, out_a, bad); });
}
int32_t dgpu_bbs_plus_verify_each_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a, const uint64_t *e, const uint64_t *s,
                                     const uint64_t *messages, size_t row_stride, size_t n, int32_t montgomery, uint8_t *ok) {
    return abi_guard([&] { return verify_each(params, pk_pc, g2_pc, sig_a, Rows{messages, e, s, L, row_stride, n, montgomery != 0, 2}, ok); });
}
int32_t dgpu_bbs_plus_verify_batch_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a, const uint64_t *e, const uint64_t *s,
                                      const uint64_t *messages, size_t row_stride, size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] { return verify_batch(params, pk_pc, g2_pc, sig_a, Rows{messages, e, s, L, row_stride, n, montgomery != 0, 2}, random, ok); });
}
int32_t dgpu_bbs_plus_pok_verify_each_g1(uint64_t params, size_t L, const uint64_t h_0[12], const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points,
                                         const uint64_t *resp_fixed, const uint64_t *values, size_t row_stride, const uint8_t *revealed, const uint64_t *challenge, size_t n,
                                         int32_t montgomery, uint8_t *status) {
    return abi_guard([&] { return pok_verify_each(params, pk_pc, g2_pc, Proofs{h_0, points, resp_fixed, values, revealed, challenge, L, row_stride, n, montgomery != 0}, status); });
}
int32_t dgpu_bbs_plus_pok_verify_batch_g1(uint64_t params, size_t L, const uint64_t h_0[12], const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points,
                                          const uint64_t *resp_fixed, const uint64_t *values, size_t row_stride, const uint8_t *revealed, const uint64_t *challenge, size_t n,
                                          int32_t montgomery, const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] {
        return pok_verify_batch(params, pk_pc, g2_pc, Proofs{h_0, points, resp_fixed, values, revealed, challenge, L, row_stride, n, montgomery != 0}, random, ok);
    });
}
}  // extern "C"
