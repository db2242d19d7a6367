// crypto_amd/csrc/dock_ps.hip — Pointcheval-Sanders (Coconut) signatures in bulk (include/dock_gpu.h: dgpu_ps_sign_many_g1, dgpu_ps_verify_each,
// dgpu_ps_verify_batch, dgpu_ps_pok_verify_each): Signature::new and Signature::verify (coconut/src/signature/ps_signature.rs:46-64, 95-142) and
// SignaturePoK::verify (coconut/src/proof/signature_pok/proof.rs:32-56) for many rows under one key, each call ONE device pipeline per chunk of rows.  The public
// key is a plain G2 bases handle [alpha_tilde, beta_tilde_1 .. beta_tilde_L, g_tilde]: this protocol's verification lives in G2.
//   sign     device  r_i and u_i = r_i (x + sum_j y_j m_ij)                                                       k_ps_sign_rows
//            device  (sigma_1_i, sigma_2_i) = (r_i g, u_i g) over g's window table                                 k_fb_mul (dock_fixed.hip table_mul_device)
//   each     device  row i = (1, m_i ..), Q_i = <row_i, pk[0 .. L]> in G2, normalised                             k_bbs_rows (one fixed column), k_many_tree, k_many_fold
//            device  e(sigma_1_i, Q_i) e(-sigma_2_i, g_tilde): the fused prepare + line kernel on the first side, the lines of the prepared g_tilde shared by every
//                    row on the second, the products of every slice (i, i + m), the loop's tail, the final exponentiation compared with one
//                                                                                                                 pair_check.hip.h launch_check (affine first side)
//   batch    device  w_i = rho^i, w_i m_ij, -w_i column-major                                                     k_ps_col_scalars
//            device  L + 1 MSMs per chunk over the sigma_1_i, one over the sigma_2_i; the host adds the chunks' points
//            device  ONE multi-pairing of L + 2 pairs against the prepared key: e(sum w_i sigma_1_i, alpha_tilde) prod_j e(sum w_i m_ij sigma_1_i, beta_tilde_j)
//                    e(-sum w_i sigma_2_i, g_tilde) against one                                                   k_lines_from_prepared, k_line_products, k_miller_tail, k_final_exp
//   pok each host    the GLS split of -c_i (an input: nothing of the device is waited for), -sigma_2'_i
//            device  the rows S_i = (0, hidden ? z : 0 .., z_r) and R_i = (1, revealed ? m : 0 .., 0), ONE many-row MSM of 2 rows over the whole key
//                                                                                                                 k_ps_pok_rows, k_many_tree, k_many_fold
//            device  S_i + (-c_i) k_i (compared with t_i) and Q_i = R_i + 1 k_i                                    k_mul_add_g2_gls x 2
//            device  e(sigma_1'_i, Q_i) e(-sigma_2'_i, g_tilde) as above; the checks into a status byte            .., k_ps_verdict
// Only verdict bytes or the signatures (sign) come back.  The device copies of the secret key, of the r_i and of the u_i are zeroed on every return path before
// the slot is released; the host holds no copy of them (the caller's words are uploaded as they are).
#include "msm_many.hip.h"
#include "qap_launch.hip.h"
#include "fixed_launch.hip.h"
#include "bbs_launch.hip.h"
#include "ps_launch.hip.h"
#include "acc_host_tables.hpp"
#include "pair_check.hip.h"             // zero_words, ws_check, coeffs_up, launch_check, check_tail, add_jac, merged_multi_verdict
using namespace dock;
using namespace acch;
using namespace mlk;

namespace dock {
template <class C> int32_t table_mul_device(Slot &sl, const void *table, const uint32_t *d_scalars, size_t n, void **keep, uint64_t *out, uint8_t *out_inf);   // dock_fixed.hip
}

namespace {

// the argument checks that come before the device is looked at (n > 0)
bool bad_shape(size_t L, size_t stride, size_t n) {
    return L == 0 || stride < L || n >= (1ull << 31) || L >= (1ull << 31) - 2 || stride >= (1ull << 31);
}
// the public key: a plain G2 bases handle of exactly L + 2 points, pinned for the call
bool pk_ok(const HandleRef &hb, size_t L) { return hb.ok && hb.h.kind == 2 && hb.h.n == L + 2; }
// rows per chunk of a call that runs no many-row MSM: the many-row kernels' rule all the same (dgpu_set_many_chunk_rows of the development surface cuts it)
size_t sign_chunk(size_t n, size_t L) { return std::min(n, std::min(psk::PS_EACH_CHUNK, many_chunk_rows(L + 1))); }
// [sigma_1 | -sigma_2] of the rows [r0, r0 + rows) of n x 2 x 12 words, to dst (rows x 24 u32 words each, the second block right behind the first)
void sides(const uint64_t *sigs, size_t r0, size_t rows, uint64_t *dst) {
    for (size_t i = 0; i < rows; i++) {
        memcpy(dst + 12 * i, sigs + 24 * (r0 + i), PT);
        neg_g1(dst + 12 * (rows + i), sigs + 24 * (r0 + i) + 12);
    }
}

// ---- Signature::new for n rows (ps_signature.rs:46-64): sigma_1 = r g, sigma_2 = (r (x + sum y_j m_j)) g with the caller's r_i ---------------------------------
int32_t sign_many(uint64_t g_table, size_t L, const uint64_t *sk, const uint64_t *messages, size_t stride, const uint64_t *r, size_t n, bool mont, uint64_t *out_sig, uint8_t *bad) {
    if (n == 0) return DGPU_OK;
    if (bad_shape(L, stride, n) || !sk || !messages || !r || !out_sig || !bad) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    HandleRef ht(g_table);
    if (!ht.ok || ht.h.kind != 5) return DGPU_E_BADARG;
    CtxScope on_owner(ht.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = sign_chunk(n, L);
    int32_t rc;
    // q[0]: the secret key, q[1]: r, q[2]: the messages, q[3]: [r_i | u_i]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure((1 + L) * 32))) return e;
        if ((e = o.q[1].ensure(chunk * 32))) return e;
        if ((e = o.q[2].ensure(chunk * L * 32))) return e;
        if ((e = o.q[3].ensure(2 * chunk * 32))) return e;
        return o.in_bases.ensure(2 * chunk * PT + 2 * chunk);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<uint8_t> inf(2 * n);
    DrainUnlessDone guard(sl);
    DeviceWipe dw(sl);
    dw.add(sl.q[0].p, (1 + L) * 32); dw.add(sl.q[1].p, chunk * 32); dw.add(sl.q[3].p, 2 * chunk * 32);
    HIPCHK(hipMemcpyAsync(sl.q[0].p, sk, (1 + L) * 32, hipMemcpyHostToDevice, s));
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        HIPCHK(hipMemcpyAsync(sl.q[1].p, r + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
        if ((rc = upload_rows_packed(s, sl.q[2].p, messages + r0 * stride * 4, L, stride, rows))) return rc;
        { StageTimer st(sl, "ps.sign_rows");
          psk::launch_ps_sign_rows(s, sl.q[0].as<uint32_t>(), sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), mont ? 1 : 0, rows, L, sl.q[3].as<uint32_t>()); }
        HIPCHK(hipGetLastError());
        // (the products come back and the stream is waited for inside: the next chunk's operands overwrite this one's)
        if ((rc = table_mul_device<G1>(sl, ht.h.p, sl.q[3].as<uint32_t>(), 2 * rows, nullptr, out_sig + 24 * r0, inf.data() + 2 * r0))) return rc;
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    // the reference returns such a signature (r_i = 0, or x + sum y_j m_ij = 0) and every verifier refuses it
    for (size_t k = 0; k < 2 * n; k++) if (inf[k]) memset(out_sig + 12 * k, 0, PT);
    for (size_t i = 0; i < n; i++) bad[i] = (inf[2 * i] || inf[2 * i + 1]) ? 1 : 0;
    return DGPU_OK;
}

// ---- Signature::verify for n rows (ps_signature.rs:95-142), a verdict per row ------------------------------------------------------------------------------------------
int32_t verify_each(uint64_t pk, size_t L, const uint64_t *g_tilde_pc, const uint64_t *sigs, const uint64_t *messages, size_t stride, size_t n, bool mont, uint8_t *ok) {
    if (n == 0) return DGPU_OK;
    if (bad_shape(L, stride, n) || !g_tilde_pc || !sigs || !messages || !ok) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    HandleRef hb(pk);
    if (!pk_ok(hb, L)) return DGPU_E_BADARG;
    const size_t nn = L + 1;
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const RowMsm<G2> qp = param_rows<G2>(sl, pk, hb.h, nn, psk::PS_EACH_CHUNK, n);
    const size_t chunk = qp.chunk;
    int32_t rc;
    // q[2]: the messages, q[3]: [sigma_1 | -sigma_2], q[4]: [Q | identity flags]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[2].ensure(chunk * L * 32))) return e;
        if ((e = o.q[3].ensure(2 * chunk * PT))) return e;
        if ((e = o.q[4].ensure(chunk * PT2 + chunk))) return e;
        if ((e = ws_check(o, chunk))) return e;
        return qp.workspace(o);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<uint64_t> pts(2 * chunk * 12);
    DrainUnlessDone guard(sl);
    uint32_t *d_rows = sl.in_scalars.as<uint32_t>(), *d_bad = sl.flags.as<uint32_t>(), *dS = sl.q[3].as<uint32_t>();
    uint8_t *dQ = sl.q[4].as<uint8_t>(), *dQinf = dQ + chunk * PT2;
    if ((rc = coeffs_up(sl, nullptr, g_tilde_pc, chunk))) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        sides(sigs, r0, rows, pts.data());
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                          // (rows are canonical: the flag stays clear; sl.flags takes the verdicts afterwards)
        HIPCHK(hipMemcpyAsync(dS, pts.data(), 2 * rows * PT, hipMemcpyHostToDevice, s));
        if ((rc = upload_rows_packed(s, sl.q[2].p, messages + r0 * stride * 4, L, stride, rows))) return rc;
        { StageTimer st(sl, "ps.rows"); psk::launch_ps_rows(s, sl.q[2].as<uint32_t>(), mont ? 1 : 0, rows, nn, d_rows); }
        if ((rc = qp.points(sl, d_rows, rows, d_bad, dQ, dQinf))) return rc;
        launch_check(sl, dS, (const uint32_t *)dQ, dQinf, dS + rows * 24, rows, chunk);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ok + r0, sl.flags.p, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    for (size_t i = 0; i < n; i++) if (zero_words(sigs + 24 * i, 12) || zero_words(sigs + 24 * i + 12, 12)) ok[i] = 0;      // ZeroSignature (ps_signature.rs:128-130)
    return DGPU_OK;
}

// ---- one verdict for n rows: with w_i = rho^i, e(sum w_i sigma_1_i, alpha_tilde) prod_j e(sum w_i m_ij sigma_1_i, beta_tilde_j) e(-sum w_i sigma_2_i, g_tilde) = 1 ----
int32_t verify_batch(uint64_t pk, size_t L, const uint64_t *all_pc, const uint64_t *sigs, const uint64_t *messages, size_t stride, size_t n, bool mont, const uint64_t *random,
                     int32_t *ok) {
    if (n == 0) { if (ok) *ok = 1; return DGPU_OK; }
    if (bad_shape(L, stride, n) || !all_pc || !sigs || !messages || !random || !ok) return DGPU_E_BADARG;
    if (fr_is_zero(fr_in(random, mont))) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    HandleRef hb(pk);
    if (!pk_ok(hb, L)) return DGPU_E_BADARG;
    for (size_t i = 0; i < n; i++) if (zero_words(sigs + 24 * i, 12) || zero_words(sigs + 24 * i + 12, 12)) { *ok = 0; return DGPU_OK; }      // ZeroSignature
    const size_t np = L + 2, cw = (size_t)DGPU_G2_PREPARED_WORDS;
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const int forced = gs.many_chunk.load();
    const size_t chunk = std::min(n, forced > 0 ? (size_t)forced : std::min(psk::PS_BATCH_CHUNK, std::max<size_t>(1, psk::PS_BATCH_TERMS / L)));
    int32_t rc;
    // q[2]: the messages, q[3]: the signatures, q[4]: the L + 2 merged points and their skip flags, q[9]: the L + 2 columns of scalars, q[10]: the prepared records
    // of [the sigma_1 | the sigma_2]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[2].ensure(chunk * L * 32))) return e;
        if ((e = o.q[3].ensure(2 * chunk * PT))) return e;
        if ((e = o.q[4].ensure(np * PT + np + 64))) return e;
        if ((e = o.q[9].ensure(np * chunk * 32))) return e;
        if ((e = o.q[10].ensure(2 * chunk * G1::AFF_STRIDE * 4))) return e;
        if ((e = ws_for<G1>(o, 2, chunk, 0, nullptr))) return e;
        if ((e = o.ml_coeffs.ensure(np * cw * 8 + 16))) return e;
        if ((e = o.ml_lines.ensure((size_t)N_LINES * LW * np * 4))) return e;
        return ws_check(o, 1);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<HPoint> P(np, HPoint::identity());
    DrainUnlessDone guard(sl);
    uint32_t *d_cols = sl.q[9].as<uint32_t>(), *d_rec1 = sl.q[10].as<uint32_t>(), *d_rec2 = d_rec1 + chunk * G1::AFF_STRIDE;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        const uint8_t *raw = sl.q[3].as<uint8_t>();
        HIPCHK(hipMemcpyAsync(sl.q[3].p, sigs + 24 * r0, 2 * rows * PT, hipMemcpyHostToDevice, s));
        if ((rc = upload_rows_packed(s, sl.q[2].p, messages + r0 * stride * 4, L, stride, rows))) return rc;
        { StageTimer st(sl, "msm.prep_bases");
          prep_g1(s, raw, 2 * PT, rows, d_rec1);
          prep_g1(s, raw + PT, 2 * PT, rows, d_rec2); }
        { StageTimer st(sl, "ps.columns"); psk::launch_ps_col_scalars(s, sl.q[2].as<uint32_t>(), (const uint32_t *)random, mont ? 1 : 0, rows, L, r0, chunk, d_cols); }
        HIPCHK(hipGetLastError());
        for (size_t k = 0; k < np; k++) if ((rc = msm_add(sl, k == L + 1 ? d_rec2 : d_rec1, d_cols + k * chunk * 8, rows, P[k]))) return rc;
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;                                                   // (every chunk's MSMs were waited for)
    // ONE multi-pairing of L + 2 pairs, each against its own prepared point
    return merged_multi_verdict(sl, P, all_pc, sl.q[4], "ps.lines", ok);
}

// ---- SignaturePoK::verify for n proofs (proof.rs:32-56) -------------------------------------------------------------------------------------------------------------
struct Proofs {
    const uint64_t *sigs, *g2_points, *resp_r, *values; const uint8_t *revealed; const uint64_t *challenge; size_t L, stride, n; bool mont;
};
// the four base-|x| digits of -c mod r: the scalar of S_i + (-c_i) k_i
void neg_gls(const uint64_t *c_words, bool mont, uint64_t *out) {
    uint64_t c[4];
    fr_in(c_words, mont).to_canonical(c);
    if (c[0] | c[1] | c[2] | c[3]) {
        uint64_t br = 0;
        for (int i = 0; i < 4; i++) { u128 d = (u128)FrH::MOD[i] - c[i] - br; c[i] = (uint64_t)d; br = (uint64_t)(d >> 64) & 1; }
    }
    hostf::gls4_decompose(c, out);
}
int32_t pok_verify_each(uint64_t pk, const uint64_t *g_tilde_pc, const Proofs &p, uint8_t *status) {
    if (p.n == 0) return DGPU_OK;
    if (bad_shape(p.L, p.stride, p.n) || !g_tilde_pc || !p.sigs || !p.g2_points || !p.resp_r || !p.values || !p.revealed || !p.challenge || !status) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n, L = p.L, nn = L + 2;
    HandleRef hb(pk);
    if (!pk_ok(hb, L)) return DGPU_E_BADARG;
    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> split(n * 4);
    const size_t parts = std::min<size_t>(16, (n + 4095) / 4096);
    int32_t rc = par_run(parts, [&](size_t k) {
        for (size_t i = n * k / parts; i < n * (k + 1) / parts; i++) neg_gls(p.challenge + 4 * i, p.mont, &split[4 * i]);
        return (int32_t)DGPU_OK;
    });
    if (rc) return rc;
    if (gs.prof) prof_add_host("ps.gls_split", ms_since(t0));
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    // two MSM rows per proof: a chunk is half the rows of the many-row rule, a whole number of pairs (a forced chunk of one row becomes two)
    const RowMsm<G2> qp = param_rows<G2>(sl, pk, hb.h, nn, psk::PS_EACH_CHUNK, 2 * n, 2);
    const size_t chunk = qp.chunk / 2;
    // q[0]: the split -c | the digits of one, q[1]: the responses over g_tilde, q[2]: the values, q[3]: the mask, q[4]: [S | R | identity flags], q[5]: k, q[6]: t,
    // q[7]: [sigma_1' | -sigma_2'], q[8]: [S - c k | Q | their identity flags | status]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure(chunk * 32 + 32))) return e;
        if ((e = o.q[1].ensure(chunk * 32))) return e;
        if ((e = o.q[2].ensure(chunk * L * 32))) return e;
        if ((e = o.q[3].ensure(chunk * L))) return e;
        if ((e = o.q[4].ensure(2 * chunk * PT2 + 2 * chunk))) return e;
        if ((e = o.q[5].ensure(chunk * PT2))) return e;
        if ((e = o.q[6].ensure(chunk * PT2))) return e;
        if ((e = o.q[7].ensure(2 * chunk * PT))) return e;
        if ((e = o.q[8].ensure(2 * chunk * PT2 + 3 * chunk))) return e;
        if ((e = ws_check(o, chunk))) return e;
        return qp.workspace(o);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<uint64_t> pts(2 * chunk * 12);
    DrainUnlessDone guard(sl);
    uint32_t *d_rows = sl.in_scalars.as<uint32_t>(), *d_bad = sl.flags.as<uint32_t>(), *d_split = sl.q[0].as<uint32_t>(), *d_one = d_split + chunk * 8;
    uint32_t *dSig = sl.q[7].as<uint32_t>(), *dK = sl.q[5].as<uint32_t>(), *dT = sl.q[6].as<uint32_t>();
    uint8_t *dSR = sl.q[4].as<uint8_t>(), *dSRinf = dSR + 2 * chunk * PT2;
    uint8_t *dGot = sl.q[8].as<uint8_t>(), *dQ = dGot + chunk * PT2, *dGotinf = dQ + chunk * PT2, *dQinf = dGotinf + chunk, *dstatus = dQinf + chunk;
    static const uint64_t one_digits[4] = {1, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(d_one, one_digits, 32, hipMemcpyHostToDevice, s));
    if ((rc = coeffs_up(sl, nullptr, g_tilde_pc, chunk))) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        sides(p.sigs, r0, rows, pts.data());
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                          // (rows are canonical: the flag stays clear; sl.flags takes the pairing's verdicts afterwards)
        HIPCHK(hipMemcpyAsync(d_split, &split[4 * r0], rows * 32, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sl.q[1].p, p.resp_r + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
        if ((rc = upload_rows_packed(s, sl.q[2].p, p.values + r0 * p.stride * 4, L, p.stride, rows))) return rc;
        HIPCHK(hipMemcpyAsync(sl.q[3].p, p.revealed + r0 * L, rows * L, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpy2DAsync(dK, PT2, p.g2_points + 48 * r0, 2 * PT2, PT2, rows, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpy2DAsync(dT, PT2, p.g2_points + 48 * r0 + 24, 2 * PT2, PT2, rows, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dSig, pts.data(), 2 * rows * PT, hipMemcpyHostToDevice, s));
        { StageTimer st(sl, "ps.pok_rows");
          psk::launch_ps_pok_rows(s, psk::PokDev{sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), sl.q[3].as<uint8_t>(), L, p.mont ? 1 : 0}, rows, d_rows); }
        // S_i: rows [0, rows), R_i: rows [rows, 2 rows)
        if ((rc = qp.points(sl, d_rows, 2 * rows, d_bad, dSR, dSRinf))) return rc;
        { StageTimer st(sl, "ps.mul_add");
          msm::launch_mul_add_g2_gls(s, dK, nullptr, d_split, 8, (const uint32_t *)dSR, dSRinf, rows, (uint32_t *)dGot, dGotinf);
          msm::launch_mul_add_g2_gls(s, dK, nullptr, d_one, 0, (const uint32_t *)(dSR + rows * PT2), dSRinf + rows, rows, (uint32_t *)dQ, dQinf); }
        launch_check(sl, dSig, (const uint32_t *)dQ, dQinf, dSig + rows * 24, rows, chunk);
        { StageTimer st(sl, "ps.pok_verdict"); psk::launch_ps_verdict(s, (const uint32_t *)dGot, dGotinf, dT, dSig, sl.flags.as<uint8_t>(), rows, dstatus); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(status + r0, dstatus, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    return DGPU_OK;
}

}  // namespace

extern "C" {
int32_t dgpu_ps_sign_many_g1(uint64_t g_table, size_t L, const uint64_t *sk, const uint64_t *messages, size_t row_stride, const uint64_t *r, size_t n, int32_t montgomery,
                             uint64_t *out_sig, uint8_t *bad) {
    return abi_guard([&] { return sign_many(g_table, L, sk, messages, row_stride, r, n, montgomery != 0, out_sig, bad); });
}
int32_t dgpu_ps_verify_each(uint64_t pk_g2, size_t L, const uint64_t *g_tilde_pc, const uint64_t *sigs, const uint64_t *messages, size_t row_stride, size_t n, int32_t montgomery,
                            uint8_t *ok) {
    return abi_guard([&] { return verify_each(pk_g2, L, g_tilde_pc, sigs, messages, row_stride, n, montgomery != 0, ok); });
}
int32_t dgpu_ps_verify_batch(uint64_t pk_g2, size_t L, const uint64_t *all_pc, const uint64_t *sigs, const uint64_t *messages, size_t row_stride, size_t n, int32_t montgomery,
                             const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] { return verify_batch(pk_g2, L, all_pc, sigs, messages, row_stride, n, montgomery != 0, random, ok); });
}
int32_t dgpu_ps_pok_verify_each(uint64_t pk_g2, size_t L, const uint64_t *g_tilde_pc, const uint64_t *sigs, const uint64_t *g2_points, const uint64_t *resp_r, const uint64_t *values,
                                size_t row_stride, const uint8_t *revealed, const uint64_t *challenge, size_t n, int32_t montgomery, uint8_t *status) {
    return abi_guard([&] {
        return pok_verify_each(pk_g2, g_tilde_pc, Proofs{sigs, g2_points, resp_r, values, revealed, challenge, L, row_stride, n, montgomery != 0}, status);
    });
}
}  // extern "C"
