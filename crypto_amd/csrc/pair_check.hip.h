// crypto_amd/csrc/pair_check.hip.h — the two-pair pairing check with shared lines and the merged verdict of a batch, for the bulk verifiers that end in
// e(P1_i, w) e(P2_i, g2) == 1 (dock_bbs.hip: BBS+ signatures and proofs of knowledge; dock_acc_pok.hip: accumulator proofs; dock_ps.hip; dock_saver.hip, which
// takes the pairing VALUES of its slices and a product of K + 2 pairs per slice from the same tail); and, in front, the small parts every bulk driver shares
// (dock_smc.hip and dock_bpp.hip too): PT / PT2, chunk_rows, row_layout, prep_g1, and beside add_jac: msm_add, params_msm, shared_points_add.  Host code of a
// driver unit: it is included after msm_many.hip.h and lives in the unit's anonymous namespace, as it did while dock_bbs.hip was its only user.
#pragma once
#include "msm_many.hip.h"
#include "pairing_launch.hip.h"
#include "gt_launch.hip.h"
using namespace dock;
using namespace mlk;

namespace {

// ---- the small parts the bulk drivers share (a unit uses those it needs: chunk_rows serves dock_smc.hip and dock_bpp.hip, params_msm dock_bbs.hip and
// dock_bpp.hip, shared_points_add dock_acc_pok.hip and dock_smc.hip, PT2 dock_ps.hip and dock_saver.hip) --------------------------------------------------------------
constexpr size_t PT = 96, PT2 = 192;      // bytes of an affine G1 / G2 point of the ABI
// rows per chunk: the largest count with rows * per <= limit, at least one (dgpu_set_many_chunk_rows of the development surface cuts it further)
size_t chunk_rows(size_t n, size_t limit, size_t per) {
    const int forced = gs.many_chunk.load();
    const size_t cap = std::max<size_t>(1, limit / per);
    return std::min(n, forced > 0 ? std::min((size_t)forced, cap) : cap);
}
// the segments of every row of a chunk — `own` terms a row, in one segment (first = 0) or in two, of `first` and own - first terms: the layout depends on the
// counts alone
void row_layout(size_t rows, size_t own, size_t first, SegLayout &lay) {
    const size_t segs = first ? 2 : 1;
    std::vector<uint64_t> ends(segs * rows);
    for (size_t i = 0; i < rows; i++) {
        if (first) ends[2 * i] = own * i + first;
        ends[segs * i + segs - 1] = own * (i + 1);
    }
    seg_layout(ends.data(), 0, ends.size(), lay);
}
// the prepared records of n affine G1 points of the ABI on the device, `stride` bytes apart, none marked as the identity
void prep_g1(hipStream_t s, const void *raw, size_t stride, size_t n, uint32_t *out) {
    msm::launch_prep_bases_raw<G1>(s, (const uint8_t *)raw, stride, 0, PT / 2, msm::NO_INF_OFF, nullptr, n, out);
}

bool zero_words(const uint64_t *w, int k) { uint64_t o = 0; for (int i = 0; i < k; i++) o |= w[i]; return o == 0; }
// -P on affine Montgomery words (y -> p - y; the identity, zero words, stays)
void neg_g1(uint64_t *out, const uint64_t *p) {
    memcpy(out, p, 48);
    hostf::Fq y; memcpy(&y, p + 6, 48);
    y = y.neg();
    memcpy(out + 6, &y, 48);
}

// ---- the pairing check of m <= `cols` rows on the device: e(P1_i, w) e(P2_i, g2) == 1 ---------------------------------------------------------------------------
// dP: [P1 | P2], cols affine points each; dsk: their skip flags in the same order (an identity contributes one, as everywhere in the library).  The coefficients
// of w and g2 are in sl.ml_coeffs, the wanted value (one) behind the Miller outputs in sl.ml_out.  Verdicts: sl.flags.
int32_t ws_check(Slot &o, size_t cols) {
    int32_t e;
    if ((e = o.ml_coeffs.ensure(2 * (size_t)DGPU_G2_PREPARED_WORDS * 8 + 16))) return e;
    if ((e = o.ml_lines.ensure((size_t)N_LINES * LW * 2 * cols * 4))) return e;
    if ((e = o.ml_partial.ensure((size_t)N_LINES * cols * F12W * 4))) return e;
    if ((e = o.ml_out.ensure(cols * 576 + 576))) return e;
    if ((e = o.ml_state.ensure((size_t)PXY_W * 2 * cols * 4))) return e;      // px, py of every pair: the affine-first-side form leaves its lines unevaluated
    return o.flags.ensure(std::max<size_t>(cols, 64));
}
// pk_pc == nullptr: the second set alone (the affine-first-side form has no fixed first point)
int32_t coeffs_up(Slot &sl, const uint64_t *pk_pc, const uint64_t *g2_pc, size_t cols) {
    const size_t cw = (size_t)DGPU_G2_PREPARED_WORDS;
    static const hostf::Fq12 one = hostf::Fq12::one();
    if (pk_pc) HIPCHK(hipMemcpyAsync(sl.ml_coeffs.p, pk_pc, cw * 8, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(hipMemcpyAsync(sl.ml_coeffs.as<uint64_t>() + cw, g2_pc, cw * 8, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(hipMemcpyAsync(sl.ml_out.as<uint8_t>() + cols * 576, &one, 576, hipMemcpyHostToDevice, sl.stream));
    return DGPU_OK;
}
// What follows the pairs' lines in sl.ml_lines, whoever wrote them: one "segment" of slice_len m pairs in m slices (slice i is the pairs i, i + m, ..), the loop's
// tail, the final exponentiation.  out_gt != nullptr receives the m pairing VALUES (144 words each); want != nullptr (an element on the device) sets the verdict
// bytes sl.flags[i] = (value i == want).  The Miller outputs go to the head of sl.ml_out.  pxy: the pairs' px, py where the lines came unevaluated, else nullptr
void pair_tail(Slot &sl, size_t m, int slice_len, const uint32_t *pxy, uint32_t *out_gt, const uint32_t *want) {
    hipStream_t s = sl.stream;
    uint32_t *fout = sl.ml_out.as<uint32_t>();
    { StageTimer st(sl, "bbs.products");
      launch_line_products(s, gs.ml_mode.load(), sl.ml_lines.as<uint32_t>(), (size_t)slice_len * m, slice_len, (int)m, sl.ml_partial.as<uint32_t>(), nullptr, 1, 0, N_LINES, pxy, false); }
    { StageTimer st(sl, "bbs.tail"); gtk::launch_miller_tail(s, sl.ml_partial.as<uint32_t>(), m, fout); }
    { StageTimer st(sl, "bbs.final_exp"); gtk::launch_final_exp(s, fout, m, out_gt, (uint8_t *)nullptr, want, want ? sl.flags.as<uint8_t>() : nullptr); }
}
// the check of m two-pair rows: slice i is the pairs i and i + m, i.e. the two lines of row i, compared with the one behind the `cols` Miller outputs
void check_tail(Slot &sl, size_t m, size_t cols, const uint32_t *pxy) { pair_tail(sl, m, 2, pxy, nullptr, sl.ml_out.as<uint32_t>() + cols * 144); }
// the value-returning sibling (dock_saver.hip: a pairing value per slice goes on to a table lookup): the values behind the m Miller outputs in sl.ml_out
// (which holds 2 m elements then); want as above, or nullptr
uint32_t *value_tail(Slot &sl, size_t m, const uint32_t *want) {
    uint32_t *gt = sl.ml_out.as<uint32_t>() + m * 144;
    pair_tail(sl, m, 2, nullptr, gt, want);
    return gt;
}
void launch_check(Slot &sl, const uint32_t *dP1, const uint32_t *dP2, const uint8_t *dsk, size_t m, size_t cols) {
    hipStream_t s = sl.stream;
    const size_t cw = (size_t)DGPU_G2_PREPARED_WORDS, np = 2 * m;
    uint32_t *lines = sl.ml_lines.as<uint32_t>();
    { StageTimer st(sl, "bbs.lines");
      launch_lines_from_prepared(s, dP1, sl.ml_coeffs.as<uint32_t>(), dsk, m, lines, np, nullptr, true);
      launch_lines_from_prepared(s, dP2, sl.ml_coeffs.as<uint32_t>() + cw * 2, dsk + m, m, lines + m, np, nullptr, true); }
    check_tail(sl, m, cols, nullptr);
}
// The second form: e(P1_i, Q_i) e(P2_i, g2) == 1 with a G2 point of its own per row (dock_ps.hip: PS signatures, whose verification lives in G2).  dQ: m affine
// G2 points on the device (48 words each) with their identity flags dQ_inf: such a pair is skipped, and so is one whose P is zero words (both line kernels
// see that themselves).  The first side runs the fused prepare + line kernel the mixed Miller loop runs for its affine pairs (one launch: no state between
// pieces), its lines unevaluated; the second side's prepared lines join them with neutral px, py; the product kernel evaluates.  m <= 8192 (the callers'
// chunks are at most 4096 rows).
void launch_check(Slot &sl, const uint32_t *dP1, const uint32_t *dQ, const uint8_t *dQ_inf, const uint32_t *dP2, size_t m, size_t cols) {
    hipStream_t s = sl.stream;
    const size_t cw = (size_t)DGPU_G2_PREPARED_WORDS, np = 2 * m;
    uint32_t *lines = sl.ml_lines.as<uint32_t>(), *pxy = sl.ml_state.as<uint32_t>();
    { StageTimer st(sl, "ps.lines");
      launch_lines_uneval(s, gs.ml_mode.load(), dP1, dQ, dQ_inf, m, lines, np, 62, 0, 0, nullptr, pxy);
      launch_lines_from_prepared(s, dP2, sl.ml_coeffs.as<uint32_t>() + cw * 2, nullptr, m, lines + m, np, pxy + m, true); }
    check_tail(sl, m, cols, pxy);
}

// ---- one verdict for n rows: the random linear combination RandomizedPairingChecker forms (utils/src/randomized_pairing_check.rs), merged before the pairing ----------
typedef hostf::HXyzz<hostf::Fq> HPoint;
void add_jac(HPoint &acc, const uint64_t *jac) {
    if (jac_is_identity(jac, 18)) return;
    hostf::Fq x, y, z; memcpy(&x, jac, 48); memcpy(&y, jac + 6, 48); memcpy(&z, jac + 12, 48);
    const hostf::Fq zz = z * z;
    HPoint p; p.x = x; p.y = y; p.zz = zz; p.zzz = zz * z; p.inf = false;
    acc.add_in_place(p);
}
// acc += sum_k scalars_k rec_k: one MSM of n terms over prepared records on the device (sub: msm_device's), waited for
int32_t msm_add(Slot &sl, const uint32_t *rec, const uint32_t *scalars, size_t n, HPoint &acc, const SmallSub *sub = nullptr) {
    uint64_t jac[18];
    int32_t rc;
    if ((rc = msm_device<G1, hostf::Fq>(sl, rec, scalars, n, jac, sub))) return rc;
    add_jac(acc, jac);
    return DGPU_OK;
}
// acc += sum_k c_k H_k: ONE MSM of nn terms over a resident base set (handle `params`), the scalars at d_c
int32_t params_msm(Slot &sl, uint64_t params, const Handle &h, const uint32_t *d_c, size_t nn, HPoint &acc) {
    SmallSub sub;
    const bool have = small_sub_for<G1>(sl, params, h, 0, nn, sub, true);
    return msm_add(sl, (const uint32_t *)h.p, d_c, nn, acc, have ? &sub : nullptr);
}
// the close of a batch's G1 equation: the nsh <= 3 shared points (host words) onto the device at `raw`, their prepared records at d_recs, and
// acc += sum_k c_k shared_k with the finished coefficients d_c — ONE small MSM
int32_t shared_points_add(Slot &sl, const uint64_t *shared, size_t nsh, Buf &raw, uint32_t *d_recs, const uint32_t *d_c, HPoint &acc) {
    hipStream_t s = sl.stream;
    HIPCHK(hipMemcpyAsync(raw.p, shared, nsh * PT, hipMemcpyHostToDevice, s));
    { StageTimer st(sl, "msm.prep_bases"); prep_g1(s, raw.p, PT, nsh, d_recs); }
    HIPCHK(hipGetLastError());
    return msm_add(sl, d_recs, d_c, nsh, acc);
}
// *ok = [e(P1, w) e(P2, g2) == 1] for the two merged points of a batch (an identity member is skipped); scratch: 2 PT + 64 bytes of the slot
int32_t merged_pair_verdict(Slot &sl, const HPoint &P1, const HPoint &P2, const uint64_t *pk_pc, const uint64_t *g2_pc, Buf &scratch, int32_t *ok) {
    hipStream_t s = sl.stream;
    int32_t rc;
    uint64_t pts[24 + 8] = {0};
    uint8_t *sk = (uint8_t *)(pts + 24);
    for (int k = 0; k < 2; k++) {
        const HPoint &P = k ? P2 : P1;
        sk[k] = P.inf ? 1 : 0;
        if (P.inf) continue;
        hostf::Fq X, Y, Z; P.to_normalised_jacobian(X, Y, Z);
        memcpy(pts + 12 * k, &X, 48); memcpy(pts + 12 * k + 6, &Y, 48);
    }
    uint8_t verdict = 0;
    DrainUnlessDone own(sl);                                             // (pts and verdict are this frame's)
    uint32_t *dP = scratch.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(dP, pts, sizeof pts, hipMemcpyHostToDevice, s));
    if ((rc = coeffs_up(sl, pk_pc, g2_pc, 1))) return rc;
    launch_check(sl, dP, dP + 24, (const uint8_t *)(dP + 48), 1, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&verdict, sl.flags.p, 1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    own.done = true;
    if (gs.prof) prof_flush(sl);
    *ok = verdict ? 1 : 0;
    return DGPU_OK;
}
// *ok = [prod_k e(P_k, Q_k) == 1] for the np merged points of a batch, each against its own prepared G2 point (all_pc: np coefficient blocks on the host):
// ONE multi-pairing — one segment, one slice, one final exponentiation (dock_ps.hip, dock_saver.hip: the column sums of a batch against the key).  An identity
// member is skipped.  scratch: np PT + np + 64 bytes of the slot; sl.ml_coeffs holds np blocks, sl.ml_lines np pairs' lines, the rest as ws_check(sl, 1).
int32_t merged_multi_verdict(Slot &sl, const std::vector<HPoint> &P, const uint64_t *all_pc, Buf &scratch, const char *lines_stage, int32_t *ok) {
    hipStream_t s = sl.stream;
    const size_t np = P.size(), cw = (size_t)DGPU_G2_PREPARED_WORDS;
    std::vector<uint64_t> pts(np * 12 + (np + 7) / 8, 0);
    uint8_t *sk = (uint8_t *)(pts.data() + np * 12);
    for (size_t k = 0; k < np; k++) {
        sk[k] = P[k].inf ? 1 : 0;
        if (P[k].inf) continue;
        hostf::Fq X, Y, Z; P[k].to_normalised_jacobian(X, Y, Z);
        memcpy(pts.data() + 12 * k, &X, 48); memcpy(pts.data() + 12 * k + 6, &Y, 48);
    }
    static const hostf::Fq12 one = hostf::Fq12::one();
    uint8_t verdict = 0;
    DrainUnlessDone own(sl);                                             // (pts and verdict are this frame's)
    uint32_t *dP = scratch.as<uint32_t>(), *fout = sl.ml_out.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(dP, pts.data(), np * 96 + np, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.ml_coeffs.p, all_pc, np * cw * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.ml_out.as<uint8_t>() + 576, &one, 576, hipMemcpyHostToDevice, s));
    { StageTimer st(sl, lines_stage); launch_lines_from_prepared(s, dP, sl.ml_coeffs.as<uint32_t>(), (const uint8_t *)(dP + np * 24), np, sl.ml_lines.as<uint32_t>(), np, nullptr, false); }
    pair_tail(sl, 1, (int)np, nullptr, nullptr, fout + 144);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&verdict, sl.flags.p, 1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    own.done = true;
    if (gs.prof) prof_flush(sl);
    *ok = verdict ? 1 : 0;
    return DGPU_OK;
}

}  // namespace
