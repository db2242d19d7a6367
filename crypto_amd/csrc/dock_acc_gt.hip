// crypto_amd/csrc/dock_acc_gt.hip — the accumulator proofs with a GT commitment in bulk (include/dock_gpu_acc_gt.h, libdock_gpu_acc_gt.so:
// dgpu_accumulator_gt_membership_proofs_verify_each_g1 / _verify_batch_g1, dgpu_accumulator_gt_non_membership_proofs_verify_each_g1 / _verify_batch_g1):
// MembershipProof::verify and NonMembershipProof::verify of vb_accumulator/src/proofs.rs (:890-996, :697-724, :1516-1580), for many proofs against ONE
// accumulator value V and one key, each call ONE device pipeline per chunk of rows.
//   each    device  the own scalars of the row's 17 (27) terms                                                                k_acc_gt_own
//           device  the bases of the row's segments, the shared points V, X, Y, Z [, K, P] copied into every row                k_acc_gt_stage
//           device  six segments a row (3, 3, 3, 3, 3, 2 terms), respectively eight (4, 4, 3, 3, 3, 3, 5, 2)                    k_small_table, k_seg_tree, k_seg_fold (seg_rows_resident)
//           device  the last two sums of a row, p and q, as the sides of its pairing and their skip flags                      k_acc_gt_sides
//           device  e(q_i, pk) e(p_i, P~): the lines of the two prepared points shared by every row, the VALUES left on the device      pair_check.hip.h value_tail
//           device  the first failing check of the row: the identity flags of its Schnorr sums, its value against its own R_E   k_acc_gt_verdict
//   batch   device  the coefficients of the shared points, the weights over the own points, t_i s_y, t_i c, t_i                 k_acc_gt_col_sums, k_col_finish
//           device  one MSM over the chunk's 7 n (11 n) own points, one (two) over the side against P~, one over the side against pk; the host adds the chunks'
//                   points
//           device  prod R_E_i^(t_i) of the chunk                                                                              k_gt_pow, k_gt_fold; the host multiplies the chunks'
//           device  small MSMs over the shared points: X, Y [, P, K] close the G1 equation; Z, V [, K] and Z the two sides
//           device  e(sum t q, pk) e(sum t p, P~) against the GT product                                                        pair_tail
// Only status bytes (each) or one verdict (batch) come back.  Nothing secret passes through: nothing is wiped.
#include "msm_many.hip.h"
#include "../../include/dock_gpu_acc_gt.h"
#include "acc_gt_launch.hip.h"
#include "acc_host_tables.hpp"
#include "pair_check.hip.h"
using namespace dock;
using namespace acch;
using namespace mlk;

namespace {

constexpr size_t GTB = 576, GT_ELW = 168;      // bytes of a GT element of the ABI; u32 words of one in the internal form (gt_kernels.hip.h)
// what the four calls share: the proofs' inputs.  prk: X, Y, Z [, K]; pp: params.P (non-membership)
struct Proofs {
    int kind; const uint64_t *v, *pp, *prk, *pk_pc, *ptilde_pc, *points, *r_e, *resp, *challenge; size_t n; bool mont;
    accgt::KindShape sh() const { return accgt::kind_shape(kind); }
};
// the argument checks that come before the device is looked at (n > 0)
bool bad_proofs(const Proofs &p) {
    if (p.kind == accgt::KIND_NON_MEMBERSHIP && !p.pp) return true;
    return !p.v || !p.prk || !p.pk_pc || !p.ptilde_pc || !p.points || !p.r_e || !p.resp || !p.challenge || p.n >= (1ull << 31);
}
// rows per chunk: the call's cap (dgpu_set_many_chunk_rows of the development surface cuts it, as it does for the CDH proofs)
size_t chunk_rows(size_t n, size_t cap) {
    const int forced = gs.many_chunk.load();
    return std::min(n, forced > 0 ? std::min((size_t)forced, cap) : cap);
}
// the shared points in the stage kernel's order: V, X, Y, Z, K, P (zero words where the kind has none)
void shared_words(const Proofs &p, uint64_t out[72]) {
    memset(out, 0, 72 * 8);
    memcpy(out, p.v, PT);
    memcpy(out + 12, p.prk, (p.kind == accgt::KIND_MEMBERSHIP ? 3 : 4) * PT);
    if (p.kind != accgt::KIND_MEMBERSHIP) memcpy(out + 60, p.pp, PT);
}
// q[0]: the challenges, q[1]: the responses, q[5]: the points of the rows of a chunk
int32_t ws_proofs(Slot &o, const accgt::KindShape &sh, size_t chunk) {
    int32_t e;
    if ((e = o.q[0].ensure(chunk * 32))) return e;
    if ((e = o.q[1].ensure(chunk * sh.resp * 32))) return e;
    return o.q[5].ensure(chunk * sh.pts * PT);
}
int32_t proofs_up(Slot &sl, const Proofs &p, size_t r0, size_t rows, uint32_t *d_re, accgt::ProofDev &dev) {
    hipStream_t s = sl.stream;
    const accgt::KindShape sh = p.sh();
    HIPCHK(hipMemcpyAsync(sl.q[0].p, p.challenge + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[1].p, p.resp + 4 * sh.resp * r0, rows * sh.resp * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[5].p, p.points + r0 * sh.pts * 12, rows * sh.pts * PT, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_re, p.r_e + 72 * r0, rows * GTB, hipMemcpyHostToDevice, s));
    dev = accgt::ProofDev{sl.q[0].as<uint32_t>(), sl.q[1].as<uint32_t>(), p.kind, p.mont ? 1 : 0};
    return DGPU_OK;
}
// the segments of every row of a chunk: the layout depends on the counts alone
void own_layout(int kind, size_t rows, SegLayout &lay) {
    const accgt::KindShape sh = accgt::kind_shape(kind);
    unsigned e[8];
    accgt::kind_seg_ends(kind, e);
    std::vector<uint64_t> ends((size_t)sh.segs * rows);
    for (size_t i = 0; i < rows; i++) for (int g = 0; g < sh.segs; g++) ends[i * sh.segs + g] = (uint64_t)sh.own * i + e[g];
    seg_layout(ends.data(), 0, ends.size(), lay);
}
// the coefficients of pk and of P~ where the line kernel reads them (pair_check.hip.h coeffs_up without the wanted value: the pairings here have none of their own)
int32_t pair_coeffs_up(Slot &sl, const uint64_t *pk_pc, const uint64_t *ptilde_pc) {
    const size_t cw = (size_t)DGPU_G2_PREPARED_WORDS;
    HIPCHK(hipMemcpyAsync(sl.ml_coeffs.p, pk_pc, cw * 8, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(hipMemcpyAsync(sl.ml_coeffs.as<uint64_t>() + cw, ptilde_pc, cw * 8, hipMemcpyHostToDevice, sl.stream));
    return DGPU_OK;
}
// the lines of m rows e(Pa_i, pk) e(Pb_i, P~) into sl.ml_lines (pair_check.hip.h launch_check without its tail)
void pair_lines(Slot &sl, const uint32_t *dPa, const uint32_t *dPb, const uint8_t *dsk, size_t m) {
    const size_t cw = (size_t)DGPU_G2_PREPARED_WORDS, np = 2 * m;
    uint32_t *lines = sl.ml_lines.as<uint32_t>();
    StageTimer st(sl, "bbs.lines");
    launch_lines_from_prepared(sl.stream, dPa, sl.ml_coeffs.as<uint32_t>(), dsk, m, lines, np, nullptr, true);
    launch_lines_from_prepared(sl.stream, dPb, sl.ml_coeffs.as<uint32_t>() + cw * 2, dsk + m, m, lines + m, np, nullptr, true);
}

int32_t verify_each(const Proofs &p, uint8_t *status) {
    if (p.n == 0) return DGPU_OK;
    if (bad_proofs(p) || !status) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n;
    const accgt::KindShape sh = p.sh();
    const size_t no = (size_t)sh.own, ns = (size_t)sh.segs;
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = chunk_rows(n, accgt::ACC_GT_EACH_CHUNK);
    int32_t rc;
    SegLayout lay, lay_tail;
    own_layout(p.kind, chunk, lay);
    if (n % chunk) own_layout(p.kind, n % chunk, lay_tail);
    uint64_t shared[72];
    shared_words(p, shared);
    // q[0], q[1], q[5]: the proofs (ws_proofs); q[2]: their R_E; q[6]: the own scalars, q[7]: the bases in segment order, q[8]: [q | p], the sides of the rows'
    // pairings, q[9]: [their skip flags | status]; sl.ml_out: [the Miller outputs | the pairings' values]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, sh, chunk))) return e;
        if ((e = o.q[2].ensure(chunk * GTB))) return e;
        if ((e = o.q[6].ensure(chunk * no * 32))) return e;
        if ((e = o.q[7].ensure(chunk * no * PT))) return e;
        if ((e = o.q[8].ensure(2 * chunk * PT))) return e;
        if ((e = o.q[9].ensure(3 * chunk + 64))) return e;
        if ((e = ws_check(o, chunk))) return e;
        if ((e = o.ml_out.ensure(2 * chunk * GTB))) return e;
        return ws_seg_resident<G1>(o, no * chunk, ns * chunk, lay.blocks);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_bad = sl.flags.as<uint32_t>(), *d_own = sl.q[6].as<uint32_t>(), *d_bases = sl.q[7].as<uint32_t>(), *d_re = sl.q[2].as<uint32_t>();
    uint32_t *dPa = sl.q[8].as<uint32_t>(), *dPb = dPa + chunk * (PT / 4);
    uint8_t *dsk = sl.q[9].as<uint8_t>(), *dstatus = dsk + 2 * chunk;
    if ((rc = pair_coeffs_up(sl, p.pk_pc, p.ptilde_pc))) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        accgt::ProofDev dev;
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                          // (the own scalars are canonical: the flag stays clear)
        if ((rc = proofs_up(sl, p, r0, rows, d_re, dev))) return rc;
        { StageTimer st(sl, "acc.gt_own"); accgt::launch_acc_gt_own(s, dev, rows, d_own); }
        { StageTimer st(sl, "acc.gt_stage"); accgt::launch_acc_gt_stage(s, sl.q[5].as<uint32_t>(), (const uint32_t *)shared, p.kind, rows, d_bases); }
        if ((rc = seg_rows_resident<G1>(sl, (const uint8_t *)d_bases, PT, d_own, no * rows, ns * rows, rows == chunk ? lay : lay_tail, d_bad))) return rc;
        { StageTimer st(sl, "acc.gt_sides"); accgt::launch_acc_gt_sides(s, sl.win.as<uint32_t>(), sl.win_inf.as<uint8_t>(), p.kind, rows, dPa, dPb, dsk); }
        pair_lines(sl, dPa, dPb, dsk, rows);
        const uint32_t *d_gt = value_tail(sl, rows, nullptr);
        { StageTimer st(sl, "acc.gt_verdict"); accgt::launch_acc_gt_verdict(s, sl.win_inf.as<uint8_t>(), d_gt, d_re, p.kind, rows, dstatus); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(status + r0, dstatus, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    return DGPU_OK;
}

// ---- the GT product of a chunk (dock_gt_dev.hip's fold, which lives in that unit's own namespace) ----
size_t fold_out(size_t m) { return (m + 7) / 8; }
size_t fold_a(size_t m) { return fold_out(m) + 1; }
size_t fold_b(size_t m) { return fold_out(fold_out(m)) + 1; }
// in (internal form, m elements) folded level by level; the last level writes ONE element of the ABI to `last`.  a / b: two scratch regions of fold_a(m) and
// fold_b(m) elements.  m == 1 still runs one level (a copy, converting the form).
void fold_to_one(hipStream_t s, const uint32_t *in, size_t m, uint32_t *a, uint32_t *b, uint32_t *last) {
    const uint32_t *cur_in = in;
    for (;;) {
        const bool fin = m <= 8;
        uint32_t *dst = fin ? last : a;
        m = gtk::launch_gt_fold(s, cur_in, false, m, 0, dst, fin);
        if (fin) return;
        cur_in = dst; std::swap(a, b);
    }
}
// acc *= prod_i r_e_i^(t_i) over the m rows of a chunk: d_re the elements (ABI), d_t their exponents (canonical words of 8); sl.ml_partial: the power tables,
// sl.ml_state: [the groups' products | fold scratch a, b | the chunk's product]
int32_t gt_product_mul(Slot &sl, const uint32_t *d_re, const uint32_t *d_t, size_t m, size_t chunk, uint64_t acc[72]) {
    hipStream_t s = sl.stream;
    uint32_t *prod = sl.ml_state.as<uint32_t>(), *fa = prod + chunk * GT_ELW, *fb = fa + fold_a(chunk) * GT_ELW, *out = fb + fold_b(chunk) * GT_ELW;
    const int k = gtk::bases_per_group(m);
    uint64_t part[72];
    { StageTimer st(sl, "gt.multi_pow"); gtk::launch_gt_pow(s, d_re, d_t, 8, m, 0, k, sl.ml_partial.as<uint32_t>(), prod, false); }
    { StageTimer st(sl, "gt.fold"); fold_to_one(s, prod, (m + k - 1) / k, fa, fb, out); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(part, out, GTB, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return dgpu_fp12_mul(acc, part, acc);
}
// *ok = [e(Pa, pk) e(Pb, P~) == want] for the two merged points of a batch (an identity member is skipped) — pair_check.hip.h merged_pair_verdict with a GT
// element of the caller's in the place of one; scratch: 2 PT + 64 bytes of the slot
int32_t merged_pair_equals(Slot &sl, const HPoint &Pa, const HPoint &Pb, const uint64_t *pk_pc, const uint64_t *ptilde_pc, const uint64_t want[72], Buf &scratch, int32_t *ok) {
    hipStream_t s = sl.stream;
    int32_t rc;
    uint64_t pts[24 + 8] = {0};
    uint8_t *sk = (uint8_t *)(pts + 24);
    for (int k = 0; k < 2; k++) {
        const HPoint &P = k ? Pb : Pa;
        sk[k] = P.inf ? 1 : 0;
        if (P.inf) continue;
        hostf::Fq X, Y, Z; P.to_normalised_jacobian(X, Y, Z);
        memcpy(pts + 12 * k, &X, 48); memcpy(pts + 12 * k + 6, &Y, 48);
    }
    uint8_t verdict = 0;
    DrainUnlessDone own(sl);                                             // (pts and verdict are this frame's)
    uint32_t *dP = scratch.as<uint32_t>(), *d_want = sl.ml_out.as<uint32_t>() + 144;
    HIPCHK(hipMemcpyAsync(dP, pts, sizeof pts, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_want, want, GTB, hipMemcpyHostToDevice, s));
    if ((rc = pair_coeffs_up(sl, pk_pc, ptilde_pc))) return rc;
    pair_lines(sl, dP, dP + 24, (const uint8_t *)(dP + 48), 1);
    pair_tail(sl, 1, 2, nullptr, nullptr, d_want);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&verdict, sl.flags.p, 1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    own.done = true;
    if (gs.prof) prof_flush(sl);
    *ok = verdict ? 1 : 0;
    return DGPU_OK;
}

// one verdict for n proofs: Schnorr check j of proof i weighs rho^(J i + j), its pairing and its R_E t_i = rho^i
int32_t verify_batch(const Proofs &p, const uint64_t *random, int32_t *ok) {
    if (p.n == 0) { if (ok) *ok = 1; return DGPU_OK; }
    if (bad_proofs(p) || !random || !ok) return DGPU_E_BADARG;
    if (fr_is_zero(fr_in(random, p.mont))) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n;
    const accgt::KindShape sh = p.sh();
    const size_t np = (size_t)sh.pts, ng = (size_t)sh.g1cols, npc = (size_t)sh.pcols, ncols = ng + npc + 1;
    const bool nm = p.kind != accgt::KIND_MEMBERSHIP;
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = chunk_rows(n, accgt::ACC_GT_BATCH_CHUNK);
    int32_t rc;
    // the shared points in the order of their columns: X, Y [P, K, X, Y] | Z, V [, K] | Z
    uint64_t all[72], cols[8 * 12];
    shared_words(p, all);
    const uint64_t *V = all, *X = all + 12, *Y = all + 24, *Z = all + 36, *K = all + 48, *Pp = all + 60;
    {
        size_t c = 0;
        auto put = [&](const uint64_t *pt) { memcpy(cols + 12 * c++, pt, PT); };
        if (nm) { put(Pp); put(K); }
        put(X); put(Y); put(Z); put(V);
        if (nm) put(K);
        put(Z);
    }
    // q[0], q[1], q[5]: the proofs (ws_proofs); q[2]: their R_E; q[4]: the merged sides and their skip flags, q[6]: the weights over the own points, q[7]: the
    // blocks' partial sums, q[8]: [the columns' coefficients | the running sums], q[9]: [t s_y | t c | t], q[10]: the prepared records of the own points, q[11]:
    // those of E_C and E_d, q[12]: the shared points, q[13]: their prepared records
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, sh, chunk))) return e;
        if ((e = o.q[2].ensure(chunk * GTB))) return e;
        if ((e = o.q[4].ensure(2 * PT + 64))) return e;
        if ((e = o.q[6].ensure(chunk * np * 32))) return e;
        if ((e = o.q[7].ensure(accgt::acc_gt_part_words(chunk, p.kind) * 4))) return e;
        if ((e = o.q[8].ensure(ncols * 32 + ncols * 40 + 64))) return e;
        if ((e = o.q[9].ensure(3 * chunk * 32))) return e;
        if ((e = o.q[10].ensure(chunk * np * G1::AFF_STRIDE * 4))) return e;
        if ((e = o.q[11].ensure(2 * chunk * G1::AFF_STRIDE * 4))) return e;
        if ((e = o.q[12].ensure(4 * PT))) return e;
        if ((e = o.q[13].ensure(4 * G1::AFF_STRIDE * 4))) return e;
        for (size_t terms : {np * chunk, chunk, (size_t)4}) if ((e = ws_for<G1>(o, 2, terms, 0, nullptr))) return e;
        if ((e = ws_check(o, 1))) return e;
        if ((e = o.ml_partial.ensure(gtk::pow_table_words(chunk) * 4))) return e;
        return o.ml_state.ensure((chunk + fold_a(chunk) + fold_b(chunk) + 1) * GT_ELW * 4);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_re = sl.q[2].as<uint32_t>(), *d_c = sl.q[8].as<uint32_t>(), *d_run = d_c + ncols * 8, *d_w = sl.q[6].as<uint32_t>();
    uint32_t *d_wp = sl.q[9].as<uint32_t>(), *d_wq = d_wp + chunk * 8, *d_tp = d_wq + chunk * 8;
    uint32_t *d_rec = sl.q[10].as<uint32_t>(), *d_recc = sl.q[11].as<uint32_t>(), *d_recd = d_recc + chunk * G1::AFF_STRIDE, *d_recs = sl.q[13].as<uint32_t>();
    HPoint Gsum = HPoint::identity(), Pside = HPoint::identity(), Qside = HPoint::identity();
    uint64_t gt[72];
    { static const hostf::Fq12 one = hostf::Fq12::one(); memcpy(gt, &one, GTB); }
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        accgt::ProofDev dev;
        if ((rc = proofs_up(sl, p, r0, rows, d_re, dev))) return rc;
        const uint8_t *raw = sl.q[5].as<uint8_t>();
        { StageTimer st(sl, "msm.prep_bases");
          prep_g1(s, raw, PT, np * rows, d_rec);
          prep_g1(s, raw, np * PT, rows, d_recc);                        // E_C
          if (nm) prep_g1(s, raw + 7 * PT, np * PT, rows, d_recd); }     // E_d
        { StageTimer st(sl, "acc.gt_columns");
          accgt::launch_acc_gt_columns(s, dev, (const uint32_t *)random, rows, r0, r0 == 0, sl.q[7].as<uint32_t>(), d_run, d_w, d_wp, d_wq, d_tp, d_c); }
        HIPCHK(hipGetLastError());
        if ((rc = msm_add(sl, d_rec, d_w, np * rows, Gsum))) return rc;
        if ((rc = msm_add(sl, d_recc, d_wp, rows, Pside))) return rc;
        if (nm && (rc = msm_add(sl, d_recd, d_wq, rows, Pside))) return rc;
        if ((rc = msm_add(sl, d_recc, d_wq, rows, Qside))) return rc;
        if ((rc = gt_product_mul(sl, d_re, d_tp, rows, chunk, gt))) return rc;
        if (gs.prof) prof_flush(sl);
    }
    // the shared points' terms of the G1 equation: ONE small MSM over X, Y [, P, K] with the finished coefficients
    if ((rc = shared_points_add(sl, cols, ng, sl.q[12], d_recs, d_c, Gsum))) return rc;
    if (!Gsum.inf) { HIPCHK(hipStreamSynchronize(s)); guard.done = true; *ok = 0; return DGPU_OK; }      // the G1 equation fails: the pairing cannot mend it
    // ... and of the two sides: -(sum t (s_delta_sigma + s_delta_rho)) Z - (sum t c) V [- (sum t s_v) K], and -(sum t (s_sigma + s_rho)) Z
    if ((rc = shared_points_add(sl, cols + 12 * ng, npc, sl.q[12], d_recs, d_c + 8 * ng, Pside))) return rc;
    if ((rc = shared_points_add(sl, cols + 12 * (ng + npc), 1, sl.q[12], d_recs, d_c + 8 * (ng + npc), Qside))) return rc;
    if ((rc = merged_pair_equals(sl, Qside, Pside, p.pk_pc, p.ptilde_pc, gt, sl.q[4], ok))) return rc;
    guard.done = true;
    return DGPU_OK;
}

Proofs membership(const uint64_t *v, const uint64_t *prk, const uint64_t *pk_pc, const uint64_t *ptilde_pc, const uint64_t *points, const uint64_t *r_e, const uint64_t *resp,
                  const uint64_t *challenge, size_t n, int32_t mont) {
    return Proofs{accgt::KIND_MEMBERSHIP, v, nullptr, prk, pk_pc, ptilde_pc, points, r_e, resp, challenge, n, mont != 0};
}
Proofs non_membership(const uint64_t *v, const uint64_t *pp, const uint64_t *prk, const uint64_t *pk_pc, const uint64_t *ptilde_pc, const uint64_t *points, const uint64_t *r_e,
                      const uint64_t *resp, const uint64_t *challenge, size_t n, int32_t mont) {
    return Proofs{accgt::KIND_NON_MEMBERSHIP, v, pp, prk, pk_pc, ptilde_pc, points, r_e, resp, challenge, n, mont != 0};
}

}  // namespace

extern "C" {
int32_t dgpu_accumulator_gt_membership_proofs_verify_each_g1(const uint64_t accumulator_xy[12], const uint64_t prk_xy[36], const uint64_t *pk_pc, const uint64_t *ptilde_pc,
                                                             const uint64_t *points, const uint64_t *r_e, const uint64_t *responses, const uint64_t *challenge, size_t n,
                                                             int32_t montgomery, uint8_t *status) {
    return abi_guard([&] { return verify_each(membership(accumulator_xy, prk_xy, pk_pc, ptilde_pc, points, r_e, responses, challenge, n, montgomery), status); });
}
int32_t dgpu_accumulator_gt_membership_proofs_verify_batch_g1(const uint64_t accumulator_xy[12], const uint64_t prk_xy[36], const uint64_t *pk_pc, const uint64_t *ptilde_pc,
                                                              const uint64_t *points, const uint64_t *r_e, const uint64_t *responses, const uint64_t *challenge, size_t n,
                                                              int32_t montgomery, const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] { return verify_batch(membership(accumulator_xy, prk_xy, pk_pc, ptilde_pc, points, r_e, responses, challenge, n, montgomery), random, ok); });
}
int32_t dgpu_accumulator_gt_non_membership_proofs_verify_each_g1(const uint64_t accumulator_xy[12], const uint64_t p_xy[12], const uint64_t prk_xy[48], const uint64_t *pk_pc,
                                                                 const uint64_t *ptilde_pc, const uint64_t *points, const uint64_t *r_e, const uint64_t *responses,
                                                                 const uint64_t *challenge, size_t n, int32_t montgomery, uint8_t *status) {
    return abi_guard([&] { return verify_each(non_membership(accumulator_xy, p_xy, prk_xy, pk_pc, ptilde_pc, points, r_e, responses, challenge, n, montgomery), status); });
}
int32_t dgpu_accumulator_gt_non_membership_proofs_verify_batch_g1(const uint64_t accumulator_xy[12], const uint64_t p_xy[12], const uint64_t prk_xy[48], const uint64_t *pk_pc,
                                                                  const uint64_t *ptilde_pc, const uint64_t *points, const uint64_t *r_e, const uint64_t *responses,
                                                                  const uint64_t *challenge, size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] { return verify_batch(non_membership(accumulator_xy, p_xy, prk_xy, pk_pc, ptilde_pc, points, r_e, responses, challenge, n, montgomery), random, ok); });
}
}  // extern "C"
