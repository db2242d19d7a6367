// crypto_amd/csrc/dock_acc_pok.hip — accumulator proofs in bulk (include/dock_gpu.h: dgpu_accumulator_membership_proofs_verify_each_g1 / _verify_batch_g1,
// dgpu_accumulator_non_membership_proofs_verify_each_g1 / _verify_batch_g1): the CDH proofs of the VB accumulator, MembershipProof::verify and
// NonMembershipProof::verify (vb_accumulator/src/proofs_cdh.rs:138-149, :365-387, :481-523 over short_group_sig/src/weak_bb_sig_pok_cdh.rs:145-287), for many
// proofs against ONE accumulator value V and one key, each call ONE device pipeline per chunk of rows.
//   each    device  the own scalars (z1, -z2, -c, -1), respectively (s_d, -c, -1 | s_r, -s_y, -s_d, -c, -1)        k_acc_pok_own
//           device  the bases of the row's segments ([V, A', Abar, T], respectively [Q, J, T2 | V, C', P, Cbar, T1]), the two sides of its pairing
//                   (A' and -Abar, respectively C' and -Cbar), the zero-point flags                                 k_acc_pok_stage
//           device  one 4-term segment per row, respectively a 3-term and a 5-term one                              k_small_table, k_seg_tree, k_seg_fold (seg_rows_resident)
//           device  e(A'_i, pk) e(-Abar_i, P~): the lines of the two prepared points shared by every row            pair_check.hip.h launch_check
//           device  the first failing check of the row                                                              k_acc_pok_verdict
//   batch   device  the coefficients of the shared points, the weights over the own points, +-rho^i                 k_acc_pok_col_sums, k_col_finish
//           device  one MSM over the chunk's 3 n (5 n) own points, one each over the two pairing sides; ONE over the 1 (3) shared points; the host adds the
//                   chunks' points
//           device  e(sum rho^i A'_i, pk) e(-sum rho^i Abar_i, P~) against one                                      pair_check.hip.h merged_pair_verdict
// Only status bytes (each) or one verdict (batch) come back.  Nothing secret passes through: nothing is wiped.
#include "msm_many.hip.h"
#include "acc_pok_launch.hip.h"
#include "acc_host_tables.hpp"
#include "pair_check.hip.h"
using namespace dock;
using namespace acch;
using namespace mlk;

namespace {

// what the four calls share: the proofs' inputs.  shared: V, then P and Q for non-membership
struct Proofs {
    int kind; const uint64_t *shared[3]; const uint64_t *points, *resp, *challenge; size_t n; bool mont;
    accpk::KindShape sh() const { return accpk::kind_shape(kind); }
};
// the argument checks that come before the device is looked at (n > 0)
bool bad_proofs(const Proofs &p) {
    for (int k = 0; k < p.sh().shared; k++) if (!p.shared[k]) return true;
    return !p.points || !p.resp || !p.challenge || p.n >= (1ull << 31);
}
// the points that must not be the identity: the proof's first (A', C') and, for non-membership, J — decided on the zero words
bool has_zero_point(const Proofs &p, size_t i) {
    const size_t np = (size_t)p.sh().pts;
    return zero_words(p.points + np * 12 * i, 12) || (p.kind == accpk::KIND_NON_MEMBERSHIP && zero_words(p.points + (np * i + 2) * 12, 12));
}
// rows per chunk: the call's cap (dgpu_set_many_chunk_rows of the development surface cuts it, as it does for BBS+)
size_t chunk_rows(size_t n, size_t cap) {
    const int forced = gs.many_chunk.load();
    return std::min(n, forced > 0 ? (size_t)forced : cap);
}
// q[0]: the challenges, q[1]: the responses, q[5]: the points of the rows of a chunk
int32_t ws_proofs(Slot &o, const accpk::KindShape &sh, size_t chunk) {
    int32_t e;
    if ((e = o.q[0].ensure(chunk * 32))) return e;
    if ((e = o.q[1].ensure(chunk * sh.resp * 32))) return e;
    return o.q[5].ensure(chunk * sh.pts * PT);
}
int32_t proofs_up(Slot &sl, const Proofs &p, size_t r0, size_t rows, accpk::ProofDev &dev) {
    hipStream_t s = sl.stream;
    const accpk::KindShape sh = p.sh();
    HIPCHK(hipMemcpyAsync(sl.q[0].p, p.challenge + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[1].p, p.resp + 4 * sh.resp * r0, rows * sh.resp * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[5].p, p.points + r0 * sh.pts * 12, rows * sh.pts * PT, hipMemcpyHostToDevice, s));
    dev = accpk::ProofDev{sl.q[0].as<uint32_t>(), sl.q[1].as<uint32_t>(), p.kind, p.mont ? 1 : 0};
    return DGPU_OK;
}
// the segments of every row of a chunk — one of 4 terms, respectively one of 3 and one of 5
void own_layout(const accpk::KindShape &sh, size_t rows, SegLayout &lay) { row_layout(rows, (size_t)sh.own, sh.segs == 1 ? 0 : 3, lay); }
void shared_words(const Proofs &p, uint64_t out[36]) {
    memset(out, 0, 36 * 8);
    for (int k = 0; k < p.sh().shared; k++) memcpy(out + 12 * k, p.shared[k], PT);
}

int32_t verify_each(const uint64_t *pk_pc, const uint64_t *ptilde_pc, const Proofs &p, uint8_t *status) {
    if (p.n == 0) return DGPU_OK;
    if (bad_proofs(p) || !pk_pc || !ptilde_pc || !status) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n;
    const accpk::KindShape sh = p.sh();
    const size_t no = (size_t)sh.own, ns = (size_t)sh.segs;
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = chunk_rows(n, accpk::ACC_POK_EACH_CHUNK);
    int32_t rc;
    SegLayout lay, lay_tail;
    own_layout(sh, chunk, lay);
    if (n % chunk) own_layout(sh, n % chunk, lay_tail);
    uint64_t shared[36];
    shared_words(p, shared);
    // q[0], q[1], q[5]: the proofs (ws_proofs); q[6]: the own scalars, q[7]: the bases in segment order, q[8]: [A' | -Abar], q[9]: [the zero-point flags | status]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, sh, chunk))) return e;
        if ((e = o.q[6].ensure(chunk * no * 32))) return e;
        if ((e = o.q[7].ensure(chunk * no * PT))) return e;
        if ((e = o.q[8].ensure(2 * chunk * PT))) return e;
        if ((e = o.q[9].ensure(4 * chunk))) return e;
        if ((e = ws_check(o, chunk))) return e;
        return ws_seg_resident<G1>(o, no * chunk, ns * chunk, lay.blocks);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_bad = sl.flags.as<uint32_t>(), *d_own = sl.q[6].as<uint32_t>(), *d_opts = sl.q[7].as<uint32_t>();
    uint32_t *dPa = sl.q[8].as<uint32_t>(), *dPb = dPa + chunk * (PT / 4);
    uint8_t *dsk = sl.q[9].as<uint8_t>(), *dstatus = dsk + 3 * chunk;
    if ((rc = coeffs_up(sl, pk_pc, ptilde_pc, chunk))) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        accpk::ProofDev dev;
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                          // (the own scalars are canonical: the flag stays clear; sl.flags takes the pairing's verdicts afterwards)
        if ((rc = proofs_up(sl, p, r0, rows, dev))) return rc;
        { StageTimer st(sl, "acc.pok_own"); accpk::launch_acc_pok_own(s, dev, rows, d_own); }
        { StageTimer st(sl, "acc.pok_stage"); accpk::launch_acc_pok_stage(s, sl.q[5].as<uint32_t>(), (const uint32_t *)shared, p.kind, rows, d_opts, dPa, dPb, dsk); }
        if ((rc = seg_rows_resident<G1>(sl, (const uint8_t *)d_opts, PT, d_own, no * rows, ns * rows, rows == chunk ? lay : lay_tail, d_bad))) return rc;
        launch_check(sl, dPa, dPb, dsk, rows, chunk);
        { StageTimer st(sl, "acc.pok_verdict"); accpk::launch_acc_pok_verdict(s, sl.win_inf.as<uint8_t>(), sl.flags.as<uint8_t>(), dsk, p.kind, rows, dstatus); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(status + r0, dstatus, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    return DGPU_OK;
}

// one verdict for n proofs.  Membership: row i weighs its Schnorr check and its pairing with rho^i.  Non-membership: the five-term check with u_i = rho^(2 i), the
// check of J with v_i = rho^(2 i + 1), the pairing with t_i = rho^i
int32_t verify_batch(const uint64_t *pk_pc, const uint64_t *ptilde_pc, const Proofs &p, const uint64_t *random, int32_t *ok) {
    if (p.n == 0) { if (ok) *ok = 1; return DGPU_OK; }
    if (bad_proofs(p) || !pk_pc || !ptilde_pc || !random || !ok) return DGPU_E_BADARG;
    if (fr_is_zero(fr_in(random, p.mont))) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n;
    const accpk::KindShape sh = p.sh();
    const size_t np = (size_t)sh.pts, nsh = (size_t)sh.shared;
    for (size_t i = 0; i < n; i++) if (has_zero_point(p, i)) { *ok = 0; return DGPU_OK; }      // CannotBeZero / InvalidProof
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = chunk_rows(n, accpk::ACC_POK_BATCH_CHUNK);
    int32_t rc;
    uint64_t shared[36];
    shared_words(p, shared);
    // q[0], q[1], q[5]: the proofs (ws_proofs); q[4]: [P1 | P2] and their skip flags, q[6]: the weights over the own points, q[7]: the blocks' partial sums,
    // q[8]: [the shared points' coefficients | the running sums], q[9]: [rho^i | -rho^i], q[10]: the prepared records of the own points, q[11]: those of the
    // two pairing sides, q[12]: the shared points, q[13]: their prepared records
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, sh, chunk))) return e;
        if ((e = o.q[4].ensure(2 * PT + 64))) return e;
        if ((e = o.q[6].ensure(chunk * np * 32))) return e;
        if ((e = o.q[7].ensure(accpk::acc_pok_part_words(chunk, p.kind) * 4))) return e;
        if ((e = o.q[8].ensure(nsh * 40 + nsh * 32 + 64))) return e;
        if ((e = o.q[9].ensure(2 * chunk * 32))) return e;
        if ((e = o.q[10].ensure(chunk * np * G1::AFF_STRIDE * 4))) return e;
        if ((e = o.q[11].ensure(2 * chunk * G1::AFF_STRIDE * 4))) return e;
        if ((e = o.q[12].ensure(3 * PT))) return e;
        if ((e = o.q[13].ensure(3 * G1::AFF_STRIDE * 4))) return e;
        for (size_t terms : {np * chunk, chunk, nsh}) if ((e = ws_for<G1>(o, 2, terms, 0, nullptr))) return e;
        return ws_check(o, 1);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_c = sl.q[8].as<uint32_t>(), *d_run = d_c + nsh * 8, *d_w = sl.q[6].as<uint32_t>(), *d_tp = sl.q[9].as<uint32_t>(), *d_tn = d_tp + chunk * 8;
    uint32_t *d_rec = sl.q[10].as<uint32_t>(), *d_reca = sl.q[11].as<uint32_t>(), *d_recb = d_reca + chunk * G1::AFF_STRIDE, *d_recs = sl.q[13].as<uint32_t>();
    HPoint Gsum = HPoint::identity(), P1 = HPoint::identity(), P2 = HPoint::identity();
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        accpk::ProofDev dev;
        if ((rc = proofs_up(sl, p, r0, rows, dev))) return rc;
        const uint8_t *raw = sl.q[5].as<uint8_t>();
        { StageTimer st(sl, "msm.prep_bases");
          prep_g1(s, raw, PT, np * rows, d_rec);
          prep_g1(s, raw, np * PT, rows, d_reca);
          prep_g1(s, raw + PT, np * PT, rows, d_recb); }
        { StageTimer st(sl, "acc.pok_columns");
          accpk::launch_acc_pok_columns(s, dev, (const uint32_t *)random, rows, r0, r0 == 0, sl.q[7].as<uint32_t>(), d_run, d_w, d_tp, d_tn, d_c); }
        HIPCHK(hipGetLastError());
        if ((rc = msm_add(sl, d_rec, d_w, np * rows, Gsum))) return rc;
        if ((rc = msm_add(sl, d_reca, d_tp, rows, P1))) return rc;
        if ((rc = msm_add(sl, d_recb, d_tn, rows, P2))) return rc;
        if (gs.prof) prof_flush(sl);
    }
    // the shared points' terms: ONE small MSM over V [, P, Q] with the finished coefficients
    if ((rc = shared_points_add(sl, shared, nsh, sl.q[12], d_recs, d_c, Gsum))) return rc;
    if (!Gsum.inf) { HIPCHK(hipStreamSynchronize(s)); guard.done = true; *ok = 0; return DGPU_OK; }      // the G1 equation fails: the pairing cannot mend it
    if ((rc = merged_pair_verdict(sl, P1, P2, pk_pc, ptilde_pc, sl.q[4], ok))) return rc;
    guard.done = true;
    return DGPU_OK;
}

Proofs membership(const uint64_t *v, const uint64_t *points, const uint64_t *resp, const uint64_t *challenge, size_t n, int32_t mont) {
    return Proofs{accpk::KIND_MEMBERSHIP, {v, nullptr, nullptr}, points, resp, challenge, n, mont != 0};
}
Proofs non_membership(const uint64_t *v, const uint64_t *pp, const uint64_t *q, const uint64_t *points, const uint64_t *resp, const uint64_t *challenge, size_t n, int32_t mont) {
    return Proofs{accpk::KIND_NON_MEMBERSHIP, {v, pp, q}, points, resp, challenge, n, mont != 0};
}

}  // namespace

extern "C" {
int32_t dgpu_accumulator_membership_proofs_verify_each_g1(const uint64_t accumulator_xy[12], const uint64_t *pk_pc, const uint64_t *ptilde_pc, const uint64_t *points,
                                                          const uint64_t *responses, const uint64_t *challenge, size_t n, int32_t montgomery, uint8_t *status) {
    return abi_guard([&] { return verify_each(pk_pc, ptilde_pc, membership(accumulator_xy, points, responses, challenge, n, montgomery), status); });
}
int32_t dgpu_accumulator_membership_proofs_verify_batch_g1(const uint64_t accumulator_xy[12], const uint64_t *pk_pc, const uint64_t *ptilde_pc, const uint64_t *points,
                                                           const uint64_t *responses, const uint64_t *challenge, size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] { return verify_batch(pk_pc, ptilde_pc, membership(accumulator_xy, points, responses, challenge, n, montgomery), random, ok); });
}
int32_t dgpu_accumulator_non_membership_proofs_verify_each_g1(const uint64_t accumulator_xy[12], const uint64_t p_xy[12], const uint64_t q_xy[12], const uint64_t *pk_pc,
                                                              const uint64_t *ptilde_pc, const uint64_t *points, const uint64_t *responses, const uint64_t *challenge, size_t n,
                                                              int32_t montgomery, uint8_t *status) {
    return abi_guard([&] { return verify_each(pk_pc, ptilde_pc, non_membership(accumulator_xy, p_xy, q_xy, points, responses, challenge, n, montgomery), status); });
}
int32_t dgpu_accumulator_non_membership_proofs_verify_batch_g1(const uint64_t accumulator_xy[12], const uint64_t p_xy[12], const uint64_t q_xy[12], const uint64_t *pk_pc,
                                                               const uint64_t *ptilde_pc, const uint64_t *points, const uint64_t *responses, const uint64_t *challenge, size_t n,
                                                               int32_t montgomery, const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] { return verify_batch(pk_pc, ptilde_pc, non_membership(accumulator_xy, p_xy, q_xy, points, responses, challenge, n, montgomery), random, ok); });
}
}  // extern "C"
