// crypto_amd/csrc/dock_smc.hip — range proofs over weak-BB signatures in bulk (include/dock_gpu_smc.h, libdock_gpu_smc.so: dgpu_smc_range_proofs_verify_each_g1 /
// _verify_batch_g1): CLSRangeProof::verify (smc_range_proof/src/cls_range_proof/range_proof_cdh.rs:164-189, :226-256) and CCSArbitraryRangeProof::verify
// (ccs_range_proof/arbitrary_range_cdh.rs:210-250, :311-359) over short_group_sig/src/weak_bb_sig_pok_cdh.rs:145-287, for many proofs of ONE statement, each
// call ONE device pipeline per chunk of proofs.  A proof is M = S (l + 1) four-term equations — S commitment equations, S l digit proofs — and S l pairings.
//   each    device  the own scalars (a_s c, b_s c + sum_j w_j z2_sj, e_s zr_s, -1) and (z1, -z2, -c, -1), one lane per equation     k_smc_own
//           device  the bases [C, g, h, D_s] and [g1, A', Abar, T] with g1, g, h copied into every segment, the two sides of every digit's pairing (A' and
//                   -Abar), the zero-point flags                                                                                     k_smc_stage
//           device  one 4-term segment per equation                                                         k_small_table, k_seg_tree, k_seg_fold (seg_rows_resident)
//           device  e(A'_d, pk) e(-Abar_d, g2): the lines of the two prepared points shared by every slice                           pair_check.hip.h launch_check
//           device  (status, detail) of the proof: its first failure in the reference's order                                        k_smc_verdict
//   merged  (each with random_i) as each, but the proof's pairings become ONE: the weights random_i^d, two more segments of S l terms over the staged A'
//           and -Abar in the SAME segment launch, their sums as the pairing's two sides               k_smc_merge_weights, k_smc_merged_sides, launch_check
//   batch   device  the own scalars as above; the coefficients of g1, g, h, the weights over the own points, +-rho^slice             k_smc_own, k_smc_col_sums, k_col_finish
//           device  one MSM over the chunk's C and D points, one over its 3 S l n digit points, one each over the two pairing sides; ONE over g1, g, h; the
//                   host adds the chunks' points
//           device  e(sum t A', pk) e(-sum t Abar, g2) against one                                                                   pair_check.hip.h merged_pair_verdict
// Only status bytes and details (each) or one verdict (batch) come back.  Nothing secret passes through: nothing is wiped.
#include "msm_many.hip.h"
#include "../../include/dock_gpu_smc.h"
#include "smc_launch.hip.h"
#include "acc_host_tables.hpp"
#include "pair_check.hip.h"
using namespace dock;
using namespace acch;
using namespace mlk;

namespace {

// what the two calls share: the statement and the proofs' inputs
struct Proofs {
    const uint64_t *g1, *ck_g, *ck_h, *pk_pc, *g2_pc; int32_t sides; size_t l; const uint64_t *weights, *side_consts;
    const uint64_t *commitments, *digit_points, *digit_resp, *side_points, *side_resp, *challenge; size_t n; bool mont;
    size_t S() const { return (size_t)sides; }
    size_t D() const { return S() * l; }            // digits = pairing slices of a proof
    size_t M() const { return S() * (l + 1); }      // equations of a proof
};
// the argument checks that come before the device is looked at (n > 0)
bool bad_proofs(const Proofs &p) {
    if (p.sides != 1 && p.sides != 2) return true;
    if (p.l > (size_t)smck::SMC_MAX_L || p.n >= (1ull << 31)) return true;
    if (!p.g1 || !p.ck_g || !p.ck_h || !p.pk_pc || !p.g2_pc || !p.side_consts || !p.commitments || !p.side_points || !p.side_resp || !p.challenge) return true;
    return p.l > 0 && (!p.weights || !p.digit_points || !p.digit_resp);
}
// q[0]: the challenges, q[1]: the sides' responses, q[2]: the digits' responses, q[3]: the statement, q[4]: [C | D] (the scratch of the merged verdict afterwards),
// q[5]: the digits' points, q[6]: the own scalars
int32_t ws_proofs(Slot &o, const Proofs &p, size_t chunk) {
    int32_t e;
    if ((e = o.q[0].ensure(chunk * 32))) return e;
    if ((e = o.q[1].ensure(chunk * p.S() * 32))) return e;
    if ((e = o.q[2].ensure(std::max<size_t>(chunk * p.D() * 64, 64)))) return e;
    if ((e = o.q[3].ensure((smck::SMC_STMT_CONSTS + (size_t)smck::SMC_MAX_L) * 32))) return e;
    if ((e = o.q[4].ensure(std::max(chunk * (1 + p.S()) * PT, 2 * PT + 64)))) return e;
    if ((e = o.q[5].ensure(std::max<size_t>(chunk * p.D() * 3 * PT, 64)))) return e;
    return o.q[6].ensure(chunk * p.M() * 4 * 32);
}
int32_t statement_up(Slot &sl, const Proofs &p) {
    uint64_t st[(smck::SMC_STMT_CONSTS + smck::SMC_MAX_L) * 4] = {0};
    memcpy(st, p.side_consts, p.S() * 3 * 32);
    if (p.l) memcpy(st + smck::SMC_STMT_CONSTS * 4, p.weights, p.l * 32);
    HIPCHK(hipMemcpyAsync(sl.q[3].p, st, sizeof st, hipMemcpyHostToDevice, sl.stream));
    HIPCHK(hipStreamSynchronize(sl.stream));             // (st is this frame's)
    return DGPU_OK;
}
// the rows [r0, r0 + rows) onto the device; C and D lie back to back, so that one MSM of the batch covers both
int32_t proofs_up(Slot &sl, const Proofs &p, size_t r0, size_t rows, smck::ProofDev &dev) {
    hipStream_t s = sl.stream;
    const size_t S = p.S(), D = p.D();
    HIPCHK(hipMemcpyAsync(sl.q[0].p, p.challenge + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[1].p, p.side_resp + 4 * S * r0, rows * S * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[4].p, p.commitments + 12 * r0, rows * PT, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[4].as<uint8_t>() + rows * PT, p.side_points + 12 * S * r0, rows * S * PT, hipMemcpyHostToDevice, s));
    if (D) {
        HIPCHK(hipMemcpyAsync(sl.q[2].p, p.digit_resp + 8 * D * r0, rows * D * 64, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sl.q[5].p, p.digit_points + 36 * D * r0, rows * D * 3 * PT, hipMemcpyHostToDevice, s));
    }
    dev = smck::ProofDev{sl.q[0].as<uint32_t>(), sl.q[1].as<uint32_t>(), sl.q[2].as<uint32_t>(), sl.q[3].as<uint32_t>(), p.sides, (int)p.l, p.mont ? 1 : 0};
    return DGPU_OK;
}
// every equation is a segment of four terms; the merged form adds 2 `extra` segments of `extra_len` terms behind them: the layout depends on the counts alone
void own_layout(size_t neq, size_t extra, size_t extra_len, SegLayout &lay) {
    std::vector<uint64_t> ends(neq + extra);
    for (size_t k = 0; k < neq; k++) ends[k] = 4 * (k + 1);
    for (size_t k = 0; k < extra; k++) ends[neq + k] = 4 * neq + extra_len * (k + 1);
    seg_layout(ends.data(), 0, ends.size(), lay);
}
void shared_words(const Proofs &p, uint64_t out[36]) {
    memcpy(out, p.g1, PT); memcpy(out + 12, p.ck_g, PT); memcpy(out + 24, p.ck_h, PT);
}

int32_t verify_each(const Proofs &p, const uint64_t *random, uint8_t *status, int32_t *detail) {
    if (p.n == 0) return DGPU_OK;
    if (bad_proofs(p) || !status) return DGPU_E_BADARG;
    if (random) for (size_t i = 0; i < p.n; i++) if (fr_is_zero(fr_in(random + 4 * i, p.mont))) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n, S = p.S(), D = p.D(), M = p.M();
    const bool merged = random && D;                     // (l = 0: there is no pairing to merge)
    const size_t xt = merged ? 2 * D : 0, xs = merged ? 2 : 0;      // the terms and segments a proof's merged check adds
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = chunk_rows(n, smck::SMC_EACH_SLICES, D ? D : S), cols = merged ? chunk : chunk * D;
    int32_t rc;
    SegLayout lay, lay_tail;
    own_layout(M * chunk, xs * chunk, D, lay);
    if (n % chunk) own_layout(M * (n % chunk), xs * (n % chunk), D, lay_tail);
    uint64_t shared[36];
    shared_words(p, shared);
    std::vector<int32_t> hdetail(detail ? 0 : chunk);
    // q[0] .. q[6]: the proofs and the scalars (ws_proofs; behind the own scalars the merged form's weights, twice); q[7]: the bases in segment order, then
    // [A' | -Abar] of every slice; q[8]: the merged form's [sum t A' | -sum t Abar] per proof; q[9]: [the slices' zero-point flags | the merged points' |
    // status], q[10]: detail, q[11]: the merged form's random_i
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, p, chunk))) return e;
        if ((e = o.q[6].ensure(chunk * (4 * M + 2 * D) * 32))) return e;
        if ((e = o.q[7].ensure(chunk * (4 * M + 2 * D) * PT))) return e;
        if ((e = o.q[8].ensure(2 * chunk * PT))) return e;
        if ((e = o.q[9].ensure(2 * chunk * D + 3 * chunk + 64))) return e;
        if ((e = o.q[10].ensure(chunk * 4))) return e;
        if ((e = o.q[11].ensure(chunk * 32))) return e;
        if (D && (e = ws_check(o, cols))) return e;
        return ws_seg_resident<G1>(o, (4 * M + xt) * chunk, (M + xs) * chunk, lay.blocks);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_bad = sl.flags.as<uint32_t>(), *d_own = sl.q[6].as<uint32_t>(), *d_bases = sl.q[7].as<uint32_t>();
    uint32_t *d_ma = sl.q[8].as<uint32_t>(), *d_mb = d_ma + chunk * (PT / 4);
    uint8_t *dsk = sl.q[9].as<uint8_t>(), *dmsk = dsk + 2 * chunk * D, *dstatus = dmsk + 2 * chunk;
    int32_t *ddetail = sl.q[10].as<int32_t>();
    if ((rc = statement_up(sl, p))) return rc;
    if (D && (rc = coeffs_up(sl, p.pk_pc, p.g2_pc, cols))) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        uint32_t *dPa = d_bases + 4 * M * rows * (PT / 4), *dPb = dPa + rows * D * (PT / 4);      // behind the equations' bases: the merged segments' bases
        smck::ProofDev dev;
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                          // (the own scalars are canonical: the flag stays clear; sl.flags takes the pairing's verdicts afterwards)
        if ((rc = proofs_up(sl, p, r0, rows, dev))) return rc;
        { StageTimer st(sl, "smc.own"); smck::launch_smc_own(s, dev, rows, d_own); }
        if (merged) {
            HIPCHK(hipMemcpyAsync(sl.q[11].p, random + 4 * r0, rows * 32, hipMemcpyHostToDevice, s));
            StageTimer st(sl, "smc.merge_weights");
            smck::launch_smc_merge_weights(s, sl.q[11].as<uint32_t>(), p.sides, (int)p.l, p.mont ? 1 : 0, rows, d_own + 4 * M * rows * 8);
        }
        { StageTimer st(sl, "smc.stage");
          smck::launch_smc_stage(s, sl.q[4].as<uint32_t>(), sl.q[4].as<uint32_t>() + rows * (PT / 4), sl.q[5].as<uint32_t>(), (const uint32_t *)shared, p.sides, (int)p.l, rows, d_bases,
                                 dPa, dPb, dsk); }
        if ((rc = seg_rows_resident<G1>(sl, (const uint8_t *)d_bases, PT, d_own, (4 * M + xt) * rows, (M + xs) * rows, rows == chunk ? lay : lay_tail, d_bad))) return rc;
        if (merged) {
            { StageTimer st(sl, "smc.merged_sides");
              smck::launch_smc_merged_sides(s, sl.win.as<uint32_t>() + M * rows * 36, sl.win_inf.as<uint8_t>() + M * rows, rows, d_ma, d_mb, dmsk); }
            launch_check(sl, d_ma, d_mb, dmsk, rows, cols);
        } else if (D) launch_check(sl, dPa, dPb, dsk, rows * D, cols);
        { StageTimer st(sl, "smc.verdict");
          smck::launch_smc_verdict(s, sl.win_inf.as<uint8_t>(), sl.flags.as<uint8_t>(), dsk, p.sides, (int)p.l, merged, rows, dstatus, ddetail); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(status + r0, dstatus, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(detail ? detail + r0 : hdetail.data(), ddetail, rows * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    return DGPU_OK;
}

// one verdict for n proofs: equation m of proof i weighs rho^(i M + m), the pairing of its digit d rho^(i S l + d)
int32_t verify_batch(const Proofs &p, const uint64_t *random, int32_t *ok) {
    if (p.n == 0) { if (ok) *ok = 1; return DGPU_OK; }
    if (bad_proofs(p) || !random || !ok) return DGPU_E_BADARG;
    if (fr_is_zero(fr_in(random, p.mont))) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t n = p.n, S = p.S(), D = p.D(), M = p.M();
    for (size_t k = 0; k < n * D; k++) if (zero_words(p.digit_points + 36 * k, 12)) { *ok = 0; return DGPU_OK; }      // InvalidProof: an A' is the identity
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = chunk_rows(n, smck::SMC_BATCH_EQS, M);
    const size_t nside = chunk * (1 + S), ndig = chunk * D;
    int32_t rc;
    uint64_t shared[36];
    shared_words(p, shared);
    // q[0] .. q[6]: the proofs and the own scalars (ws_proofs; q[4] is the merged verdict's scratch at the end); q[7]: the blocks' partial sums, q[8]: [the
    // shared points' coefficients | the running sums], q[9]: [rho^slice | -rho^slice], q[10]: the prepared records of the digits' points, q[11]: those of the two
    // pairing sides, q[12]: the shared points, q[13]: their prepared records, q[14]: the weights [over C and D | over the digits' points], q[15]: the records of C and D
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, p, chunk))) return e;
        if ((e = o.q[7].ensure(smck::smc_part_words(chunk, p.sides, (int)p.l) * 4))) return e;
        if ((e = o.q[8].ensure(3 * 32 + 3 * 40 + 64))) return e;
        if ((e = o.q[9].ensure(std::max<size_t>(2 * ndig * 32, 64)))) return e;
        if ((e = o.q[10].ensure(std::max<size_t>(3 * ndig * G1::AFF_STRIDE * 4, 64)))) return e;
        if ((e = o.q[11].ensure(std::max<size_t>(2 * ndig * G1::AFF_STRIDE * 4, 64)))) return e;
        if ((e = o.q[12].ensure(3 * PT))) return e;
        if ((e = o.q[13].ensure(3 * G1::AFF_STRIDE * 4))) return e;
        if ((e = o.q[14].ensure((nside + 3 * ndig) * 32))) return e;
        if ((e = o.q[15].ensure(nside * G1::AFF_STRIDE * 4))) return e;
        for (size_t terms : {3 * ndig, ndig, nside, (size_t)3}) if (terms && (e = ws_for<G1>(o, 2, terms, 0, nullptr))) return e;
        return ws_check(o, 1);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_own = sl.q[6].as<uint32_t>(), *d_c = sl.q[8].as<uint32_t>(), *d_run = d_c + 24, *d_tp = sl.q[9].as<uint32_t>(), *d_tn = d_tp + ndig * 8;
    uint32_t *d_wside = sl.q[14].as<uint32_t>(), *d_wdig = d_wside + nside * 8;
    uint32_t *d_rec = sl.q[10].as<uint32_t>(), *d_reca = sl.q[11].as<uint32_t>(), *d_recb = d_reca + ndig * G1::AFF_STRIDE, *d_recs = sl.q[13].as<uint32_t>(), *d_recside = sl.q[15].as<uint32_t>();
    HPoint Gsum = HPoint::identity(), P1 = HPoint::identity(), P2 = HPoint::identity();
    if ((rc = statement_up(sl, p))) return rc;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        smck::ProofDev dev;
        if ((rc = proofs_up(sl, p, r0, rows, dev))) return rc;
        const uint8_t *raw = sl.q[5].as<uint8_t>();
        { StageTimer st(sl, "msm.prep_bases");
          prep_g1(s, sl.q[4].p, PT, rows * (1 + S), d_recside);
          if (D) {
              prep_g1(s, raw, PT, 3 * D * rows, d_rec);
              prep_g1(s, raw, 3 * PT, D * rows, d_reca);
              prep_g1(s, raw + PT, 3 * PT, D * rows, d_recb);
          } }
        { StageTimer st(sl, "smc.own"); smck::launch_smc_own(s, dev, rows, d_own); }
        { StageTimer st(sl, "smc.columns");
          smck::launch_smc_columns(s, d_own, (const uint32_t *)random, p.sides, (int)p.l, p.mont ? 1 : 0, rows, r0, r0 == 0, sl.q[7].as<uint32_t>(), d_run, d_wside, d_wdig, d_tp, d_tn, d_c); }
        HIPCHK(hipGetLastError());
        if ((rc = msm_add(sl, d_recside, d_wside, rows * (1 + S), Gsum))) return rc;
        if (D) {
            if ((rc = msm_add(sl, d_rec, d_wdig, 3 * D * rows, Gsum))) return rc;
            if ((rc = msm_add(sl, d_reca, d_tp, D * rows, P1))) return rc;
            if ((rc = msm_add(sl, d_recb, d_tn, D * rows, P2))) return rc;
        }
        if (gs.prof) prof_flush(sl);
    }
    // the shared points' terms: ONE small MSM over g1, g, h with the finished coefficients
    if ((rc = shared_points_add(sl, shared, 3, sl.q[12], d_recs, d_c, Gsum))) return rc;
    if (!Gsum.inf || !D) { HIPCHK(hipStreamSynchronize(s)); guard.done = true; *ok = Gsum.inf ? 1 : 0; return DGPU_OK; }      // the G1 equation fails: the pairing cannot mend it (l = 0: there is none)
    if ((rc = merged_pair_verdict(sl, P1, P2, p.pk_pc, p.g2_pc, sl.q[4], ok))) return rc;
    guard.done = true;
    return DGPU_OK;
}

}  // namespace

extern "C" {
int32_t dgpu_smc_range_proofs_verify_each_g1(const uint64_t g1_xy[12], const uint64_t ck_g_xy[12], const uint64_t ck_h_xy[12], const uint64_t *pk_pc, const uint64_t *g2_pc,
                                             int32_t sides, size_t l, const uint64_t *weights, const uint64_t *side_consts, const uint64_t *commitments,
                                             const uint64_t *digit_points, const uint64_t *digit_responses, const uint64_t *side_points, const uint64_t *side_responses,
                                             const uint64_t *challenge, size_t n, int32_t montgomery, const uint64_t *random, uint8_t *status, int32_t *detail) {
    return abi_guard([&] {
        return verify_each(Proofs{g1_xy, ck_g_xy, ck_h_xy, pk_pc, g2_pc, sides, l, weights, side_consts, commitments, digit_points, digit_responses, side_points, side_responses,
                                  challenge, n, montgomery != 0}, random, status, detail);
    });
}
int32_t dgpu_smc_range_proofs_verify_batch_g1(const uint64_t g1_xy[12], const uint64_t ck_g_xy[12], const uint64_t ck_h_xy[12], const uint64_t *pk_pc, const uint64_t *g2_pc,
                                              int32_t sides, size_t l, const uint64_t *weights, const uint64_t *side_consts, const uint64_t *commitments,
                                              const uint64_t *digit_points, const uint64_t *digit_responses, const uint64_t *side_points, const uint64_t *side_responses,
                                              const uint64_t *challenge, size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok) {
    return abi_guard([&] {
        return verify_batch(Proofs{g1_xy, ck_g_xy, ck_h_xy, pk_pc, g2_pc, sides, l, weights, side_consts, commitments, digit_points, digit_responses, side_points, side_responses,
                                   challenge, n, montgomery != 0}, random, ok);
    });
}
}  // extern "C"
