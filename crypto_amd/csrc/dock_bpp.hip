// crypto_amd/csrc/dock_bpp.hip — Bulletproofs++ range proofs in bulk (include/dock_gpu_bpp.h, libdock_gpu_bpp.so: dgpu_bpp_range_proofs_verify_each_g1 /
// _verify_batch_g1): Proof::verify (bulletproofs_plus_plus/src/range_proof.rs:773-873) over WeightedNormLinearArgument::verify_given_commitment_multiplicands
// (weighted_norm_linear_argument.rs:213-238, :380-453), for many proofs of ONE shape over ONE resident setup [G, H_0 .. H_7, G_0 .. G_(NG-1)], each call ONE
// device pipeline per chunk of proofs.  A proof is ONE equation of 9 + NG terms over the setup and own = m + 4 + 2 K terms over its own points.
//   each    device  the per-proof constants (one inversion), the own scalars, the status-2 flag                                     k_bpp_consts
//           device  the 9 + NG scalars of every proof's row                                                                         k_bpp_shared
//           device  P_i = <row_i, setup>                                                             k_many_tree, k_many_fold (many_rows_resident over the setup's table)
//           device  the segment [V .., D, M, R, S, X .., R .., P_i] of every proof                                                  k_bpp_stage
//           device  one (own + 1)-term segment per proof                                             k_small_table, k_seg_tree, k_seg_fold (seg_rows_resident)
//           device  the status byte from the segment's identity flag and the status-2 flag                                          k_bpp_verdict
//   batch   device  constants and rows as above; the coefficients of the shared points and the own scalars times rho^i              k_bpp_col_sums, k_col_finish
//           device  one MSM over the chunk's own points; ONE over the setup at the end; the host adds the chunks' points and tests for the identity
// Only status bytes (each) or one verdict (batch) come back.  No pairing is run.  Nothing secret passes through: nothing is wiped.
#include "msm_many.hip.h"
#include "../../include/dock_gpu_bpp.h"
#include "bpp_launch.hip.h"
#include "acc_host_tables.hpp"
#include "pair_check.hip.h"
using namespace dock;
using namespace acch;

namespace {

// what the two calls share: the shape and the proofs' inputs
struct Proofs {
    uint64_t setup; uint32_t base, num_bits, m; const uint64_t *values, *round_points, *wnla_points, *l_n, *challenges; size_t n; bool mont;
};
// the argument checks that come before the device is looked at (n > 0), the handle apart
bool bad_proofs(const Proofs &p, bppk::ShapeInfo &sh) {
    if (!p.values || !p.round_points || !p.wnla_points || !p.l_n || !p.challenges || p.n >= (1ull << 31)) return true;
    sh = bppk::bpp_shape(p.base, p.num_bits, p.m);
    return !sh.ok;
}
bool setup_ok(const HandleRef &hb, const bppk::ShapeInfo &sh) { return hb.ok && hb.h.kind == 1 && hb.h.n == sh.shared; }
// q[0]: the challenges, q[1]: l0, n0, q[2]: V, q[3]: D, M, R, S, q[4]: X .., R .., q[5]: the record
int32_t ws_proofs(Slot &o, const Proofs &p, const bppk::ShapeInfo &sh, size_t chunk) {
    int32_t e;
    if ((e = o.q[0].ensure(chunk * (7 + sh.K) * 32))) return e;
    if ((e = o.q[1].ensure(chunk * 2 * 32))) return e;
    if ((e = o.q[2].ensure(chunk * p.m * PT))) return e;
    if ((e = o.q[3].ensure(chunk * 4 * PT))) return e;
    if ((e = o.q[4].ensure(chunk * 2 * sh.K * PT))) return e;
    return o.q[5].ensure(bppk::bpp_rec_words(chunk) * 4);
}
// the rows [r0, r0 + rows) onto the device
int32_t proofs_up(Slot &sl, const Proofs &p, const bppk::ShapeInfo &sh, size_t r0, size_t rows, bppk::ProofDev &dev) {
    hipStream_t s = sl.stream;
    const size_t nc = 7 + sh.K;
    HIPCHK(hipMemcpyAsync(sl.q[0].p, p.challenges + 4 * nc * r0, rows * nc * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[1].p, p.l_n + 8 * r0, rows * 64, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[2].p, p.values + 12 * p.m * r0, rows * p.m * PT, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[3].p, p.round_points + 48 * r0, rows * 4 * PT, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.q[4].p, p.wnla_points + 24 * sh.K * r0, rows * 2 * sh.K * PT, hipMemcpyHostToDevice, s));
    dev = bppk::ProofDev{sl.q[0].as<uint32_t>(), sl.q[1].as<uint32_t>(), p.base, p.num_bits, p.m, p.mont ? 1 : 0};
    return DGPU_OK;
}

int32_t verify_each(const Proofs &p, uint8_t *status) {
    if (p.n == 0) return DGPU_OK;
    bppk::ShapeInfo sh;
    if (bad_proofs(p, sh) || !status) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    HandleRef hb(p.setup);
    if (!setup_ok(hb, sh)) return DGPU_E_BADARG;                         // (a handle exists only where a device does)
    const size_t n = p.n, T = sh.own + 1;
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const RowMsm<G1> bp = param_rows<G1>(sl, p.setup, hb.h, sh.shared, bppk::BPP_EACH_CHUNK, n);
    const size_t chunk = bp.chunk;
    int32_t rc;
    SegLayout lay, lay_tail;
    row_layout(chunk, T, 0, lay);                                        // one segment of T terms per proof
    if (n % chunk) row_layout(n % chunk, T, 0, lay_tail);
    // q[0] .. q[5]: the proofs and the record (ws_proofs); q[6]: the own scalars and the one behind them, q[7]: the segments' bases, q[8]: [P | identity flags],
    // q[9]: [status-2 flags | status]
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, p, sh, chunk))) return e;
        if ((e = o.q[6].ensure(chunk * T * 32))) return e;
        if ((e = o.q[7].ensure(chunk * T * PT))) return e;
        if ((e = o.q[8].ensure(chunk * PT + chunk))) return e;
        if ((e = o.q[9].ensure(2 * chunk + 64))) return e;
        if ((e = ws_seg_resident<G1>(o, T * chunk, chunk, lay.blocks))) return e;
        return bp.workspace(o);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_rows = sl.in_scalars.as<uint32_t>(), *d_bad = sl.flags.as<uint32_t>(), *d_rec = sl.q[5].as<uint32_t>(), *d_own = sl.q[6].as<uint32_t>(), *d_bases = sl.q[7].as<uint32_t>();
    uint8_t *dP = sl.q[8].as<uint8_t>(), *dPinf = dP + chunk * PT, *dflag = sl.q[9].as<uint8_t>(), *dstatus = dflag + chunk;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        bppk::ProofDev dev;
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));                          // (the scalars are canonical: the flag stays clear)
        if ((rc = proofs_up(sl, p, sh, r0, rows, dev))) return rc;
        { StageTimer st(sl, "bpp.consts"); bppk::launch_bpp_consts(s, dev, rows, d_rec, T, d_own, dflag); }
        { StageTimer st(sl, "bpp.shared"); bppk::launch_bpp_shared(s, dev, rows, d_rec, d_rows); }
        if ((rc = bp.points(sl, d_rows, rows, d_bad, dP, dPinf))) return rc;
        { StageTimer st(sl, "bpp.stage");
          bppk::launch_bpp_stage(s, dev, sl.q[2].as<uint32_t>(), sl.q[3].as<uint32_t>(), sl.q[4].as<uint32_t>(), (const uint32_t *)dP, dPinf, rows, d_bases); }
        if ((rc = seg_rows_resident<G1>(sl, (const uint8_t *)d_bases, PT, d_own, T * rows, rows, rows == chunk ? lay : lay_tail, d_bad))) return rc;
        { StageTimer st(sl, "bpp.verdict"); bppk::launch_bpp_verdict(s, sl.win_inf.as<uint8_t>(), dflag, rows, dstatus); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(status + r0, dstatus, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    return DGPU_OK;
}

// one verdict for n proofs: proof i weighs rho^i
int32_t verify_batch(const Proofs &p, const uint64_t *random, int32_t *ok) {
    if (p.n == 0) { if (ok) *ok = 1; return DGPU_OK; }
    bppk::ShapeInfo sh;
    if (bad_proofs(p, sh) || !random || !ok) return DGPU_E_BADARG;
    if (fr_is_zero(fr_in(random, p.mont))) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    HandleRef hb(p.setup);
    if (!setup_ok(hb, sh)) return DGPU_E_BADARG;                         // (a handle exists only where a device does)
    const size_t n = p.n, own = sh.own, cols = sh.shared;
    CtxScope on_owner(hb.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = chunk_rows(n, bppk::BPP_BATCH_POINTS, own);
    int32_t rc;
    // q[0] .. q[5]: the proofs and the record (ws_proofs); q[6]: the own scalars, q[7]: the blocks' partial sums, q[8]: [the shared points' coefficients | the
    // running sums], q[9]: the status-2 flags, q[10]: the prepared records of the own points, q[11]: the weights over them, q[12]: the proofs' rows
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = ws_proofs(o, p, sh, chunk))) return e;
        if ((e = o.q[6].ensure(chunk * own * 32))) return e;
        if ((e = o.q[7].ensure(bppk::bpp_part_words(chunk, cols) * 4))) return e;
        if ((e = o.q[8].ensure(cols * 32 + cols * 40 + 64))) return e;
        if ((e = o.q[9].ensure(chunk + 64))) return e;
        if ((e = o.q[10].ensure(chunk * own * G1::AFF_STRIDE * 4))) return e;
        if ((e = o.q[11].ensure(chunk * own * 32))) return e;
        if ((e = o.q[12].ensure(chunk * cols * 32))) return e;
        for (size_t terms : {chunk * own, cols}) if ((e = ws_for<G1>(o, 2, terms, 0, nullptr))) return e;
        return o.flags.ensure(64);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    DrainUnlessDone guard(sl);
    uint32_t *d_recd = sl.q[5].as<uint32_t>(), *d_own = sl.q[6].as<uint32_t>(), *d_c = sl.q[8].as<uint32_t>(), *d_run = d_c + cols * 8, *d_rec = sl.q[10].as<uint32_t>();
    uint32_t *d_w = sl.q[11].as<uint32_t>(), *d_rows = sl.q[12].as<uint32_t>();
    uint8_t *dflag = sl.q[9].as<uint8_t>();
    std::vector<uint8_t> hflag(chunk);
    HPoint sum = HPoint::identity();
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        bppk::ProofDev dev;
        if ((rc = proofs_up(sl, p, sh, r0, rows, dev))) return rc;
        { StageTimer st(sl, "msm.prep_bases");
          prep_g1(s, sl.q[2].p, PT, rows * p.m, d_rec);
          prep_g1(s, sl.q[3].p, PT, rows * 4, d_rec + rows * p.m * G1::AFF_STRIDE);
          prep_g1(s, sl.q[4].p, PT, rows * 2 * sh.K, d_rec + rows * (p.m + 4) * G1::AFF_STRIDE); }
        { StageTimer st(sl, "bpp.consts"); bppk::launch_bpp_consts(s, dev, rows, d_recd, own, d_own, dflag); }
        { StageTimer st(sl, "bpp.shared"); bppk::launch_bpp_shared(s, dev, rows, d_recd, d_rows); }
        { StageTimer st(sl, "bpp.columns");
          bppk::launch_bpp_columns(s, dev, d_rows, d_own, (const uint32_t *)random, rows, r0, r0 == 0, sl.q[7].as<uint32_t>(), d_run, d_w, d_c); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hflag.data(), dflag, rows, hipMemcpyDeviceToHost, s));
        if ((rc = msm_add(sl, d_rec, d_w, rows * own, sum))) return rc;
        HIPCHK(hipStreamSynchronize(s));                                 // (hflag is this frame's; the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
        for (size_t i = 0; i < rows; i++) if (hflag[i]) { guard.done = true; *ok = 0; return DGPU_OK; }      // a proof of status 2 refuses the batch
    }
    // the shared points' terms: ONE MSM over the setup with the finished coefficients
    if ((rc = params_msm(sl, p.setup, hb.h, d_c, cols, sum))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    guard.done = true;
    *ok = sum.inf ? 1 : 0;
    return DGPU_OK;
}

}  // namespace

extern "C" {
int32_t dgpu_bpp_range_proofs_verify_each_g1(uint64_t setup, uint32_t base, uint32_t num_bits, uint32_t m, const uint64_t *values, const uint64_t *round_points,
                                             const uint64_t *wnla_points, const uint64_t *l_n, const uint64_t *challenges, size_t n, int32_t montgomery, uint8_t *status) {
    return abi_guard([&] { return verify_each(Proofs{setup, base, num_bits, m, values, round_points, wnla_points, l_n, challenges, n, montgomery != 0}, status); });
}
int32_t dgpu_bpp_range_proofs_verify_batch_g1(uint64_t setup, uint32_t base, uint32_t num_bits, uint32_t m, const uint64_t *values, const uint64_t *round_points,
                                              const uint64_t *wnla_points, const uint64_t *l_n, const uint64_t *challenges, size_t n, int32_t montgomery, const uint64_t random[4],
                                              int32_t *ok) {
    return abi_guard([&] { return verify_batch(Proofs{setup, base, num_bits, m, values, round_points, wnla_points, l_n, challenges, n, montgomery != 0}, random, ok); });
}
}  // extern "C"
