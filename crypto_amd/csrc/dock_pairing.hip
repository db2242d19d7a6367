// crypto_amd/csrc/dock_pairing.hip — dgpu_multi_miller_loop / dgpu_final_exponentiation (include/dock_gpu.h).
//
// Bls12_381::multi_miller_loop(a, b) (utils/src/randomized_pairing_check.rs:207, legogroth16/src/verifier.rs:69-76)
// computes f = conj( prod_i f_i ), f_i the 63-step double-and-add Miller function of pair i.  arkworks shares the
// 63 squarings inside rayon chunks of 4 pairs.  Because squaring distributes over products, the same value is
//      f = conj( (...((L_0)^2 L_1)^2 ...) ),   L_s = prod_i line_{i,s}(P_i)        (68 steps: 63 doublings + 5 additions)
// so the batch splits into three parts that match the hardware:
//   K9  k_miller_lines    one lane per pair: G2Prepared::from(Q_i) fused with the evaluation at P_i -> 68 sparse lines
//   K10 k_line_products   one lane per (step, slice of pairs): sparse accumulation with mul_by_014
//   K11 k_product_tree    one block per step: dense Fp12 product tree through LDS -> L_s in ABI form
//   host                  131 Fp12 operations (63 squarings + 68 products) + conjugation: 0.25 ms on one core, where a
//                         lone GPU wave would need ~70 us per dense product
// Pairs with an identity member contribute the neutral line (1, 0, 0), which is what arkworks' filter amounts to.
#include "dock_ctx.hpp"
#include "host_field.hpp"
#include "pairing_launch.hip.h"
#include "fixed_launch.hip.h"
#include "gt_launch.hip.h"
#include <thread>
#include <functional>
#include <optional>
#include <atomic>

namespace {
using namespace dock;
using namespace mlk;

// Slices of pairs per step.  A lane multiplies its slice's lines into one partial (sparse products, serial), then 64-wide trees fold
// the partials (dense products, log depth): short slices keep both latency-bound phases short at small n and fill the chip at large n
// (a fixed 64 slices left k_line_products with 4352 lanes whatever n: 59 ms at 2^16 pairs).
inline int choose_slice_len(size_t n) {
    size_t len = n > 2048 ? 8 : (n > 512 ? 4 : 2);      // (measured with the 18-role tree: 2 wins up to 512 pairs, 4 at 1024, 8 from 4096)
    while ((n + len - 1) / len > 2048 && (n + len - 1) / len > 0) len *= 2;
    return (int)len;
}
// Slices of a (segment, step) of several loops over one line buffer.  Up to 64 slices of 4 (8) pairs fold in one tree level; a longer segment keeps slices of 8 and
// takes a second level (<= 8192 pairs per segment here: <= 1024 slices, 16 groups) — with one level its slices grew to 16 / 32 pairs, i.e. a quarter of the lanes on
// chains four times as long (the commitments of a 1024-proof aggregation: 2 x 2048 + 4 x 1024 pairs on 276 waves per piece).
inline int choose_segment_slice_len(size_t maxlen) {
    int len = 4;
    if (maxlen > 4 * (size_t)MAX_SLICES) len = 8;
    while ((maxlen + len - 1) / len > (size_t)MAX_SLICES * MAX_SLICES) len *= 2;
    return len;
}

}  // namespace

extern "C" {

// conj((...((L_0)^2 L_1)^2 ...)) over the 68 per-step products; may be taken in pieces (bits 62 .. b_lo, then on to 0)
struct MlTail {
    hostf::Fq12 f = hostf::Fq12::one(); int idx = 0, b = 62;
    void run(const hostf::Fq12 *L, int b_lo) { for (; b >= b_lo; b--) { f = f.sqr() * L[idx++]; if ((hostf::BLS_X_ABS >> b) & 1) f = f * L[idx++]; } }
    hostf::Fq12 result() const { return f.conj(); }      // x < 0
};

// How the products of nseg loops over one line buffer are cut: segment g is the pairs [seg_off[g], seg_off[g + 1]) (device words; one loop over all the
// pairs: nseg = 1, seg_off = nullptr), every (segment, step) has nsl slices of slice_len pairs — of the longest segment — folded in groups of MAX_SLICES.
// base: first word of this geometry's partials in sl.ml_partial
struct MlGeom { int slice_len, nsl, ngroups; size_t base; int nseg; const uint32_t *seg_off; };
static MlGeom ml_geom(size_t len, int slice_len, size_t base = 0, int nseg = 1, const uint32_t *seg_off = nullptr) {
    const int nsl = (int)((len + slice_len - 1) / slice_len);        // <= 2048, so <= 32 groups: the second tree level is one group
    return MlGeom{slice_len, nsl, (nsl + MAX_SLICES - 1) / MAX_SLICES, base, nseg, seg_off};
}
static MlGeom ml_single(size_t n) { return ml_geom(n, choose_slice_len(n)); }
static size_t ml_geom_words(const MlGeom &g) { return (size_t)N_LINES * g.nseg * (g.nsl + (g.ngroups > 1 ? g.ngroups : 0)) * F12W; }
// room for the partials of both geometries (they may be the same one) and for the results
static int32_t ml_ensure(Slot &sl, const MlGeom &a, const MlGeom &b) {
    int32_t rc;
    if ((rc = sl.ml_partial.ensure(std::max(a.base + ml_geom_words(a), b.base + ml_geom_words(b)) * 4))) return rc;
    return sl.ml_out.ensure((size_t)N_LINES * a.nseg * 144 * 4);
}
// K10 + K11 for the steps s0 .. s0 + ns - 1 of every segment on stream s (partials and results are indexed by the step: disjoint for disjoint ranges);
// one or two tree levels, the second sees the groups as slices of MAX_SLICES * slice_len pairs.  The only place that launches them.
static void ml_products(Slot &sl, hipStream_t s, size_t n, const MlGeom &g, int s0, int ns, bool timed, const uint32_t *pxy, bool allow3) {
    const int mode = gs.ml_mode.load();
    uint32_t *lvl0 = sl.ml_partial.as<uint32_t>() + g.base, *lvl1 = lvl0 + (size_t)N_LINES * g.nseg * g.nsl * F12W, *out = sl.ml_out.as<uint32_t>();
    const unsigned nodes = (unsigned)(ns * g.nseg);
    std::optional<StageTimer> st;                                    // (stage timers record on sl.stream)
    if (timed) st.emplace(sl, "ml.products");
    launch_line_products(s, mode, sl.ml_lines.as<uint32_t>(), n, g.slice_len, g.nsl, lvl0, g.seg_off, g.nseg, s0, ns, pxy, allow3);
    st.reset();
    if (timed) st.emplace(sl, "ml.tree");
    if (g.ngroups == 1) { launch_product_tree(s, mode, nodes, lvl0, g.nsl, 1, nullptr, out, g.seg_off, g.slice_len, s0, ns); return; }
    launch_product_tree(s, mode, nodes * g.ngroups, lvl0, g.nsl, g.ngroups, lvl1, nullptr, g.seg_off, g.slice_len, s0, ns);
    launch_product_tree(s, mode, nodes, lvl1, g.ngroups, 1, nullptr, out, g.seg_off, g.slice_len * MAX_SLICES, s0, ns);
}
// segment g's value from its N_LINES per-step products (an empty segment — off given, off[g] == off[g + 1] — yields one), then done(out), if given
typedef std::function<void(uint64_t *)> MlDone;
static void ml_put(uint64_t *out, const hostf::Fq12 &f, const MlDone &done) { memcpy(out, &f, sizeof f); if (done) done(out); }
static size_t ml_tail_threads(size_t nseg) { return std::min<size_t>(std::min<size_t>(nseg, 16), std::max<size_t>(1, std::thread::hardware_concurrency())); }
// K10 + K11 in one launch each over every segment + the host tails (on the library's threads when there are several) on the lines already in sl.ml_lines:
// out + 72 g = the value of segment g.  off: the segments' bounds on the host
static int32_t ml_finish(Slot &sl, size_t n, const MlGeom &g, uint64_t *out, const uint32_t *pxy = nullptr, bool allow3 = true, const uint32_t *off = nullptr, const MlDone &done = nullptr) {
    int32_t rc;
    if ((rc = ml_ensure(sl, g, g))) return rc;
    hipStream_t s = sl.stream;
    ml_products(sl, s, n, g, 0, N_LINES, true, pxy, allow3);
    HIPCHK(hipGetLastError());
    const size_t nseg = (size_t)g.nseg, T = ml_tail_threads(nseg);
    std::vector<hostf::Fq12> L((size_t)N_LINES * nseg);
    HIPCHK(hipMemcpyAsync(L.data(), sl.ml_out.p, (size_t)N_LINES * nseg * 576, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (gs.prof) prof_flush(sl);
    return par_run(T, [&](size_t k) -> int32_t {
        for (size_t i = k; i < nseg; i += T) {
            const bool empty = off && off[i + 1] == off[i];
            MlTail t; if (!empty) t.run(&L[i * N_LINES], 0);
            ml_put(out + i * 72, empty ? hostf::Fq12::one() : t.result(), done);
        }
        return DGPU_OK; });
}

// A call of up to 8192 pairs lasts as long as its chain: 68 dependent line steps (K9: the chip nearly empty), then the product levels of
// K10 / K11 (~0.18 ms whatever the number of steps), then 131 Fp12 operations on the host (~0.25 ms: as long as the chain itself since K9
// has sixteen lanes per pair).  The chain is therefore cut into ML_PIECES launches at the bits ML_CUTS of |x|: the products of a finished
// piece run on a stream of their own while the next piece is computed, its results land in pinned memory and the host folds them into f
// as they arrive — what is left after the last launch is the product levels of the last piece and its share of the host's work.  Same
// values in the same order: bit-identical to the one-launch form, which stays for larger batches (throughput-bound) and while stage
// timers are on.  (Round 3: two pieces, cut at bit 17; 1.45 -> 1.05 ms at 1024 pairs.  Three pieces with sixteen lanes: 0.7.)
constexpr int ML_PIECES = 3;
constexpr int ML_CUTS[ML_PIECES] = {40, 17, 0};               // piece j runs the bits (ML_CUTS[j - 1] - 1, or 62) .. ML_CUTS[j]
struct MlCuts {
    int at[ML_PIECES];
    explicit MlCuts(int mode) {                                   // development twin: dgpu_set_miller_pipeline's bits 8 - 13 and 16 - 21 move the cuts
        const int a = (mode >> 8) & 63, b = (mode >> 16) & 63, moved = a > b && b > 0 && a < 62;
        for (int j = 0; j < ML_PIECES; j++) at[j] = moved && j == 0 ? a : (moved && j == 1 ? b : ML_CUTS[j]);
    }
};
// whatever happens between its construction and its end, nothing of the call stays in flight on the slot's three streams
struct MlDrain {
    Slot &sl; bool drained = false;
    hipError_t now() {
        const hipError_t e0 = hipStreamSynchronize(sl.stream), e1 = hipStreamSynchronize(sl.cstream), e2 = hipStreamSynchronize(sl.xstream);
        drained = true;
        return e0 != hipSuccess ? e0 : (e1 != hipSuccess ? e1 : e2);
    }
    ~MlDrain() { if (!drained) (void)now(); }
};
// The piece scheduler.  n pairs in the line buffer, the first n_aff of them affine (their chain is what gets cut); prepared(pxy) queues the line kernel of
// the prepared pairs n_aff .. n - 1, if any, on the slot's stream (it writes their neutral px, py).
// late(side_stream, pxy), if given, runs on the calling thread once every piece of the chain has been queued — host work that the chain hides
// (the verifier computes its third G1 operand meanwhile) — and may queue, on side_stream, whatever must precede the product kernels (the line
// kernel of prepared pairs whose P was not known before).
// p_late: the affine pairs' P are not known when the chain starts (dgpu_multi_miller_loop_scaled: they are being scaled meanwhile) — the line kernel gets
// no P and leaves px, py alone; `late` must write them (pxy[(c FPW + k) n + i], the internal form) before the product kernels run.
// The products of the pieces alternate between the side streams (a piece's products outlast the next piece's chain), the last piece's — cut by `last` —
// stay on the slot's stream; the results of (segment g, step s) land in L[g * N_LINES + s] (pinned).  fold(done) then runs on the calling thread: done[j] is
// recorded behind piece j's results.  Every stream is drained before this returns.
typedef std::function<void(uint32_t *)> MlPrepared;
typedef std::function<int32_t(hipStream_t, uint32_t *)> MlLate;
static int32_t ml_run_pieces(Slot &sl, size_t n, size_t n_aff, const uint8_t *dskip, const MlGeom &head, const MlGeom &last, const MlCuts &cuts, hostf::Fq12 *L, const MlPrepared &prepared, const MlLate &late, bool p_late, const std::function<int32_t(const hipEvent_t *)> &fold) {
    int32_t rc;
    if ((rc = ml_ensure(sl, head, last))) return rc;
    if ((rc = sl.ml_state.ensure(((size_t)STATE_W * n_aff + (size_t)PXY_W * n) * 4))) return rc;      // R of every lane, then px, py of every pair
    hipStream_t sa = sl.stream, side[2] = {sl.cstream, sl.xstream};
    // ready and done of every piece but the last one's ready, `late`, and one event of the caller's (dgpu_legogroth16_verify)
    static_assert(2 * ML_PIECES - 1 + 1 + 1 <= Slot::N_COPY_EV + 1, "events");
    auto event = [&] { return sl.copy_ev[sl.ev_next++ % (Slot::N_COPY_EV + 1)]; };
    uint32_t *state = sl.ml_state.as<uint32_t>(), *pxy = state + (size_t)STATE_W * n_aff;
    const int mode = gs.ml_mode.load(), nseg = head.nseg;
    // (a failed enqueue must not leave the slot with work in flight: every step is checked, and `drain` holds on every way out)
    MlDrain drain{sl};
    auto ok = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = DGPU_E_HIP; return rc == DGPU_OK; };
    prepared(pxy);
    hipEvent_t done[ML_PIECES] = {}, ready[ML_PIECES - 1] = {};
    int first_step[ML_PIECES], steps[ML_PIECES];
    { int s_first = 0, b_hi = 62;                                        // the whole chain first: its launches depend on nothing but each other
      for (int j = 0; j < ML_PIECES && !rc; j++) {
          const int b_lo = cuts.at[j], ns = chain_steps(b_hi, b_lo);
          first_step[j] = s_first; steps[j] = ns;
          launch_lines_uneval(sa, mode, p_late ? (const uint32_t *)nullptr : sl.in_bases.as<uint32_t>(), sl.in_scalars.as<uint32_t>(), dskip, n_aff, sl.ml_lines.as<uint32_t>(), n, b_hi, b_lo, s_first, state, p_late ? (uint32_t *)nullptr : pxy);
          if (j + 1 < ML_PIECES) { ready[j] = event(); ok(hipEventRecord(ready[j], sa)); }
          s_first += ns; b_hi = b_lo - 1;
      } }
    if (late && !rc && !(rc = late(side[0], pxy))) {
        hipEvent_t late_done = event();
        ok(hipEventRecord(late_done, side[0])); ok(hipStreamWaitEvent(side[1], late_done, 0)); ok(hipStreamWaitEvent(sa, late_done, 0));
    }
    for (int j = 0; j < ML_PIECES && !rc; j++) {
        const bool is_last = j + 1 == ML_PIECES;
        hipStream_t sp = is_last ? sa : side[j & 1];
        if (!is_last && !ok(hipStreamWaitEvent(sp, ready[j], 0))) break;
        const int s0 = first_step[j], ns = steps[j];
        ml_products(sl, sp, n, is_last ? last : head, s0, ns, false, pxy, true);
        const char *src = (const char *)sl.ml_out.p + (size_t)s0 * 576;
        if (nseg == 1) ok(hipMemcpyAsync(L + s0, src, (size_t)ns * 576, hipMemcpyDeviceToHost, sp));
        else ok(hipMemcpy2DAsync(L + s0, (size_t)N_LINES * 576, src, (size_t)N_LINES * 576, (size_t)ns * 576, (size_t)nseg, hipMemcpyDeviceToHost, sp));
        done[j] = event(); ok(hipEventRecord(done[j], sp));
    }
    ok(hipGetLastError());
    if (!rc) { const int32_t frc = fold(done); if (frc) rc = frc; }
    ok(drain.now());
    return rc;
}
// one loop, pipelined: the calling thread folds the pieces as they arrive
static int32_t ml_pipelined(Slot &sl, size_t n, size_t n_aff, const uint8_t *dskip, uint64_t *out, const MlPrepared &prepared, const MlLate &late = nullptr, bool p_late = false) {
    const int mode = gs.ml_mode.load();
    const MlCuts cuts(mode); const MlGeom g = ml_single(n);
    // the last steps' products are all that is left when the chain ends: from 8-pair slices on they take half the slice length (fewer
    // sparse products in front of the tree, more tree for a quarter of the steps: 1.46 -> 1.39 ms at 4096 pairs; measured the other way
    // round at 1024 pairs, 4 -> 2: 1.06 -> 1.14)
    int tail_slice = g.slice_len >= 8 && (n + g.slice_len / 2 - 1) / (g.slice_len / 2) <= 2048 ? g.slice_len / 2 : g.slice_len;
    { const int v = (mode >> 24) & 15;                                // development twin: the slice length of the last piece
      if (v >= 1 && (n + v - 1) / v <= 2048) tail_slice = v; }
    static_assert((size_t)N_LINES * 576 <= Slot::HPIN_BYTES, "pinned scratch");
    hostf::Fq12 *L = (hostf::Fq12 *)sl.hpin;                          // pinned: the copies are asynchronous for the host
    MlTail tail;
    const int32_t rc = ml_run_pieces(sl, n, n_aff, dskip, g, ml_geom(n, tail_slice, ml_geom_words(g)), cuts, L, prepared, late, p_late, [&](const hipEvent_t *done) -> int32_t {
        for (int j = 0; j < ML_PIECES; j++) { if (hipEventSynchronize(done[j]) != hipSuccess) return DGPU_E_HIP; tail.run(L, cuts.at[j]); }
        return DGPU_OK; });
    if (!rc) ml_put(out, tail.result(), nullptr);
    return rc;
}
// how many Miller loops are in flight on the context (the two-launch form needs the slot's second stream and an event wait between the
// two; with more streams than hardware queues a waiting stream holds up whatever shares its queue — measured, 1024 pairs: 0.62 vs 0.70 ms
// per call with two calls in flight, but 0.49 vs 0.36 with six — so it is taken while at most two are in flight)
struct MlActive { std::atomic<int> &c; int v; explicit MlActive(std::atomic<int> &c_) : c(c_), v(++c_) {} ~MlActive() { --c; } MlActive(const MlActive &) = delete; };

// The workspace of a call's pairs and their way to the device, on the slot's stream: n_aff affine pairs (P, Q, skip) in front, n_prep prepared ones
// (P, coefficients, skip) behind them.  p_aff == nullptr: the affine pairs' P come later.  inf_extra: bytes the caller wants behind the skip flags
static int32_t ml_upload(Slot &sl, const uint64_t *p_aff, const uint64_t *q_aff, const uint8_t *skip_aff, size_t n_aff, const uint64_t *p_prep, const uint64_t *coeffs, const uint8_t *skip_prep, size_t n_prep, size_t inf_extra = 0) {
    int32_t rc;
    const size_t n = n_aff + n_prep, cbytes = n_prep * (size_t)DGPU_G2_PREPARED_WORDS * 8;
    if ((rc = sl.in_bases.ensure(n * 96))) return rc;
    if (n_aff && (rc = sl.in_scalars.ensure(n_aff * 192 + 16))) return rc;
    if ((rc = sl.in_inf.ensure(n + inf_extra))) return rc;
    if (n_prep && (rc = sl.ml_coeffs.ensure(cbytes + 16))) return rc;
    if ((rc = sl.ml_lines.ensure((size_t)N_LINES * LW * n * 4))) return rc;
    hipStream_t s = sl.stream; uint32_t *dp = sl.in_bases.as<uint32_t>(); uint8_t *dsk = sl.in_inf.as<uint8_t>();
    if (n_aff) {
        if (p_aff) HIPCHK(hipMemcpyAsync(dp, p_aff, n_aff * 96, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sl.in_scalars.p, q_aff, n_aff * 192, hipMemcpyHostToDevice, s));
        if (skip_aff) HIPCHK(hipMemcpyAsync(dsk, skip_aff, n_aff, hipMemcpyHostToDevice, s));
    }
    if (n_prep) {
        HIPCHK(hipMemcpyAsync(dp + n_aff * 24, p_prep, n_prep * 96, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sl.ml_coeffs.p, coeffs, cbytes, hipMemcpyHostToDevice, s));
        if (skip_prep) HIPCHK(hipMemcpyAsync(dsk + n_aff, skip_prep, n_prep, hipMemcpyHostToDevice, s));
    }
    return DGPU_OK;
}

// the line kernel of the prepared pairs n_aff .. n_aff + n_prep - 1 as ml_upload laid them out, on the slot's stream; pxy: their neutral px, py, for a product kernel that evaluates
static void ml_prepared_lines(Slot &sl, size_t n_aff, size_t n_prep, bool skip, uint32_t *pxy) {
    if (!n_prep) return;
    launch_lines_from_prepared(sl.stream, sl.in_bases.as<uint32_t>() + n_aff * 24, sl.ml_coeffs.as<uint32_t>(), skip ? sl.in_inf.as<uint8_t>() + n_aff : nullptr, n_prep,
                               sl.ml_lines.as<uint32_t>() + n_aff, n_aff + n_prep, pxy ? pxy + n_aff : nullptr);
}

int32_t dgpu_multi_miller_loop(const uint64_t *p, const uint64_t *q, const uint8_t *skip, size_t n, uint64_t *out) {
    if (!out || (n && (!p || !q))) return DGPU_E_BADARG;
    if (n == 0) { hostf::Fq12 one = hostf::Fq12::one(); memcpy(out, &one, sizeof one); return DGPU_OK; }
    if (n >= (1ull << 24)) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    if ((rc = ml_upload(sl, p, q, skip, n, nullptr, nullptr, nullptr, 0))) return rc;
    hipStream_t s = sl.stream;
    const uint8_t *dskip = skip ? sl.in_inf.as<uint8_t>() : nullptr;
    const MlGeom g = ml_single(n);
    { StageTimer st(sl, "ml.lines");
#ifdef DGPU_DEV
      static const bool one_lane = getenv("DGPU_ML_ONE_LANE") != nullptr;     // development switches: one lane / one lane pair per (P, Q)
      static const bool two_lanes = getenv("DGPU_ML_TWO_LANES") != nullptr;
#else
      constexpr bool one_lane = false, two_lanes = false;
#endif
      const int mode = gs.ml_mode.load();
      if (!one_lane && !two_lanes && n <= 8192 && !gs.prof && (mode & 1)) {
          // Either way the evaluation at P is left to the product kernel.
          MlActive act(cur().ml_active);
          if (act.v <= 2) return ml_pipelined(sl, n, n, dskip, out, [](uint32_t *) {});
          if ((rc = sl.ml_state.ensure((size_t)PXY_W * n * 4))) return rc;
          uint32_t *pxy = sl.ml_state.as<uint32_t>();
          launch_lines_uneval(s, mode, sl.in_bases.as<uint32_t>(), sl.in_scalars.as<uint32_t>(), dskip, n, sl.ml_lines.as<uint32_t>(), n, 62, 0, 0, nullptr, pxy);
          return ml_finish(sl, n, g, out, pxy);
      }
      // (with the chip full, the pair form does less total work)
      launch_lines_eval(s, sl.in_bases.as<uint32_t>(), sl.in_scalars.as<uint32_t>(), dskip, n, sl.ml_lines.as<uint32_t>(), n, one_lane ? 1 : (two_lanes || n > 8192 ? 2 : 4));
    }
    return ml_finish(sl, n, g, out);
}

// nseg independent Miller loops in one call: segment g is the pairs [seg_end[g - 1], seg_end[g]) (seg_end ascending, seg_end[nseg - 1] == n;
// an empty segment yields one).  The ten `E::multi_pairing` calls of a GIPA round (legogroth16/src/aggregation/commitment.rs:30-31,54-67,
// aggregation/utils.rs:95-96, issued one after another in the reference) have 1 ... n/2 pairs each, and every launch of the line kernel lasts as
// long as its 68 dependent steps whatever the pair count: one line launch over all the pairs, one product launch and one tree launch over
// (segment, step), the nseg host tails on host threads.  out_f12: nseg x 72 words, each limb for limb what dgpu_multi_miller_loop
// returns for that segment alone.
static int32_t ml_segments(const uint64_t *p, const uint64_t *q, const uint8_t *skip, size_t n, const uint64_t *seg_end, size_t nseg, uint64_t *out, bool final_exp) {
    if (!out || !seg_end || nseg == 0 || (n && (!p || !q)) || n >= (1ull << 24) || nseg > 4096) return DGPU_E_BADARG;
    size_t maxlen = 0;
    { uint64_t prev = 0; for (size_t g = 0; g < nseg; g++) { if (seg_end[g] < prev || seg_end[g] > n) return DGPU_E_BADARG; maxlen = std::max<size_t>(maxlen, seg_end[g] - prev); prev = seg_end[g]; }
      if (prev != n) return DGPU_E_BADARG; }
    // (a Miller output of valid operands is never zero; arkworks' multi_pairing unwraps the Option — here a zero is DGPU_E_ZERO for the call)
    std::atomic<bool> zero{false};
    const MlDone finish = [&](uint64_t *o) {
        if (!final_exp) return;
        hostf::Fq12 f, r; memcpy(&f, o, sizeof f);
        if (!hostf::final_exponentiation(r, f)) { zero = true; return; }
        memcpy(o, &r, sizeof r);
    };
    if (nseg == 1 || maxlen > 8192) {                      // long segments fill the chip on their own: one call each
        uint64_t prev = 0;
        for (size_t g = 0; g < nseg; g++) {
            const int32_t rc = dgpu_multi_miller_loop(p + prev * 12, q + prev * 24, skip ? skip + prev : nullptr, seg_end[g] - prev, out + g * 72);
            if (rc) return rc;
            finish(out + g * 72);
            prev = seg_end[g];
        }
        return zero ? DGPU_E_ZERO : DGPU_OK;
    }
    const hostf::Fq12 one = hostf::Fq12::one();
    if (n == 0) { for (size_t g = 0; g < nseg; g++) memcpy(out + g * 72, &one, sizeof one); return DGPU_OK; }
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    std::vector<uint32_t> off(nseg + 1, 0);
    for (size_t g = 0; g < nseg; g++) off[g + 1] = (uint32_t)seg_end[g];
    if ((rc = ml_upload(sl, p, q, skip, n, nullptr, nullptr, nullptr, 0, (nseg + 1) * 4 + 8))) return rc;
    hipStream_t s = sl.stream;
    const uint8_t *dskip = skip ? sl.in_inf.as<uint8_t>() : nullptr;
    uint32_t *doff = (uint32_t *)(sl.in_inf.as<uint8_t>() + ((n + 7) & ~(size_t)7));
    HIPCHK(hipMemcpyAsync(doff, off.data(), (nseg + 1) * 4, hipMemcpyHostToDevice, s));
    const MlGeom g = ml_geom(maxlen, choose_segment_slice_len(maxlen), 0, (int)nseg, doff);
    const int mode = gs.ml_mode.load();
    // pieces: like ml_pipelined, the chain runs in ML_PIECES launches; the products and trees of a finished piece (every segment's) run on a side stream
    // under the next piece, its results land in pinned memory, and the host tails of the segments advance piece by piece on the library's threads —
    // what is left when the chain ends is the last piece's share of the tail and the final exponentiations (a GIPA round: 1.8 -> 1.5 ms)
    const size_t pin_bytes = (size_t)N_LINES * nseg * 576;
    if (n <= 8192 && (mode & 1) && pin_bytes <= ((size_t)4 << 20)) {
        if (sl.hpin2_bytes < pin_bytes) {
            if (sl.hpin2) { (void)hipHostFree(sl.hpin2); sl.hpin2 = nullptr; sl.hpin2_bytes = 0; }
            if (hipHostMalloc(&sl.hpin2, pin_bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); sl.hpin2 = nullptr; return DGPU_E_OOM; }
            sl.hpin2_bytes = pin_bytes;
        }
        hostf::Fq12 *Lp = (hostf::Fq12 *)sl.hpin2;                          // [segment][step]
        const MlCuts cuts(mode);
        const int device = cur().device;
        const size_t T = ml_tail_threads(nseg);
        rc = ml_run_pieces(sl, n, n, dskip, g, g, cuts, Lp, [](uint32_t *) {}, nullptr, false, [&](const hipEvent_t *done) -> int32_t {
            return par_run(T, [&](size_t k) -> int32_t {
                if (hipSetDevice(device) != hipSuccess) return DGPU_E_HIP;
                std::vector<MlTail> tails((nseg - k + T - 1) / T);
                for (int j = 0; j < ML_PIECES; j++) {
                    if (hipEventSynchronize(done[j]) != hipSuccess) return DGPU_E_HIP;
                    size_t m = 0;
                    for (size_t i = k; i < nseg; i += T, m++) if (off[i + 1] != off[i]) tails[m].run(Lp + i * N_LINES, cuts.at[j]);
                }
                size_t m = 0;
                for (size_t i = k; i < nseg; i += T, m++) ml_put(out + i * 72, off[i + 1] == off[i] ? one : tails[m].result(), finish);
                return DGPU_OK; }); });
        if (gs.prof) prof_flush(sl);
    } else {
        if ((rc = sl.ml_state.ensure((size_t)PXY_W * n * 4))) return rc;      // px, py of every pair for the product kernel
        uint32_t *pxy = sl.ml_state.as<uint32_t>();
        { StageTimer st(sl, "ml.lines");
          if (n > 8192) launch_lines_eval(s, sl.in_bases.as<uint32_t>(), sl.in_scalars.as<uint32_t>(), dskip, n, sl.ml_lines.as<uint32_t>(), n, 2);
          else launch_lines_uneval(s, mode, sl.in_bases.as<uint32_t>(), sl.in_scalars.as<uint32_t>(), dskip, n, sl.ml_lines.as<uint32_t>(), n,
                                   62, 0, 0, nullptr, pxy); }       // (the evaluation at P is left to the product kernel: not part of the chain)
        rc = ml_finish(sl, n, g, out, n > 8192 ? nullptr : pxy, false, off.data(), finish);
    }
    if (rc) return rc;
    return zero ? DGPU_E_ZERO : DGPU_OK;
}

int32_t dgpu_multi_miller_loop_segments(const uint64_t *p, const uint64_t *q, const uint8_t *skip, size_t n, const uint64_t *seg_end, size_t nseg, uint64_t *out) {
    return ml_segments(p, q, skip, n, seg_end, nseg, out, false);
}
// E::multi_pairing per segment: the final exponentiation of every Miller output on the host thread that assembled it
int32_t dgpu_multi_pairing_segments(const uint64_t *p, const uint64_t *q, const uint8_t *skip, size_t n, const uint64_t *seg_end, size_t nseg, uint64_t *out) {
    return ml_segments(p, q, skip, n, seg_end, nseg, out, true);
}

// pairs chunked over the process's device contexts (SURVEY 8e "Miller loop": pairs are independent, the per-device raw outputs multiply —
// limb for limb the single-device value, because squaring distributes over the per-step line products and Fp12 products are exact)
int32_t dgpu_multi_miller_loop_sharded(const uint64_t *p, const uint64_t *q, const uint8_t *skip, size_t n, int32_t ngpus, uint64_t *out) {
    if (!out || (n && (!p || !q)) || ngpus < 0) return DGPU_E_BADARG;
    const std::vector<int> cx = ready_contexts(ngpus);
    if (cx.empty()) return DGPU_E_NODEVICE;
    if (ngpus > 0 && (int)cx.size() < ngpus) return DGPU_E_BADARG;
    const size_t G = cx.size();
    std::vector<hostf::Fq12> parts(G);
    const int32_t prc = par_run(G, [&](size_t k) -> int32_t {
        const size_t lo = k * (n / G) + std::min(k, n % G), hi = (k + 1) * (n / G) + std::min(k + 1, n % G);
        CtxScope here(cx[k]);
        return dgpu_multi_miller_loop(p + lo * 12, q + lo * 24, skip ? skip + lo : nullptr, hi - lo, (uint64_t *)&parts[k]);
    });
    if (prc) return prc;
    hostf::Fq12 f = parts[0];
    for (size_t k = 1; k < G; k++) f = f * parts[k];
    memcpy(out, &f, sizeof f);
    return DGPU_OK;
}

// E::G2Prepared::from for a batch (utils/src/randomized_pairing_check.rs:132 `b.into()`, legogroth16/src/verifier.rs:22-23,72)
int32_t dgpu_g2_prepare(const uint64_t *q, const uint8_t *is_inf, size_t n, uint64_t *out_coeffs, uint8_t *out_inf) {
    if (n && (!q || !out_coeffs || !out_inf)) return DGPU_E_BADARG;
    if (n == 0) return DGPU_OK;
    if (n > DGPU_MAX_PREPARED) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    const size_t cbytes = n * (size_t)DGPU_G2_PREPARED_WORDS * 8;
    if ((rc = sl.in_scalars.ensure(n * 192))) return rc;
    if ((rc = sl.in_inf.ensure(2 * n))) return rc;
    if ((rc = sl.ml_coeffs.ensure(cbytes))) return rc;
    hipStream_t s = sl.stream;
    HIPCHK(hipMemcpyAsync(sl.in_scalars.p, q, n * 192, hipMemcpyHostToDevice, s));
    const uint8_t *dinf = nullptr;
    if (is_inf) { HIPCHK(hipMemcpyAsync(sl.in_inf.p, is_inf, n, hipMemcpyHostToDevice, s)); dinf = sl.in_inf.as<uint8_t>(); }
    { StageTimer st(sl, "ml.g2_prepare");
      const int mode = gs.ml_mode.load();
      if (n <= 8192 && (mode & 1)) {
          if ((rc = sl.ml_lines.ensure((size_t)N_LINES * LW * n * 4))) return rc;
          launch_lines_uneval(s, mode, nullptr, sl.in_scalars.as<uint32_t>(), dinf, n, sl.ml_lines.as<uint32_t>(), n, 62, 0, 0, nullptr, nullptr);
          launch_prepared_from_lines(s, sl.ml_lines.as<uint32_t>(), sl.in_scalars.as<uint32_t>(), dinf, n, sl.ml_coeffs.as<uint32_t>(), sl.in_inf.as<uint8_t>() + n);
      } else
          launch_g2_prepare(s, sl.in_scalars.as<uint32_t>(), dinf, n, sl.ml_coeffs.as<uint32_t>(), sl.in_inf.as<uint8_t>() + n); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_coeffs, sl.ml_coeffs.p, cbytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_inf, sl.in_inf.as<uint8_t>() + n, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (gs.prof) prof_flush(sl);
    return DGPU_OK;
}

// E::multi_miller_loop(a, b) with b already G2Prepared (what verifier.rs:69-76 and randomized_pairing_check.rs:207 pass)
int32_t dgpu_multi_miller_loop_prepared(const uint64_t *p, const uint64_t *coeffs, const uint8_t *skip, size_t n, uint64_t *out) {
    if (!out || (n && (!p || !coeffs))) return DGPU_E_BADARG;
    if (n == 0) { hostf::Fq12 one = hostf::Fq12::one(); memcpy(out, &one, sizeof one); return DGPU_OK; }
    if (n > DGPU_MAX_PREPARED) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    if ((rc = ml_upload(sl, nullptr, nullptr, nullptr, 0, p, coeffs, skip, n))) return rc;
    { StageTimer st(sl, "ml.lines_prepared");
      ml_prepared_lines(sl, 0, n, skip != nullptr, nullptr); }
    return ml_finish(sl, n, ml_single(n), out);
}

// Affine and prepared G2 operands in ONE Miller loop: the line kernels of both forms fill one line buffer (the affine pairs first), the
// products / tree / host part run once.  This is what a verifier holds: proof.b affine, the key's -delta and -gamma prepared
// (legogroth16/src/verifier.rs:69-76: `[proof.b.into(), pvk.delta_g2_neg_pc.clone(), pvk.gamma_g2_neg_pc.clone()]`).  Preparing the affine
// members first costs a call of its own plus 19.5 KB per point down and up again.
int32_t dgpu_multi_miller_loop_mixed(const uint64_t *p_aff, const uint64_t *q_aff, const uint8_t *skip_aff, size_t n_aff,
                                     const uint64_t *p_prep, const uint64_t *coeffs, const uint8_t *skip_prep, size_t n_prep, uint64_t *out) {
    if (!out || (n_aff && (!p_aff || !q_aff)) || (n_prep && (!p_prep || !coeffs))) return DGPU_E_BADARG;
    const size_t n = n_aff + n_prep;
    if (n == 0) { hostf::Fq12 one = hostf::Fq12::one(); memcpy(out, &one, sizeof one); return DGPU_OK; }
    if (n_prep > DGPU_MAX_PREPARED || n >= (1ull << 24)) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    if ((rc = ml_upload(sl, p_aff, q_aff, skip_aff, n_aff, p_prep, coeffs, skip_prep, n_prep))) return rc;
    const uint8_t *dskip = skip_aff ? sl.in_inf.as<uint8_t>() : nullptr;
    if (n_aff && n_aff <= 8192 && !gs.prof && (gs.ml_mode.load() & 1)) {
        // what a verifier calls (proof.b affine, the key's -delta and -gamma prepared): the affine pairs' chain is cut like
        // dgpu_multi_miller_loop's; the prepared pairs' lines are ready long before the first launch of the line kernel ends
        MlActive act(cur().ml_active);
        if (act.v <= 2) return ml_pipelined(sl, n, n_aff, dskip, out, [&](uint32_t *pxy) { ml_prepared_lines(sl, n_aff, n_prep, skip_prep != nullptr, pxy); });
    }
    { StageTimer st(sl, "ml.lines");
      if (n_aff) launch_lines_eval(sl.stream, sl.in_bases.as<uint32_t>(), sl.in_scalars.as<uint32_t>(), dskip, n_aff, sl.ml_lines.as<uint32_t>(), n, n_aff > 8192 ? 2 : 4);
      ml_prepared_lines(sl, n_aff, n_prep, skip_prep != nullptr, nullptr); }
    return ml_finish(sl, n, ml_single(n), out);
}

// ---- prod_i e(m_i P_i, Q_i) x prod_j e(P'_j, prepared_j): the scalings and the Miller loop of RandomizedPairingChecker as ONE call ----
// utils/src/randomized_pairing_check.rs:125-134: `a.mul_bigint(m)` for every source, then the pairs go to one multi_miller_loop (:204-214 in lazy mode).
// The line coefficients of a pair depend on Q alone and P enters only in the product kernels (the lines leave unevaluated, px and py travel beside
// them), so the chain of the Q_i starts at once and the 128-step scaling chains of the P_i (k_g1_scale_quad) run BESIDE it instead of in front of it;
// the scaled points never visit the host.  1024 pairs: 1.14 (scalings) + 0.75 (Miller loop) ms one after the other -> ~1.3 ms.
int32_t dgpu_multi_miller_loop_scaled(const uint64_t *p_aff, const uint64_t *scalars, size_t scalar_stride, const uint64_t *q_aff, const uint8_t *skip_aff, size_t n_aff,
                                      const uint64_t *p_prep, const uint64_t *coeffs, const uint8_t *skip_prep, size_t n_prep, uint64_t *out) {
    if (!out || (n_aff && (!p_aff || !q_aff || !scalars)) || (n_prep && (!p_prep || !coeffs)) || (scalar_stride != 0 && scalar_stride != 4)) return DGPU_E_BADARG;
    const size_t n = n_aff + n_prep;
    if (n_aff == 0) return dgpu_multi_miller_loop_mixed(nullptr, nullptr, nullptr, 0, p_prep, coeffs, skip_prep, n_prep, out);
    if (n_prep > DGPU_MAX_PREPARED || n >= (1ull << 24)) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    // GLV: every scalar goes to the device as (k1 | k2), k mod r = k1 + k2 lambda; a pair whose scaled point is the identity is skipped (m = 0 mod r or P = 0)
    const size_t nsc = scalar_stride ? n_aff : 1;
    std::vector<uint64_t> split(nsc * 4);
    for (size_t k = 0; k < nsc; k++) hostf::glv_decompose(scalars + 4 * k, &split[4 * k], &split[4 * k + 2]);
    auto zero = [](const uint64_t *w, int k) { uint64_t o = 0; for (int i = 0; i < k; i++) o |= w[i]; return o == 0; };
    std::vector<uint8_t> skip(n_aff);
    for (size_t i = 0; i < n_aff; i++)
        skip[i] = (skip_aff && skip_aff[i]) || zero(&split[scalar_stride ? 4 * i : 0], 4) || zero(p_aff + 12 * i, 12) ? 1 : 0;
    bool pipelined = n_aff <= 8192 && !gs.prof && (gs.ml_mode.load() & 1);
    if (pipelined) { MlActive probe(cur().ml_active); pipelined = probe.v <= 2; }
    if (!pipelined) {          // large batches (throughput-bound), stage timers on, or many loops in flight: the two calls one after the other
        std::vector<uint64_t> scaled(n_aff * 12); std::vector<uint8_t> sinf(n_aff);
        int32_t rc = dgpu_g1_scale_batch(p_aff, nullptr, scalars, scalar_stride, nullptr, n_aff, scaled.data(), sinf.data());
        if (rc) return rc;
        for (size_t i = 0; i < n_aff; i++) skip[i] |= sinf[i];
        return dgpu_multi_miller_loop_mixed(scaled.data(), q_aff, skip.data(), n_aff, p_prep, coeffs, skip_prep, n_prep, out);
    }
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    const size_t sc_off = (n_aff * 96 + n_aff + 63) & ~(size_t)63;            // prepped: [scaled points | their flags | pad | split scalars]
    if ((rc = sl.prepped.ensure(sc_off + nsc * 32))) return rc;
    if ((rc = ml_upload(sl, nullptr, q_aff, skip.data(), n_aff, p_prep, coeffs, skip_prep, n_prep))) return rc;
    MlActive act(cur().ml_active);
    uint32_t *dp = sl.in_bases.as<uint32_t>();
    uint32_t *scaled = sl.prepped.as<uint32_t>(); uint8_t *scaled_inf = sl.prepped.as<uint8_t>() + n_aff * 96;
    uint32_t *dsplit = (uint32_t *)(sl.prepped.as<uint8_t>() + sc_off);
    return ml_pipelined(sl, n, n_aff, sl.in_inf.as<uint8_t>(), out, [&](uint32_t *pxy) { ml_prepared_lines(sl, n_aff, n_prep, skip_prep != nullptr, pxy); },
                        [&](hipStream_t side, uint32_t *pxy) -> int32_t {
        // the chain of the Q_i is queued: the scalings run beside it on the side stream, their results go straight to px, py
        if (hipMemcpyAsync(dp, p_aff, n_aff * 96, hipMemcpyHostToDevice, side) != hipSuccess) return DGPU_E_HIP;
        if (hipMemcpyAsync(dsplit, split.data(), nsc * 32, hipMemcpyHostToDevice, side) != hipSuccess) return DGPU_E_HIP;
        msm::launch_g1_scale_quad(side, dp, nullptr, dsplit, (int)(scalar_stride * 2), nullptr, n_aff, scaled, scaled_inf);
        launch_pxy_from_abi(side, scaled, n_aff, pxy, n);
        return hipGetLastError() == hipSuccess ? DGPU_OK : DGPU_E_HIP;
    }, true);
}

// ---- the LegoGroth16 verifier as one call (legogroth16/src/verifier.rs:62-99 `verify_proof`: calculate_d :29-50,101-109, then verify_qap_proof) ----
// e(A, B) e(C, -delta) e(gamma_abc[0] + sum x_j gamma_abc[1 + j] + D, -gamma) == e(alpha, beta), with -delta, -gamma held prepared and e(alpha, beta)
// precomputed in the PreparedVerifyingKey (verifier.rs:17-25).  One call instead of calculate_d + multi_miller_loop + final_exponentiation lets
// the library hide the host's share under the device's: the chain of the one affine pair (A, B) is queued first, the third G1 operand (a
// 255-bit scalar multiplication per public input, ~0.15 ms of one host core) is computed while it runs, the two prepared pairs' lines follow on
// a side stream in front of the product kernels.  *ok = 1 / 0; DGPU_E_BADARG for a key too short for the inputs (`MalformedVerifyingKey`).
int32_t dgpu_legogroth16_verify(const uint64_t alpha_beta_gt[72], const uint64_t *delta_neg_pc, const uint64_t *gamma_neg_pc, const uint64_t *gamma_abc_g1, size_t gamma_abc_len,
                                const uint64_t proof_a[12], const uint64_t proof_b[24], const uint64_t proof_c[12], const uint64_t proof_d[12], const uint8_t *proof_inf /* 4 or NULL */,
                                const uint64_t *public_inputs, size_t n_pub, int32_t montgomery, int32_t *ok_out) {
    if (!alpha_beta_gt || !delta_neg_pc || !gamma_neg_pc || !gamma_abc_g1 || !proof_a || !proof_b || !proof_c || !proof_d || !ok_out || (n_pub && !public_inputs)) return DGPU_E_BADARG;
    if (n_pub + 1 > gamma_abc_len) return DGPU_E_BADARG;                       // verifier.rs:38-40 MalformedVerifyingKey
    if (n_pub + 2 > DGPU_MAX_LINCOMB) return DGPU_E_BADARG;                    // (more public inputs: calculate_d through dgpu_msm_g1, then dgpu_multi_miller_loop_mixed)
    if (!cur().ready) return DGPU_E_NODEVICE;
    auto all_zero = [](const uint64_t *w, int k) { uint64_t o = 0; for (int i = 0; i < k; i++) o |= w[i]; return o == 0; };
    const bool inf_a = (proof_inf && proof_inf[0]) || all_zero(proof_a, 12), inf_b = (proof_inf && proof_inf[1]) || all_zero(proof_b, 24);
    const bool inf_c = (proof_inf && proof_inf[2]) || all_zero(proof_c, 12), inf_d = (proof_inf && proof_inf[3]) || all_zero(proof_d, 12);
    // d = gamma_abc[0] + sum x_j gamma_abc[1 + j] + proof.d on a host core
    uint64_t dxy[12]; bool d_inf = true;
    auto compute_d = [&]() -> int32_t {
        uint64_t pts[DGPU_MAX_LINCOMB * 12], sc[DGPU_MAX_LINCOMB * 4], jac[18]; uint8_t inf[DGPU_MAX_LINCOMB] = {0};
        const size_t k = n_pub + 2;
        memcpy(pts, gamma_abc_g1, (n_pub + 1) * 96); memcpy(pts + (n_pub + 1) * 12, proof_d, 96); inf[n_pub + 1] = inf_d;
        memset(sc, 0, sizeof sc); sc[0] = 1; sc[4 * (n_pub + 1)] = 1;
        for (size_t j = 0; j < n_pub; j++) { if (montgomery) hostf::fr_from_mont(&sc[4 * (1 + j)], public_inputs + 4 * j); else memcpy(&sc[4 * (1 + j)], public_inputs + 4 * j, 32); }
        const int32_t e = dgpu_lincomb_g1(pts, inf, sc, k, jac);
        if (e) return e;
        d_inf = all_zero(jac + 12, 6);
        memcpy(dxy, jac, 96);                                                   // normalised: (x, y, 1)
        return DGPU_OK;
    };
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    const size_t n = 3, cbytes = 2 * (size_t)DGPU_G2_PREPARED_WORDS * 8;
    if ((rc = sl.in_bases.ensure(n * 96))) return rc;
    if ((rc = sl.in_scalars.ensure(192 + 16))) return rc;
    if ((rc = sl.in_inf.ensure(16))) return rc;
    if ((rc = sl.ml_coeffs.ensure(cbytes + 16))) return rc;
    if ((rc = sl.ml_lines.ensure((size_t)N_LINES * LW * n * 4))) return rc;
    hipStream_t s = sl.stream;
    uint32_t *dp = sl.in_bases.as<uint32_t>();
    uint8_t *dsk = sl.in_inf.as<uint8_t>();
    uint8_t *hsk = (uint8_t *)sl.hpin + Slot::HPIN_BYTES - 256;                 // pinned: the flags of the three pairs, and d's coordinates behind them
    hsk[0] = (inf_a || inf_b) ? 1 : 0; hsk[1] = inf_c ? 1 : 0; hsk[2] = 0;
    HIPCHK(hipMemcpyAsync(dp, proof_a, 96, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dp + 24, proof_c, 96, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.in_scalars.p, proof_b, 192, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sl.ml_coeffs.p, delta_neg_pc, cbytes / 2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync((char *)sl.ml_coeffs.p + cbytes / 2, gamma_neg_pc, cbytes / 2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dsk, hsk, 1, hipMemcpyHostToDevice, s));
    hostf::Fq12 f;
    uint32_t *lines = sl.ml_lines.as<uint32_t>();
    auto prepared_lines = [&](hipStream_t st, uint32_t *pxy) {
        launch_lines_from_prepared(st, dp + 24, sl.ml_coeffs.as<uint32_t>(), dsk + 1, 2, lines + 1, n, pxy ? pxy + 1 : nullptr);
    };
    MlActive act(cur().ml_active);
    if (!gs.prof && (gs.ml_mode.load() & 1) && act.v <= 2) {
        hipEvent_t in_ev = sl.copy_ev[sl.ev_next++ % (Slot::N_COPY_EV + 1)];
        HIPCHK(hipEventRecord(in_ev, s));
        rc = ml_pipelined(sl, n, 1, dsk, (uint64_t *)&f, [](uint32_t *) {}, [&](hipStream_t side, uint32_t *pxy) -> int32_t {
            const int32_t e = compute_d(); if (e) return e;                     // (the chain of (A, B) is running)
            memcpy(hsk + 16, dxy, 96); hsk[2] = d_inf ? 1 : 0;
            if (hipStreamWaitEvent(side, in_ev, 0) != hipSuccess) return DGPU_E_HIP;       // C, the coefficients and the first flag are on their way on `s`
            if (hipMemcpyAsync(dp + 48, hsk + 16, 96, hipMemcpyHostToDevice, side) != hipSuccess) return DGPU_E_HIP;
            if (hipMemcpyAsync(dsk + 1, hsk + 1, 2, hipMemcpyHostToDevice, side) != hipSuccess) return DGPU_E_HIP;
            prepared_lines(side, pxy);
            return DGPU_OK;
        });
        if (rc) return rc;
    } else {
        if ((rc = compute_d())) return rc;
        memcpy(hsk + 16, dxy, 96); hsk[2] = d_inf ? 1 : 0;
        HIPCHK(hipMemcpyAsync(dp + 48, hsk + 16, 96, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dsk + 1, hsk + 1, 2, hipMemcpyHostToDevice, s));
        if ((rc = sl.ml_state.ensure((size_t)PXY_W * n * 4))) return rc;
        uint32_t *pxy = sl.ml_state.as<uint32_t>();
        launch_lines_uneval(s, gs.ml_mode.load(), dp, sl.in_scalars.as<uint32_t>(), dsk, 1, lines, n, 62, 0, 0, nullptr, pxy);
        prepared_lines(s, pxy);
        if ((rc = ml_finish(sl, n, ml_single(n), (uint64_t *)&f, pxy))) return rc;
    }
    hostf::Fq12 gt, want; memcpy(&want, alpha_beta_gt, sizeof want);
    if (!hostf::final_exponentiation(gt, f)) return DGPU_E_ZERO;               // (verifier.rs:78 `.ok_or(UnexpectedIdentity)`)
    *ok_out = memcmp(&gt, &want, sizeof gt) == 0 ? 1 : 0;
    return DGPU_OK;
}

int32_t dgpu_g1_scale_batch(const uint64_t *p, const uint8_t *is_inf, const uint64_t *scalars, size_t scalar_stride, const uint8_t *negate, size_t n, uint64_t *out, uint8_t *out_inf) {
    if ((n && (!p || !scalars || !out || !out_inf)) || (scalar_stride != 0 && scalar_stride != 4)) return DGPU_E_BADARG;
    if (n == 0) return DGPU_OK;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    const size_t nsc = scalar_stride ? n : 1;
    if ((rc = sl.in_bases.ensure(n * 96))) return rc;
    if ((rc = sl.in_scalars.ensure(nsc * 32))) return rc;
    if ((rc = sl.in_inf.ensure(2 * n))) return rc;
    if ((rc = sl.prepped.ensure(n * 96 + n))) return rc;
    hipStream_t s = sl.stream;
    HIPCHK(hipMemcpyAsync(sl.in_bases.p, p, n * 96, hipMemcpyHostToDevice, s));
    // GLV: every scalar is sent as (k1 | k2), k mod r = k1 + k2 lambda, both below 2^128 (host_field.hpp)
    std::vector<uint64_t> split(nsc * 4);
    for (size_t k = 0; k < nsc; k++) hostf::glv_decompose(scalars + 4 * k, &split[4 * k], &split[4 * k + 2]);
    HIPCHK(hipMemcpyAsync(sl.in_scalars.p, split.data(), nsc * 32, hipMemcpyHostToDevice, s));
    const uint8_t *dinf = nullptr, *dneg = nullptr;
    if (is_inf) { HIPCHK(hipMemcpyAsync(sl.in_inf.p, is_inf, n, hipMemcpyHostToDevice, s)); dinf = sl.in_inf.as<uint8_t>(); }
    if (negate) { HIPCHK(hipMemcpyAsync(sl.in_inf.as<uint8_t>() + n, negate, n, hipMemcpyHostToDevice, s)); dneg = sl.in_inf.as<uint8_t>() + n; }
    uint8_t *dout_inf = sl.prepped.as<uint8_t>() + n * 96;
    { StageTimer st(sl, "pc.g1_scale");
      msm::launch_g1_scale_quad(s, sl.in_bases.as<uint32_t>(), dinf, sl.in_scalars.as<uint32_t>(), (int)(scalar_stride * 2), dneg, n, sl.prepped.as<uint32_t>(), dout_inf); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, sl.prepped.p, n * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_inf, dout_inf, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (gs.prof) prof_flush(sl);
    return DGPU_OK;
}
// ---- many independent GT elements: the Fp12 chains on the device (k_gt.hip, gt_kernels.hip.h) ----
constexpr size_t FE_CHUNK = 16384;        // elements per launch: 9.4 MB of device memory in and out
int32_t dgpu_final_exponentiation_batch(const uint64_t *in, size_t n, uint64_t *out, uint8_t *is_zero) {
    if (n == 0) return DGPU_OK;
    if (!in || !out || !is_zero) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(slot_lock, sl);
    HIPCHK(hipSetDevice(cur().device));
    int32_t rc;
    const size_t ch = std::min(n, FE_CHUNK);
    if ((rc = sl.ml_out.ensure(ch * 576 * 2))) return rc;
    if ((rc = sl.flags.ensure(ch))) return rc;
    hipStream_t s = sl.stream;
    uint32_t *din = sl.ml_out.as<uint32_t>(), *dout = din + ch * 144;
    for (size_t lo = 0; lo < n; lo += ch) {
        const size_t m = std::min(ch, n - lo);
        HIPCHK(hipMemcpyAsync(din, in + lo * 72, m * 576, hipMemcpyHostToDevice, s));
        { StageTimer st(sl, "gt.final_exp"); gtk::launch_final_exp(s, din, m, dout, sl.flags.as<uint8_t>(), nullptr, nullptr); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + lo * 72, dout, m * 576, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(is_zero + lo, sl.flags.p, m, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (gs.prof) prof_flush(sl);
    return DGPU_OK;
}

// ---- one verdict per LegoGroth16 proof (verifier.rs:62-99 `verify_proof` once per statement) ----
// Per chunk of up to VE_CHUNK proofs:
//   d_i = gamma_abc[0] + sum_j x_ij gamma_abc[1 + j] + D_i    n_pub + 1 calls of dgpu_g1_mul_add_batch (one shared point each)
//   lines: (A_i, B_i) affine in columns [0, m), (C_i, -delta) in [m, 2m), (d_i, -gamma) in [2m, 3m) — the two prepared points' coefficients
//          uploaded ONCE and shared by every column (k_lines_from_prepared, shared)
//   k_line_products over one "segment" of 3m pairs with slices of 3: slice j is the pairs j, j + m, j + 2 m, i.e. partial (s, j) = L_s of proof j
//   k_miller_tail, k_final_exp against e(alpha, beta): only the m verdict bytes come back.
// Device memory of a chunk: 68 x 84 x 4 B x 3m of lines + 68 x 672 B x m of per-step products + 576 B x m ~ 115 KB per proof (0.47 GB at 4096).
constexpr size_t VE_CHUNK = 4096;
int32_t dgpu_legogroth16_verify_each(const uint64_t alpha_beta_gt[72], const uint64_t *delta_neg_pc, const uint64_t *gamma_neg_pc, const uint64_t *gamma_abc_g1, size_t gamma_abc_len,
                                     const uint64_t *proofs_a, const uint64_t *proofs_b, const uint64_t *proofs_c, const uint64_t *proofs_d, size_t n,
                                     const uint64_t *public_inputs, size_t n_pub, int32_t montgomery, uint8_t *ok) {
    if (!alpha_beta_gt || !delta_neg_pc || !gamma_neg_pc || !gamma_abc_g1) return DGPU_E_BADARG;
    if (n && (!proofs_a || !proofs_b || !proofs_c || !proofs_d || !ok)) return DGPU_E_BADARG;
    if (n_pub + 1 > gamma_abc_len || (n && n_pub && !public_inputs)) return DGPU_E_BADARG;          // MalformedVerifyingKey (verifier.rs:101-109)
    if (n == 0) return DGPU_OK;
    if (!cur().ready) return DGPU_E_NODEVICE;
    auto zero_words = [](const uint64_t *w, int k) { uint64_t o = 0; for (int i = 0; i < k; i++) o |= w[i]; return o == 0; };
    const size_t cw = (size_t)DGPU_G2_PREPARED_WORDS;
    for (size_t lo = 0; lo < n; lo += VE_CHUNK) {
        const size_t m = std::min(VE_CHUNK, n - lo), np = 3 * m;
        // d_i on the device, before a slot is taken (the mul-add calls take their own)
        std::vector<uint64_t> rep(m * 12), d(m * 12), d2(m * 12), sc(m * 4);
        std::vector<uint8_t> dinf(m), dinf2(m);
        const uint64_t one[4] = {1, 0, 0, 0};
        for (size_t i = 0; i < m; i++) memcpy(&rep[i * 12], gamma_abc_g1, 96);
        int32_t rc = dgpu_g1_mul_add_batch(rep.data(), nullptr, one, 0, proofs_d + lo * 12, nullptr, m, d.data(), dinf.data());
        if (rc) return rc;
        for (size_t j = 0; j < n_pub; j++) {
            for (size_t i = 0; i < m; i++) {
                memcpy(&rep[i * 12], gamma_abc_g1 + 12 * (1 + j), 96);
                const uint64_t *x = public_inputs + 4 * ((lo + i) * n_pub + j);
                if (montgomery) hostf::fr_from_mont(&sc[4 * i], x); else memcpy(&sc[4 * i], x, 32);
            }
            if ((rc = dgpu_g1_mul_add_batch(rep.data(), nullptr, sc.data(), 4, d.data(), dinf.data(), m, d2.data(), dinf2.data()))) return rc;
            d.swap(d2); dinf.swap(dinf2);
        }
        std::vector<uint8_t> sk(np);
        for (size_t i = 0; i < m; i++) {
            sk[i] = (zero_words(proofs_a + (lo + i) * 12, 12) || zero_words(proofs_b + (lo + i) * 24, 24)) ? 1 : 0;
            sk[m + i] = zero_words(proofs_c + (lo + i) * 12, 12) ? 1 : 0;
            sk[2 * m + i] = (dinf[i] || zero_words(&d[i * 12], 12)) ? 1 : 0;
        }
        SLOT_ACQUIRE(slot_lock, sl);
        HIPCHK(hipSetDevice(cur().device));
        if ((rc = sl.in_bases.ensure(np * 96))) return rc;
        if ((rc = sl.in_scalars.ensure(m * 192 + 16))) return rc;
        if ((rc = sl.in_inf.ensure(np + 16))) return rc;
        if ((rc = sl.ml_coeffs.ensure(2 * cw * 8 + 16))) return rc;
        if ((rc = sl.ml_lines.ensure((size_t)N_LINES * LW * np * 4))) return rc;
        if ((rc = sl.ml_partial.ensure((size_t)N_LINES * m * F12W * 4))) return rc;
        if ((rc = sl.ml_out.ensure(m * 576 + 576))) return rc;
        if ((rc = sl.flags.ensure(m))) return rc;
        hipStream_t s = sl.stream;
        uint32_t *dp = sl.in_bases.as<uint32_t>(), *lines = sl.ml_lines.as<uint32_t>(), *fout = sl.ml_out.as<uint32_t>(), *want = fout + m * 144;
        uint8_t *dsk = sl.in_inf.as<uint8_t>();
        HIPCHK(hipMemcpyAsync(dp, proofs_a + lo * 12, m * 96, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dp + m * 24, proofs_c + lo * 12, m * 96, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dp + 2 * m * 24, d.data(), m * 96, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sl.in_scalars.p, proofs_b + lo * 24, m * 192, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dsk, sk.data(), np, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sl.ml_coeffs.p, delta_neg_pc, cw * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sl.ml_coeffs.as<uint64_t>() + cw, gamma_neg_pc, cw * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(want, alpha_beta_gt, 576, hipMemcpyHostToDevice, s));
        { StageTimer st(sl, "ve.lines");
          launch_lines_eval(s, dp, sl.in_scalars.as<uint32_t>(), dsk, m, lines, np, 4);
          for (int k = 0; k < 2; k++)
              launch_lines_from_prepared(s, dp + (1 + k) * m * 24, sl.ml_coeffs.as<uint32_t>() + k * cw * 2, dsk + (1 + k) * m, m, lines + (1 + k) * m, np, nullptr, true); }
        { StageTimer st(sl, "ve.products");
          launch_line_products(s, gs.ml_mode.load(), lines, np, 3, (int)m, sl.ml_partial.as<uint32_t>(), nullptr, 1, 0, N_LINES, nullptr, false); }
        { StageTimer st(sl, "ve.tail"); gtk::launch_miller_tail(s, sl.ml_partial.as<uint32_t>(), m, fout); }
        { StageTimer st(sl, "ve.final_exp"); gtk::launch_final_exp(s, fout, m, (uint32_t *)nullptr, (uint8_t *)nullptr, want, sl.flags.as<uint8_t>()); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ok + lo, sl.flags.p, m, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (gs.prof) prof_flush(sl);
    }
    return DGPU_OK;
}

// E::final_exponentiation: once per batch, host code
int32_t dgpu_final_exponentiation(const uint64_t *in, uint64_t *out) {
    if (!in || !out) return DGPU_E_BADARG;
    hostf::Fq12 f, r; memcpy(&f, in, sizeof f);
    if (!hostf::final_exponentiation(r, f)) return DGPU_E_ZERO;
    memcpy(out, &r, sizeof r);
    return DGPU_OK;
}

}  // extern "C"
