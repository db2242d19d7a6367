// crypto_amd/csrc/dock_saver.hip — SAVER (verifiable encryption over LegoGroth16, the reference's saver crate) in bulk (include/dock_gpu_saver.h, libdock_gpu_saver.so: dgpu_saver_dk_create,
// _free, _powers, dgpu_saver_decrypt_many, dgpu_saver_verify_decryption_each, dgpu_saver_verify_commitment_each, dgpu_saver_verify_commitments_batch):
// Ciphertext::decrypt_to_chunks_given_pairing_powers (saver/src/encryption.rs:569-624), verify_decryption (:425-469), verify_ciphertext_commitment (:367-393)
// and verify_commitments_in_batch (:395-422) for many ciphertexts under one key, each call ONE device pipeline per chunk of ciphertexts.  A ciphertext row is
// [c_0, c_1 .. c_K, psi], (K + 2) x 12 words; every pairing has a fixed G2 side per column, so the prepared-line kernels serve all of it.
//   key      device  the prepared coefficients of [H, V_0, V_1[K], V_2[K]]                                          k_g2_prepare
//            device  the K bases e(g_j, V_2_j): one Miller loop per column, the final exponentiation                 k_lines_from_prepared .. k_final_exp
//            device  the table T_j[m] = e(g_j, V_2_j)^m, m = 1 .. 2^b - 1, by doubling rounds                        k_gt_table_extend
//            host    the index: per column the entries' 64-bit fingerprints sorted with m (once per key)
//   decrypt  device  -rho c_0_i: the GLV scaling [s] P — for points of G1 ONLY (phi(P) = lambda P holds there) — with one scalar for all rows
//                                                                                                                   k_g1_scale_quad
//            device  per column j the lines of the c_ij against V_2_j and of the -rho c_0_i against V_1_j, both into ONE line buffer so that slice (i, j) is
//                    its two pairs (pair_check.hip.h's layout, rows column-major)                                    k_lines_from_prepared x 2 K
//            device  p_ij = e(c_ij, V_2_j) e(-rho c_0_i, V_1_j)                                                      k_line_products, k_miller_tail, k_final_exp
//            device  the chunk m with T_j[m] = p_ij (0 for one), exactly; the K miss bytes into a status             k_gt_dlog_lookup, k_saver_row_verdict
//   verify   the same pipeline with -nu_i in place of -rho c_0_i and the lookup in its compare-at-index mode; one more two-pair column,
//            e(c_0_i, V_0) e(-nu_i, H) against one, in passes of its own before it (DESIGN.md §16 has the equivalence with the reference's two checks)
//   commitment each   K + 2 pairs per row against the caller's prepared [Z_0 .. Z_K, H], -psi staged as y -> p - y; one slice per row
//   commitment batch  K + 2 MSMs over the columns with the caller's r_powers, the chunks' sums added on the host, ONE multi-pairing of K + 2 pairs
// Only chunks, nu and verdict bytes come back.  rho's device copy (the GLV split of -rho) is zeroed on every return path before the slot is released, and so
// is the host's copy of the split.
#include "msm_many.hip.h"
#include "../../include/dock_gpu_saver.h"
#include "qap_launch.hip.h"
#include "fixed_launch.hip.h"
#include "saver_launch.hip.h"
#include "acc_host_tables.hpp"
#include "pair_check.hip.h"             // neg_g1, ws_check, pair_tail, value_tail, add_jac, merged_multi_verdict
using namespace dock;
using namespace acch;
using namespace mlk;

namespace {

constexpr size_t GTB = 576;               // bytes of a GT element of the ABI
constexpr size_t CW = (size_t)DGPU_G2_PREPARED_WORDS;   // u64 words of one prepared G2 point

// kind 15.  coeffs: 2 K + 2 blocks in the order H, V_0, V_1[K], V_2[K]
struct SaverDk {
    void *coeffs = nullptr, *tab = nullptr, *fps = nullptr, *ms = nullptr, *one = nullptr;
    size_t K = 0; uint32_t E = 0; int b = 0; uint64_t mask = ~0ull;
    const uint32_t *pc(size_t k) const { return (const uint32_t *)coeffs + k * CW * 2; }
    const uint32_t *pc_H() const { return pc(0); }
    const uint32_t *pc_V0() const { return pc(1); }
    const uint32_t *pc_V1(size_t j) const { return pc(2 + j); }
    const uint32_t *pc_V2(size_t j) const { return pc(2 + K + j); }
    saverk::DkDev dev() const { return saverk::DkDev{(const uint32_t *)tab, (const uint64_t *)fps, (const uint16_t *)ms, (const uint32_t *)one, E, mask}; }
};
void release(SaverDk *d) {
    for (void *p : {d->coeffs, d->tab, d->fps, d->ms, d->one}) if (p) (void)hipFree(p);
    delete d;
}
bool dk_ok(const HandleRef &h) { return h.ok && h.h.kind == 15; }
// pairing rows per chunk (dgpu_set_many_chunk_rows of the development surface REPLACES the limit, unlike pair_check.hip.h chunk_rows, where it cuts the
// row count) -> ciphertexts per chunk when each takes `per` of them
size_t ct_chunk_rows(size_t n, size_t limit, size_t per) {
    const int forced = gs.many_chunk.load();
    const size_t lim = forced > 0 ? (size_t)forced : limit;
    return std::min(n, std::max<size_t>(1, lim / per));
}
// the buffers of the pairing pipeline over m two-pair slices (or `pairs` pairs in all): lines, products, Miller outputs + values, verdict bytes
int32_t ws_pairs(Slot &o, size_t pairs, size_t m) {
    int32_t e;
    if ((e = o.ml_lines.ensure((size_t)N_LINES * LW * pairs * 4))) return e;
    if ((e = o.ml_partial.ensure((size_t)N_LINES * m * F12W * 4))) return e;
    if ((e = o.ml_out.ensure(2 * m * GTB + GTB))) return e;
    return o.flags.ensure(std::max<size_t>(m, 64));
}

// ---- the key ---------------------------------------------------------------------------------------------------------------------------------------------------------
int32_t dk_create(const uint64_t *g_i, const uint64_t *H, const uint64_t *V_0, const uint64_t *V_1, const uint64_t *V_2, int32_t b, size_t K, uint64_t *handle) {
    if (!g_i || !H || !V_0 || !V_1 || !V_2 || !handle || b < 1 || b > 16 || K < 1 || K > 255) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const uint32_t E = (1u << b) - 1;
    const size_t np = 2 * K + 2, ne = K * (size_t)E;
    int32_t rc;
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.in_bases.ensure(np * PT2 + K * PT))) return e;
        return ws_pairs(o, K, K);
    };
    if ((rc = ws(sl))) return rc;
    SaverDk *d = new (std::nothrow) SaverDk;
    if (!d) return DGPU_E_OOM;
    d->K = K; d->E = E; d->b = b;
    const int bits = gs.saver_fp_bits.load();
    d->mask = bits == 0 ? ~0ull : (bits < 0 ? 0ull : ((1ull << bits) - 1));
    struct Undo { SaverDk *d; ~Undo() { if (d) release(d); } } undo{d};      // an allocation failure (or any error below) leaves nothing behind
    if (dev_malloc(&d->coeffs, np * CW * 8 + np + 16) != hipSuccess || dev_malloc(&d->tab, ne * GTB) != hipSuccess || dev_malloc(&d->fps, ne * 8) != hipSuccess ||
        dev_malloc(&d->ms, ne * 2 + 16) != hipSuccess || dev_malloc(&d->one, GTB) != hipSuccess) { (void)hipGetLastError(); return DGPU_E_OOM; }
    hipStream_t s = sl.stream;
    std::vector<uint64_t> fp(ne);
    std::vector<uint16_t> ms(ne);
    DrainUnlessDone guard(sl);
    static const hostf::Fq12 one = hostf::Fq12::one();
    uint8_t *dQ = sl.in_bases.as<uint8_t>(), *dG = dQ + np * PT2;
    HIPCHK(hipMemcpyAsync(dQ, H, PT2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dQ + PT2, V_0, PT2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dQ + 2 * PT2, V_1, K * PT2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dQ + (2 + K) * PT2, V_2, K * PT2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dG, g_i, K * PT, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d->one, &one, GTB, hipMemcpyHostToDevice, s));
    { StageTimer st(sl, "saver.prepare"); launch_g2_prepare(s, (const uint32_t *)dQ, nullptr, np, (uint32_t *)d->coeffs, (uint8_t *)d->coeffs + np * CW * 8); }
    // the K bases: pair j = (g_j, V_2_j) with its own coefficient block, one pair per slice
    uint32_t *fout = sl.ml_out.as<uint32_t>(), *gt = fout + K * 144;
    { StageTimer st(sl, "saver.base_lines"); launch_lines_from_prepared(s, (const uint32_t *)dG, d->pc_V2(0), nullptr, K, sl.ml_lines.as<uint32_t>(), K, nullptr, false); }
    pair_tail(sl, K, 1, nullptr, gt, nullptr);
    HIPCHK(hipMemcpy2DAsync(d->tab, (size_t)E * GTB, gt, GTB, GTB, K, hipMemcpyDeviceToDevice, s));
    { StageTimer st(sl, "saver.table");
      for (uint32_t half = 1; half < E; half *= 2) saverk::launch_gt_table_extend(s, (uint32_t *)d->tab, K, E, half, std::min(half, E - half)); }
    HIPCHK(hipGetLastError());
    // the index: the first two words of every entry come back, are masked and sorted per column together with m
    // (whole entries in pieces of 16 MB: a strided copy of 8 bytes out of every 576 has millions of rows at b = 16)
    auto t0 = std::chrono::steady_clock::now();
    {
        constexpr size_t PIECE = 28672;
        std::vector<uint64_t> piece(std::min(ne, PIECE) * 72);
        for (size_t lo = 0; lo < ne; lo += PIECE) {
            const size_t cnt = std::min(PIECE, ne - lo);
            HIPCHK(hipMemcpyAsync(piece.data(), (const uint8_t *)d->tab + lo * GTB, cnt * GTB, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (size_t k = 0; k < cnt; k++) fp[lo + k] = piece[k * 72];
        }
    }
    if (gs.prof) prof_add_host("saver.index_readback", ms_since(t0));      // (the wait for the rounds above is in it)
    t0 = std::chrono::steady_clock::now();
    {
        std::vector<std::pair<uint64_t, uint16_t>> col(E);
        for (size_t j = 0; j < K; j++) {
            for (uint32_t k = 0; k < E; k++) col[k] = {fp[j * E + k] & d->mask, (uint16_t)(k + 1)};
            std::sort(col.begin(), col.end());
            for (uint32_t k = 0; k < E; k++) { fp[j * E + k] = col[k].first; ms[j * E + k] = col[k].second; }
        }
    }
    if (gs.prof) prof_add_host("saver.index_sort", ms_since(t0));
    HIPCHK(hipMemcpyAsync(d->fps, fp.data(), ne * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d->ms, ms.data(), ne * 2, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    guard.done = true;
    if (gs.prof) prof_flush(sl);
    undo.d = nullptr;
    *handle = register_handle(d, K, 15);
    return DGPU_OK;
}
int32_t dk_free(uint64_t handle) {
    Handle hd;
    if (!take_handle(handle, [](int k) { return k == 15; }, hd)) return DGPU_E_BADARG;
    CtxScope on_owner(hd.ctx);
    if (cur().device >= 0) (void)hipSetDevice(cur().device);
    release((SaverDk *)hd.p);
    return DGPU_OK;
}
// out[k] = T_j[first + k] = e(g_j, V_2_j)^(first + k), k < count: the reference's pairing_powers[j][first - 1 + k]
int32_t dk_powers(uint64_t handle, size_t j, size_t first, size_t count, uint64_t *out) {
    HandleRef h(handle);
    if (!dk_ok(h)) return DGPU_E_BADARG;
    const SaverDk &d = *(const SaverDk *)h.h.p;
    if (j >= d.K || first < 1 || first > d.E || count > d.E - first + 1 || (count && !out)) return DGPU_E_BADARG;
    if (count == 0) return DGPU_OK;
    if (!ctxs[h.h.ctx].ready) return DGPU_E_NODEVICE;
    CtxScope on_owner(h.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    HIPCHK(hipMemcpyAsync(out, (const uint8_t *)d.tab + (j * d.E + first - 1) * GTB, count * GTB, hipMemcpyDeviceToHost, sl.stream));
    HIPCHK(hipStreamSynchronize(sl.stream));
    return DGPU_OK;
}

// ---- the decryption pipeline: decrypt (nu_in == nullptr: the second side is -rho c_0_i, chunks and nu come back) and verify (the second side is -nu_i, the
// chunks are compared at their index; the check of nu against V_0, one more two-pair column, runs FIRST and on its own — over up to 4096 ciphertexts a pass —
// so that the chunk columns keep decrypt's geometry: rows x K <= 4096 slices, the one size k_miller_tail and k_final_exp are known to run well at) -------------------
struct DecCall { bool verify; const uint64_t *ct; size_t n; const uint64_t *sk; bool mont; uint16_t *chunks; uint64_t *nu; uint8_t *status; const uint16_t *claimed; const uint64_t *nu_in; };
int32_t dec_pipeline(uint64_t handle, const DecCall &c) {
    const bool verify = c.verify;
    if (c.n == 0) return DGPU_OK;
    if (!c.ct || !c.status || c.n >= (1ull << 31) || (verify ? (!c.claimed || !c.nu_in) : (!c.sk || !c.chunks || !c.nu))) return DGPU_E_BADARG;
    HandleRef h(handle);
    if (!dk_ok(h)) return DGPU_E_BADARG;
    if (!ctxs[h.h.ctx].ready) return DGPU_E_NODEVICE;
    const SaverDk &d = *(const SaverDk *)h.h.p;
    const size_t n = c.n, K = d.K, rw = (K + 2) * 12;
    CtxScope on_owner(h.h.ctx);
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = ct_chunk_rows(n, saverk::SAVER_PAIR_ROWS, K), chunk0 = verify ? ct_chunk_rows(n, saverk::SAVER_PAIR_ROWS, 1) : 0, big = std::max(chunk, chunk0);
    int32_t rc;
    // q[0]: the GLV split of -rho, q[1]: the c_0, q[2]: the second sides (-rho c_0 | -nu) and their identity flags, q[3]: the c_ij column-major,
    // q[5]: chunks | miss bytes | status, q[6]: the verdicts of the V_0 column (verify)
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[0].ensure(64))) return e;
        if ((e = o.q[1].ensure(big * PT))) return e;
        if ((e = o.q[2].ensure(big * PT + big + 16))) return e;
        if ((e = o.q[3].ensure(K * chunk * PT))) return e;
        if ((e = o.q[5].ensure(chunk * K * 3 + chunk + 16))) return e;
        if (verify && (e = o.q[6].ensure(n))) return e;
        return ws_pairs(o, 2 * std::max(K * chunk, chunk0), std::max(K * chunk, chunk0));
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<uint64_t> hc0(big * 12), hside(big * 12), hcols(K * chunk * 12);
    std::vector<uint8_t> hinf(chunk);
    DrainUnlessDone guard(sl);
    DeviceWipe dw(sl);
    uint32_t *dC0 = sl.q[1].as<uint32_t>(), *dSide = sl.q[2].as<uint32_t>(), *dCols = sl.q[3].as<uint32_t>();
    uint8_t *dSideInf = sl.q[2].as<uint8_t>() + big * PT, *dV0 = sl.q[6].as<uint8_t>();
    uint16_t *dChunks = sl.q[5].as<uint16_t>();
    uint8_t *dMiss = sl.q[5].as<uint8_t>() + chunk * K * 2, *dStatus = dMiss + chunk * K;
    if (!verify) {
        // -rho mod r as (k1 | k2), k1 + k2 lambda, both below 2^128 (host_field.hpp): what k_g1_scale_quad takes
        uint64_t w[4], split[4];
        fr_in(c.sk, c.mont).to_canonical(w);
        if (w[0] | w[1] | w[2] | w[3]) {
            uint64_t br = 0;
            for (int i = 0; i < 4; i++) { u128 t = (u128)FrH::MOD[i] - w[i] - br; w[i] = (uint64_t)t; br = (uint64_t)(t >> 64) & 1; }
        }
        hostf::glv_decompose(w, split, split + 2);
        dw.add(sl.q[0].p, 32);
        const hipError_t e = hipMemcpy(sl.q[0].p, split, 32, hipMemcpyHostToDevice);      // (synchronous: the host's copy goes right after it)
        volatile uint64_t *vw = w, *vs = split;
        for (int i = 0; i < 4; i++) { vw[i] = 0; vs[i] = 0; }
        HIPCHK(e);
    }
    const saverk::DkDev dk = d.dev();
    uint32_t *lines = sl.ml_lines.as<uint32_t>();
    for (size_t r0 = 0; verify && r0 < n; r0 += chunk0) {               // dV0[i] = [e(c_0_i, V_0) e(-nu_i, H) == 1]
        const size_t rows = std::min(chunk0, n - r0);
        for (size_t i = 0; i < rows; i++) { memcpy(&hc0[12 * i], c.ct + (r0 + i) * rw, PT); neg_g1(&hside[12 * i], c.nu_in + 12 * (r0 + i)); }
        HIPCHK(hipMemcpyAsync(dC0, hc0.data(), rows * PT, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dSide, hside.data(), rows * PT, hipMemcpyHostToDevice, s));
        { StageTimer st(sl, "saver.lines");
          launch_lines_from_prepared(s, dC0, d.pc_V0(), nullptr, rows, lines, 2 * rows, nullptr, true);
          launch_lines_from_prepared(s, dSide, d.pc_H(), nullptr, rows, lines + rows, 2 * rows, nullptr, true); }
        (void)value_tail(sl, rows, dk.one);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dV0 + r0, sl.flags.p, rows, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next pass's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0), m = K * rows, np = 2 * m;
        for (size_t i = 0; i < rows; i++) {
            const uint64_t *row = c.ct + (r0 + i) * rw;
            if (!verify) memcpy(&hc0[12 * i], row, PT);
            for (size_t j = 0; j < K; j++) memcpy(&hcols[(j * rows + i) * 12], row + 12 * (1 + j), PT);
            if (verify) neg_g1(&hside[12 * i], c.nu_in + 12 * (r0 + i));
        }
        HIPCHK(hipMemcpyAsync(dCols, hcols.data(), K * rows * PT, hipMemcpyHostToDevice, s));
        if (verify) {
            HIPCHK(hipMemcpyAsync(dSide, hside.data(), rows * PT, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(dSideInf, 0, rows, s));                    // (an identity nu is zero words: the line kernel sees that itself)
            HIPCHK(hipMemcpyAsync(dChunks, c.claimed + r0 * K, rows * K * 2, hipMemcpyHostToDevice, s));
        } else {
            HIPCHK(hipMemcpyAsync(dC0, hc0.data(), rows * PT, hipMemcpyHostToDevice, s));
            StageTimer st(sl, "saver.scale");
            msm::launch_g1_scale_quad(s, dC0, nullptr, sl.q[0].as<uint32_t>(), 0, nullptr, rows, dSide, dSideInf);
        }
        { StageTimer st(sl, "saver.lines");
          for (size_t j = 0; j < K; j++) {
              launch_lines_from_prepared(s, dCols + j * rows * 24, d.pc_V2(j), nullptr, rows, lines + j * rows, np, nullptr, true);
              launch_lines_from_prepared(s, dSide, d.pc_V1(j), dSideInf, rows, lines + m + j * rows, np, nullptr, true);
          } }
        const uint32_t *gt = value_tail(sl, m, nullptr);
        { StageTimer st(sl, "saver.lookup"); saverk::launch_gt_dlog_lookup(s, gt, rows, K, dk, verify, dChunks, dMiss); }
        { StageTimer st(sl, "saver.verdict");
          saverk::launch_saver_row_verdict(s, dMiss, rows, K, dChunks, verify ? dV0 + r0 : nullptr, verify, dStatus); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.status + r0, dStatus, rows, hipMemcpyDeviceToHost, s));
        if (!verify) {
            HIPCHK(hipMemcpyAsync(c.chunks + r0 * K, dChunks, rows * K * 2, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(hside.data(), dSide, rows * PT, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(hinf.data(), dSideInf, rows, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (!verify) for (size_t i = 0; i < rows; i++) {                 // nu_i = -(-rho c_0_i)
            if (hinf[i]) memset(c.nu + 12 * (r0 + i), 0, PT); else neg_g1(c.nu + 12 * (r0 + i), &hside[12 * i]);
        }
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    return DGPU_OK;
}

// ---- verify_ciphertext_commitment for n rows: e(c_0, Z_0) prod_j e(c_j, Z_j) e(-psi, H) == 1, a verdict per row ------------------------------------------------------
bool bad_K(size_t K) { return K < 1 || K > 255; }
int32_t commitment_each(const uint64_t *all_pc, size_t K, const uint64_t *ct, size_t n, uint8_t *ok) {
    if (n == 0) return DGPU_OK;
    if (bad_K(K) || !all_pc || !ct || !ok || n >= (1ull << 31)) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t nc = K + 2, rw = nc * 12;
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const size_t chunk = ct_chunk_rows(n, saverk::SAVER_COMMIT_PAIRS, nc);
    int32_t rc;
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[3].ensure(nc * chunk * PT))) return e;
        if ((e = o.ml_coeffs.ensure(nc * CW * 8 + 16))) return e;
        return ws_pairs(o, nc * chunk, chunk);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<uint64_t> hcols(nc * chunk * 12);
    DrainUnlessDone guard(sl);
    static const hostf::Fq12 one = hostf::Fq12::one();
    uint32_t *dCols = sl.q[3].as<uint32_t>(), *d_one = sl.ml_out.as<uint32_t>() + chunk * 144;
    HIPCHK(hipMemcpyAsync(sl.ml_coeffs.p, all_pc, nc * CW * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_one, &one, GTB, hipMemcpyHostToDevice, s));
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0), np = nc * rows;
        for (size_t i = 0; i < rows; i++) {
            const uint64_t *row = ct + (r0 + i) * rw;
            for (size_t k = 0; k <= K; k++) memcpy(&hcols[(k * rows + i) * 12], row + 12 * k, PT);
            neg_g1(&hcols[((K + 1) * rows + i) * 12], row + 12 * (K + 1));
        }
        HIPCHK(hipMemcpyAsync(dCols, hcols.data(), np * PT, hipMemcpyHostToDevice, s));
        { StageTimer st(sl, "saver.lines");
          for (size_t k = 0; k < nc; k++)
              launch_lines_from_prepared(s, dCols + k * rows * 24, sl.ml_coeffs.as<uint32_t>() + k * CW * 2, nullptr, rows, sl.ml_lines.as<uint32_t>() + k * rows, np, nullptr, true); }
        pair_tail(sl, rows, (int)nc, nullptr, nullptr, d_one);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ok + r0, sl.flags.p, rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the next chunk's operands overwrite this one's)
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;
    return DGPU_OK;
}

// ---- verify_commitments_in_batch: with w_i = r_powers[i], prod_k e(sum_i w_i col_k_i, Q_k) == 1 over the K + 2 columns (the last one negated) ---------------------------
int32_t commitments_batch(const uint64_t *all_pc, size_t K, const uint64_t *ct, size_t n, const uint64_t *r_powers, bool mont, int32_t *ok) {
    if (n == 0) { if (ok) *ok = 1; return DGPU_OK; }
    if (bad_K(K) || !all_pc || !ct || !r_powers || !ok || n >= (1ull << 31)) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    const size_t nc = K + 2;
    SLOT_ACQUIRE(LK, sl);
    HIPCHK(hipSetDevice(cur().device));
    const int forced = gs.many_chunk.load();
    const size_t chunk = std::min(n, forced > 0 ? (size_t)forced : saverk::SAVER_BATCH_CHUNK);
    int32_t rc;
    // q[3]: the rows as they came, q[4]: the K + 2 merged points and their skip flags, q[9]: the weights, q[10]: the prepared records of one column
    auto ws = [&](Slot &o) -> int32_t {
        int32_t e;
        if ((e = o.q[3].ensure(nc * chunk * PT))) return e;
        if ((e = o.q[4].ensure(nc * PT + nc + 64))) return e;
        if ((e = o.q[9].ensure(chunk * 32))) return e;
        if ((e = o.q[10].ensure(chunk * G1::AFF_STRIDE * 4))) return e;
        if ((e = ws_for<G1>(o, 2, chunk, 0, nullptr))) return e;
        if ((e = o.ml_coeffs.ensure(nc * CW * 8 + 16))) return e;
        if ((e = o.ml_lines.ensure((size_t)N_LINES * LW * nc * 4))) return e;
        return ws_check(o, 1);
    };
    if ((rc = ensure_workspace(sl, ws))) return rc;
    hipStream_t s = sl.stream;
    std::vector<HPoint> P(nc, HPoint::identity());
    DrainUnlessDone guard(sl);
    uint32_t *d_w = sl.q[9].as<uint32_t>(), *d_rec = sl.q[10].as<uint32_t>();
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t rows = std::min(chunk, n - r0);
        const uint8_t *raw = sl.q[3].as<uint8_t>();
        HIPCHK(hipMemcpyAsync(sl.q[3].p, ct + r0 * nc * 12, rows * nc * PT, hipMemcpyHostToDevice, s));
        if ((rc = upload_scalars(sl, r_powers + 4 * r0, rows, mont, d_w))) return rc;
        for (size_t k = 0; k < nc; k++) {
            { StageTimer st(sl, "msm.prep_bases"); prep_g1(s, raw + k * PT, nc * PT, rows, d_rec); }
            HIPCHK(hipGetLastError());
            if ((rc = msm_add(sl, d_rec, d_w, rows, P[k]))) return rc;
        }
        if (gs.prof) prof_flush(sl);
    }
    guard.done = true;                                                   // (every chunk's MSMs were waited for)
    if (!P[K + 1].inf) P[K + 1].y = P[K + 1].y.neg();                   // -sum w_i psi_i
    return merged_multi_verdict(sl, P, all_pc, sl.q[4], "saver.lines", ok);
}

}  // namespace

namespace {
const bool hooked = (dock::g_free_saver_dk = [](void *p) { release((SaverDk *)p); }, true);      // (dgpu_shutdown frees what is left of kind 15 through it)
}

extern "C" {
int32_t dgpu_saver_dk_create(const uint64_t *g_i, const uint64_t H[24], const uint64_t V_0[24], const uint64_t *V_1, const uint64_t *V_2, int32_t chunk_bit_size, size_t K,
                             uint64_t *handle) {
    return abi_guard([&] { return dk_create(g_i, H, V_0, V_1, V_2, chunk_bit_size, K, handle); });
}
int32_t dgpu_saver_dk_free(uint64_t dk) { return abi_guard([&] { return dk_free(dk); }); }
int32_t dgpu_saver_dk_powers(uint64_t dk, size_t j, size_t first, size_t count, uint64_t *out) { return abi_guard([&] { return dk_powers(dk, j, first, count, out); }); }
int32_t dgpu_saver_decrypt_many(uint64_t dk, const uint64_t *ct, size_t n, const uint64_t sk[4], int32_t montgomery, uint16_t *chunks, uint64_t *nu_xy, uint8_t *status) {
    return abi_guard([&] { return dec_pipeline(dk, DecCall{false, ct, n, sk, montgomery != 0, chunks, nu_xy, status, nullptr, nullptr}); });
}
int32_t dgpu_saver_verify_decryption_each(uint64_t dk, const uint64_t *ct, size_t n, const uint16_t *chunks, const uint64_t *nu_xy, uint8_t *ok) {
    return abi_guard([&] { return dec_pipeline(dk, DecCall{true, ct, n, nullptr, false, nullptr, nullptr, ok, chunks, nu_xy}); });
}
int32_t dgpu_saver_verify_commitment_each(const uint64_t *all_pc, size_t K, const uint64_t *ct, size_t n, uint8_t *ok) {
    return abi_guard([&] { return commitment_each(all_pc, K, ct, n, ok); });
}
int32_t dgpu_saver_verify_commitments_batch(const uint64_t *all_pc, size_t K, const uint64_t *ct, size_t n, const uint64_t *r_powers, int32_t montgomery, int32_t *ok) {
    return abi_guard([&] { return commitments_batch(all_pc, K, ct, n, r_powers, montgomery != 0, ok); });
}
}  // extern "C"
