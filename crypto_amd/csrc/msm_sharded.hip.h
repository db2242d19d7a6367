// crypto_amd/csrc/msm_sharded.hip.h — the MSM entry points over several device contexts of one process.
#pragma once
#include "msm_driver.hip.h"

namespace dock {

// ---- several GPUs behind the ABI (SURVEY.md 8b `dgpu_msm_g1_sharded`, 8e point-chunk sharding) ----------------------------------------
// One process, one context per device, one host thread per device inside the call: device k runs the whole pipeline on the terms
// [lo_k, lo_{k+1}) and hands back one normalised Jacobian point (144 / 288 B); the partials are folded on the host.  No collective is
// needed inside a process; the multi-process form (one rank per GPU, RCCL all_gather of the same partials) stays above the ABI.
template <class C, class HF>
int32_t msm_sharded_oneshot(const uint64_t *bases, const uint8_t *is_inf, const uint64_t *scalars, size_t n, int32_t ngpus, bool mont, uint64_t *out) {
    if (!out || (n && (!bases || !scalars)) || n >= (1ull << 31) || ngpus < 0) return DGPU_E_BADARG;
    const std::vector<int> cx = ready_contexts(ngpus);
    if (cx.empty()) return DGPU_E_NODEVICE;
    if (ngpus > 0 && (int)cx.size() < ngpus) return DGPU_E_BADARG;
    if (!tl_no_min && n < gs.min_gpu_n) return DGPU_E_TOO_SMALL;
    std::vector<size_t> lo; shard_bounds(n, cx.size(), lo);
    const size_t JW = 3 * sizeof(HF) / 8, BW = 2 * sizeof(HF) / 8;
    std::vector<uint64_t> parts(cx.size() * JW);
    int32_t rc = run_shards(cx.size(), [&](size_t k) {
        CtxScope here(cx[k]);
        const size_t cnt = lo[k + 1] - lo[k];
        return msm_oneshot_here<C, HF>(RawBases::packed<C>(bases + lo[k] * BW, is_inf ? is_inf + lo[k] : nullptr), scalars + lo[k] * 4, cnt, mont, parts.data() + k * JW);
    });
    if (rc) return rc;
    return host_fold_jacobian<HF>(parts.data(), cx.size(), out);
}
template <class C>
int32_t bases_upload_sharded(const uint64_t *bases, const uint8_t *is_inf, size_t n, int32_t ngpus, uint64_t *handle, int kind /* 1 | 2 */) {
    if (!handle || (n && !bases) || n >= (1ull << 31) || ngpus < 0) return DGPU_E_BADARG;
    const std::vector<int> cx = ready_contexts(ngpus);
    if (cx.empty()) return DGPU_E_NODEVICE;
    if (ngpus > 0 && (int)cx.size() < ngpus) return DGPU_E_BADARG;
    ShardSet *ss = new ShardSet();
    ss->n = n; ss->sub.assign(cx.size(), 0); shard_bounds(n, cx.size(), ss->lo);
    const size_t BW = 2 * C::ABI_W / 2;           // u64 words per affine point
    int32_t rc = run_shards(cx.size(), [&](size_t k) {
        CtxScope here(cx[k]);
        return bases_upload<C>(RawBases::packed<C>(bases + ss->lo[k] * BW, is_inf ? is_inf + ss->lo[k] : nullptr), ss->lo[k + 1] - ss->lo[k], &ss->sub[k], kind);
    });
    if (rc) { for (uint64_t h : ss->sub) if (h) (void)dgpu_bases_free(h); delete ss; return rc; }
    *handle = register_handle(ss, n, kind + 6);       // 7 = G1 sharded, 8 = G2 sharded
    return DGPU_OK;
}
// fresh host scalars against a sharded bases handle: shard k uploads and uses scalars [lo_k, min(lo_{k+1}, n))
template <class C, class HF>
int32_t msm_sharded_handle(uint64_t bases, const uint64_t *scalars, size_t n, int mont, uint64_t *out, int kind) {
    if (!out || (n && !scalars)) return DGPU_E_BADARG;
    HandleRef hb(bases);
    if (!hb.ok || hb.h.kind != kind + 6 || n > hb.h.n) return DGPU_E_BADARG;
    if (!tl_no_min && n < gs.min_gpu_n) return DGPU_E_TOO_SMALL;
    const ShardSet &ss = *(const ShardSet *)hb.h.p;
    const size_t G = ss.sub.size(), JW = 3 * sizeof(HF) / 8;
    std::vector<uint64_t> parts(G * JW);
    int32_t rc = run_shards(G, [&](size_t k) {
        const size_t lo = std::min(ss.lo[k], n), hi = std::min(ss.lo[k + 1], n);
        return msm_handle<C, HF>(ss.sub[k], 0, scalars + lo * 4, hi - lo, mont, parts.data() + k * JW, kind, false);
    });
    if (rc) return rc;
    return host_fold_jacobian<HF>(parts.data(), G, out);
}
// both operands resident on their devices (inputs pre-sharded: BASELINE config 5's timed region)
template <class C, class HF>
int32_t msm_sharded_resident(uint64_t bases, uint64_t scalars, uint64_t *out, int kind) {
    if (!out) return DGPU_E_BADARG;
    HandleRef hb(bases), hs(scalars);
    if (!hb.ok || !hs.ok || hb.h.kind != kind + 6 || hs.h.kind != 9) return DGPU_E_BADARG;
    const ShardSet &sb = *(const ShardSet *)hb.h.p, &sv = *(const ShardSet *)hs.h.p;
    if (sb.sub.size() != sv.sub.size() || sv.n > sb.n) return DGPU_E_BADARG;
    for (size_t k = 0; k < sb.sub.size(); k++) if (sv.lo[k] != std::min(sb.lo[k], sv.n) || sv.lo[k + 1] != std::min(sb.lo[k + 1], sv.n)) return DGPU_E_BADARG;
    if (sv.n < gs.min_gpu_n) return DGPU_E_TOO_SMALL;
    const size_t G = sb.sub.size(), JW = 3 * sizeof(HF) / 8;
    std::vector<uint64_t> parts(G * JW);
    int32_t rc = run_shards(G, [&](size_t k) { return msm_resident<C, HF>(sb.sub[k], 0, sv.sub[k], 0, sv.lo[k + 1] - sv.lo[k], parts.data() + k * JW, kind, false); });
    if (rc) return rc;
    return host_fold_jacobian<HF>(parts.data(), G, out);
}

}  // namespace dock
