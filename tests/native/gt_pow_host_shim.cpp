// tests/native/gt_pow_host_shim.cpp — host build (g++) of the DEVICE GT power routines (crypto_amd/csrc/gt_kernels.hip.h: signed digits, the
// windowed cyclotomic power over a table, the generic power, the fold level and the membership tests) with the FP29_CHECK worst-case bound
// tracker.  Six host threads play the six lanes of a group, as in gt_dev_host_shim.cpp: a shared array for the group's LDS slots, a barrier for
// the wave's lock step, so the group bodies that k_gt_pow.hip launches run here as they are.  Test-only: tests/test_gt_pow_device_code_on_host.py
// compares the words with dgpu_fp12_pow / dgpu_fp12_multi_pow / dgpu_gt_in_subgroup and the oracle; an assertion that fires inside means a
// lazy-limb overflow is possible for some input.
#define FP29_CHECK 1
#include "../../crypto_amd/csrc/gt_kernels.hip.h"
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>
using namespace bls29;

namespace {
struct Group {
    Fp2 slots[GT_SLOTS][GT_LANES];
    bool flags[GT_LANES];
    std::atomic<int> waiting{0}; std::atomic<unsigned> gen{0};
    void barrier() {                                  // spins, then yields: the groups here run thousands of exchanges per power
        const unsigned g = gen.load(std::memory_order_acquire);
        if (waiting.fetch_add(1, std::memory_order_acq_rel) + 1 == GT_LANES) { waiting.store(0, std::memory_order_relaxed); gen.store(g + 1, std::memory_order_release); }
        else { int spins = 0; while (gen.load(std::memory_order_acquire) == g) if (++spins > 4000) std::this_thread::yield(); }
    }
};
struct HostLanes {
    Group *g; int e;
    int lane() const { return e; }
    Fp2 *slot(int j) { return g->slots[j]; }
    void sync() { g->barrier(); }
    bool all(bool v) { sync(); g->flags[e] = v; sync(); bool r = true; for (int k = 0; k < GT_LANES; k++) r = r && g->flags[k]; return r; }
    bool wave_all(bool v) { return all(v); }          // (the "wave" here is this one group)
};
template <class Fn> void run_group(Fn fn) {
    Group g;
    std::vector<std::thread> th;
    for (int e = 0; e < GT_LANES; e++) th.emplace_back([&, e] { HostLanes x{&g, e}; fn(x, e); });
    for (auto &t : th) t.join();
}
}  // namespace

extern "C" {
void shim_signed_digits(const uint64_t e[4], int8_t d[65]) {
    uint32_t w[8]; memcpy(w, e, 32);
    gt_signed_digits(w, d);
}
// what one group of k_gt_pow computes for k bases (a: k x 72 words, e: k x 4 words, or 4 words when e_stride == 0); missing = bases past nb that the
// group still has room for (they count as one); force_generic != 0 runs the generic path whatever the bases are.  Returns 1 if the short path ran.
int shim_pow_group(const uint64_t *a, const uint64_t *e, int e_stride, int nb, int k, int force_generic, int out_abi, uint64_t *out) {
    std::vector<uint32_t> tab((size_t)k * GT_TAB * GT_ELW), res(GT_ELW > GT_ABIW ? GT_ELW : GT_ABIW);
    int cyc[GT_LANES] = {};
    run_group([&](HostLanes &x, int lane) {
        uint64_t cm[GT_MAX_K];
        // (the path taken is the group's verdict on its bases: recomputed here for the caller, the group body decides for itself)
        bool c = true;
        for (int j = 0; j < k && j < nb; j++) { Fp2 f; gt_get_abi(f, (const uint32_t *)(a + 72 * j), lane); const bool cj = gt_in_cyclotomic(x, f); c = c && cj; }
        cyc[lane] = c && !force_generic;
        gt_pow_group(x, (const uint32_t *)a, (const uint32_t *)e, e_stride * 2, (size_t)nb, 0, k, tab.data(), cm, 1, force_generic != 0, res.data(), out_abi != 0);
    });
    if (out_abi) memcpy(out, res.data(), GT_ABIW * 4);
    else {                                           // internal form -> ABI through one more group
        run_group([&](HostLanes &x, int lane) { Fp2 v; gt_get(v, res.data() + lane * GT_TABW); gt_put_abi((uint32_t *)out, lane, v); });
    }
    return cyc[0];
}
// one level of k_gt_fold over n_in ABI elements: ceil(n_in / 8) ABI elements out; through_internal != 0 writes the internal form first and
// converts with a second, single-input level (the copy case), as the drivers do between levels
int shim_fold_level(const uint64_t *in, int n_in, int through_internal, uint64_t *out) {
    const int ng = (n_in + GT_FOLD - 1) / GT_FOLD;
    std::vector<uint32_t> mid((size_t)ng * GT_ELW);
    for (int i = 0; i < ng; i++) {
        if (!through_internal) { run_group([&](HostLanes &x, int) { gt_fold_group(x, (const uint32_t *)in, true, (size_t)n_in, (size_t)i * GT_FOLD, (uint32_t *)(out + 72 * i), true); }); continue; }
        run_group([&](HostLanes &x, int) { gt_fold_group(x, (const uint32_t *)in, true, (size_t)n_in, (size_t)i * GT_FOLD, mid.data() + (size_t)i * GT_ELW, false); });
        run_group([&](HostLanes &x, int) { gt_fold_group(x, mid.data() + (size_t)i * GT_ELW, false, 1, 0, (uint32_t *)(out + 72 * i), true); });
    }
    return ng;
}
// bit 0: in the cyclotomic subgroup, bit 1: in GT
int shim_membership(const uint64_t *a) {
    int r = 0;
    run_group([&](HostLanes &x, int lane) {
        Fp2 f; gt_get_abi(f, (const uint32_t *)a, lane);
        const bool c = gt_in_cyclotomic(x, f), g = gt_in_gt(x, f);
        if (lane == 0) r = (c ? 1 : 0) | (g ? 2 : 0);
    });
    return r;
}
}
