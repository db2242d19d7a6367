// tests/native/saver_dev_host_shim.cpp — host build (g++) of the DEVICE routines of the SAVER kernels (crypto_amd/csrc/saver_kernels.hip.h): the discrete-log
// lookup and the row verdict — the very functions k_gt_dlog_lookup and k_saver_row_verdict call — over whatever table the test hands in, and the group body of
// k_gt_table_extend under the FP29_CHECK worst-case bound tracker, six host threads playing the six lanes of a group as in gt_pow_host_shim.cpp.  Test-only:
// tests/test_saver_device_code_on_host.py drives it; an assertion that fires inside means a lazy-limb overflow is possible for some input.
#define FP29_CHECK 1
#include "../../crypto_amd/csrc/saver_kernels.hip.h"
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
    void barrier() {
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
    bool wave_all(bool v) { return all(v); }
};
template <class Fn> void run_group(Fn fn) {
    Group g;
    std::vector<std::thread> th;
    for (int e = 0; e < GT_LANES; e++) th.emplace_back([&, e] { HostLanes x{&g, e}; fn(x, e); });
    for (auto &t : th) t.join();
}
}  // namespace

extern "C" {
// the whole table of ONE column from its base, by the rounds dock_saver.hip launches: tab holds E entries of 72 words, entry 0 is the base on entry
void shim_table_from_base(uint64_t *tab, uint32_t E) {
    uint32_t *t = (uint32_t *)tab;
    for (uint32_t half = 1; half < E; half *= 2) {
        const uint32_t cnt = half < E - half ? half : E - half;
        for (uint32_t k = 1; k <= cnt; k++)
            run_group([&](HostLanes &x, int) { saverk::table_extend_group(x, t + (size_t)(half - 1) * GT_ABIW, t + (size_t)(k - 1) * GT_ABIW, t + (size_t)(half + k - 1) * GT_ABIW); });
    }
}
// saverk::dlog_lookup as the kernel calls it
int shim_lookup(const uint64_t *p, const uint64_t *one, const uint64_t *tab, const uint64_t *fps, const uint16_t *ms, uint32_t E, uint64_t mask, int at_index, uint32_t m) {
    return saverk::dlog_lookup((const uint32_t *)p, (const uint32_t *)one, (const uint32_t *)tab, fps, ms, E, mask, at_index != 0, m);
}
uint64_t shim_fingerprint(const uint64_t *el, uint64_t mask) { return saverk::fingerprint((const uint32_t *)el, mask); }
int shim_row_verdict(const uint8_t *miss, size_t K, uint16_t *chunks) { return saverk::row_verdict(miss, K, chunks); }
}
