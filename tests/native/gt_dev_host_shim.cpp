// tests/native/gt_dev_host_shim.cpp — host build (g++) of the DEVICE GT routines (crypto_amd/csrc/gt_kernels.hip.h) with the FP29_CHECK worst-case
// bound tracker.  Six host threads play the six lanes of a group: a shared array stands in for the group's LDS slots and a barrier for the wave's
// lock step, so the very code of k_gt.hip runs here.  Test-only: tests/test_gt_device_code_on_host.py compares it with dgpu_final_exponentiation and
// the oracles; an assertion that fires inside means a lazy-limb overflow is possible for some input.
#define FP29_CHECK 1
#include "../../crypto_amd/csrc/gt_kernels.hip.h"
#include <string.h>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
using namespace bls29;

namespace {
struct Group {
    Fp2 slots[GT_SLOTS][GT_LANES];
    bool flags[GT_LANES];
    std::mutex mu; std::condition_variable cv; int waiting = 0; unsigned gen = 0;
    void barrier() {
        std::unique_lock<std::mutex> l(mu);
        const unsigned g = gen;
        if (++waiting == GT_LANES) { waiting = 0; gen++; cv.notify_all(); }
        else cv.wait(l, [&] { return gen != g; });
    }
};
struct HostLanes {
    Group *g; int e;
    int lane() const { return e; }
    Fp2 *slot(int j) { return g->slots[j]; }
    void sync() { g->barrier(); }
    bool all(bool v) { sync(); g->flags[e] = v; sync(); bool r = true; for (int k = 0; k < GT_LANES; k++) r = r && g->flags[k]; return r; }
};
template <class Fn> void run_group(Fn fn) {
    Group g;
    std::vector<std::thread> th;
    for (int e = 0; e < GT_LANES; e++) th.emplace_back([&, e] { HostLanes x{&g, e}; fn(x, e); });
    for (auto &t : th) t.join();
}
// coefficient e (w-order) of an ABI element (72 u64: tower order, Fp2 halves)
void load(Fp2 &v, const uint64_t *f, int e) {
    uint32_t w[24]; memcpy(w, f + 12 * gt_tower_of(e), 96);
    fp_from_abi(v.c0, w); fp_from_abi(v.c1, w + 12);
}
void store(uint64_t *f, int e, const Fp2 &v) {
    uint32_t w[24]; fp_to_abi(w, v.c0); fp_to_abi(w + 12, v.c1);
    memcpy(f + 12 * gt_tower_of(e), w, 96);
}
}  // namespace

extern "C" {
// what k_final_exp computes for one element: GT words (zero for a zero input) and the zero flag
int shim_final_exp(const uint64_t *in, uint64_t *out) {
    int zero = 0;
    run_group([&](HostLanes &x, int e) {
        uint32_t w[24], any = 0; memcpy(w, in + 12 * gt_tower_of(e), 96);
        for (int k = 0; k < 24; k++) any |= w[k];
        const bool z = x.all(any == 0);
        Fp2 f, r; load(f, in, e);
        gt_final_exp(x, r, f);
        if (z) { fzero(r); if (e == 0) zero = 1; }
        store(out, e, r);
    });
    return zero;
}
// one step alone: 0 product, 1 cyclotomic squaring, 2 Frobenius p, 3 Frobenius p^2, 4 inverse, 5 conjugation, 6 exp_by_x
void shim_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    run_group([&](HostLanes &x, int e) {
        Fp2 u, v, r; load(u, a, e);
        if (b) load(v, b, e);
        switch (op) {
            case 0: gt_mul(x, r, u, v); break;
            case 1: gt_cyc_sqr(x, r, u); break;
            case 2: gt_frob1(r, u, e); break;
            case 3: gt_frob2(r, u, e); break;
            case 4: gt_inv(x, r, u); break;
            case 5: gt_conj(r, u, e); break;
            default: gt_exp_by_x(x, r, u); break;
        }
        store(out, e, r);
    });
}
// the Miller tail over 68 per-step products given in ABI form (68 x 72 words)
void shim_miller_tail(const uint64_t *L, uint64_t *out) {
    run_group([&](HostLanes &x, int e) {
        auto ld = [&](int s, Fp2 &v) { load(v, L + 72 * s, e); };
        Fp2 r; gt_miller_tail(x, r, ld);
        store(out, e, r);
    });
}
}
