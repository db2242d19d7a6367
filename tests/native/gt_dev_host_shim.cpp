// tests/native/gt_dev_host_shim.cpp — host build (g++) of the DEVICE GT routines (crypto_amd/csrc/gt_kernels.hip.h) with the FP29_CHECK worst-case
// bound tracker.  Six host threads play the six lanes of a group: a shared array stands in for the group's LDS slots and a barrier for the wave's
// lock step, so the very code of k_gt.hip runs here.  Test-only: tests/test_gt_device_code_on_host.py compares it with dgpu_final_exponentiation and
// the oracles; an assertion that fires inside means a lazy-limb overflow is possible for some input.
#define FP29_CHECK 1
#include "../../crypto_amd/csrc/gt_kernels.hip.h"
#include "../../crypto_amd/csrc/selftest_gt_kernels.hip.h"
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

// ---- the wrappers of the device self-tests (selftest_gt_kernels.hip.h), the same bodies k_selftest_gt runs, a group of six threads per row: n rows of
// in_words u64 in, out_words u64 out; stress = reps | G << 8 as on the device (G, the groups per wave, means nothing here).  0: done; -3: no such op,
// or a row shape that is not the op's ----
template <int OP> static int gt_rows(int reps, const uint64_t *in, size_t in_words, size_t n, uint64_t *out, size_t out_words) {
    using O = selftest::StOp<OP>;
    if (in_words != (size_t)O::IN64 || out_words != (size_t)O::OUT64) return -3;
    for (size_t i = 0; i < n; i++)
        run_group([&](HostLanes &x, int) { O::run(x, reinterpret_cast<const uint32_t *>(in + i * in_words), reinterpret_cast<uint32_t *>(out + i * out_words), reps); });
    return 0;
}
extern "C" int shim_selftest_gt(int op, int stress, const uint64_t *in, size_t in_words, size_t n, uint64_t *out, size_t out_words) {
    using namespace selftest;
    const int reps = stress & 0xff;
    if (stress < 0 || reps > 64) return -3;
    switch (op) {
#define X(ID) case ID: return gt_rows<ID>(reps, in, in_words, n, out, out_words);
        X(ST_GT_ROUNDTRIP) X(ST_GT_CONJ) X(ST_GT_NEG) X(ST_GT_MUL) X(ST_GT_SQR_BY_MUL) X(ST_GT_CYC_SQR) X(ST_GT_FROB1) X(ST_GT_FROB2) X(ST_GT_INV) X(ST_GT_EXP_BY_X)
        X(ST_GT_FINAL_EXP) X(ST_GT_MEMBERSHIP) X(ST_GT_SHRINK) X(ST_GT_TAIL_STEP)
#undef X
        case ST_GT_DIGITS: {
            using O = StOp<ST_GT_DIGITS>;
            if (in_words != (size_t)O::IN64 || out_words != (size_t)O::OUT64) return -3;
            for (size_t i = 0; i < n; i++) O::run(reinterpret_cast<const uint32_t *>(in + i * in_words), reinterpret_cast<uint32_t *>(out + i * out_words), stress);
            return 0;
        }
        default: return -3;
    }
}
