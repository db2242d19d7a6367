// tests/native/acc_issue_host.cpp — the host's share of today's recipe for issuing witnesses, natively and on several threads, so that
// tests/perf/acc_issue_timing.py can time the recipe whole: the scalars (f_V - d_i) / (y_i + alpha) (with_d) or 1 / (y_i + alpha), one batch inversion per
// thread, canonical words in and out, with the library's own host field (crypto_amd/csrc/host_field.hpp, acc_host_tables.hpp).  The scalars then go through
// dgpu_window_table_g1 + dgpu_window_table_mul_g1.  Built and loaded by that script.
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include "../../crypto_amd/csrc/acc_host_tables.hpp"
using acch::FrH;

static FrH fr_neg(const FrH &a) {
    if (acch::fr_is_zero(a)) return a;
    FrH r; uint64_t br = 0;
    for (int i = 0; i < 4; i++) { acch::u128 d = (acch::u128)FrH::MOD[i] - a.l[i] - br; r.l[i] = (uint64_t)d; br = (uint64_t)(d >> 64) & 1; }
    return r;
}

extern "C" int acc_issue_scalars_host(const uint64_t *d, const uint64_t *ys, size_t m, const uint64_t *f_v, const uint64_t *alpha, int with_d, int threads, uint64_t *out) {
    std::vector<uint64_t> t(m * 4);
    const size_t T = threads < 1 ? 1 : (size_t)threads;
    std::vector<int> rc(T, 0);
    auto work = [&](size_t k) {
        const size_t lo = m * k / T, hi = m * (k + 1) / T;
        rc[k] = acch::issue_inverses(ys, lo, hi, alpha, false, t.data());
        if (rc[k]) return;
        const FrH fv = with_d ? acch::fr_in(f_v, false) : FrH::from_u64(0);
        for (size_t i = lo; i < hi; i++) {
            FrH s; memcpy(s.l, &t[4 * i], 32);
            if (with_d) s = acch::fr_plus(fv, fr_neg(acch::fr_in(d + 4 * i, false))) * s;
            s.to_canonical(out + 4 * i);
        }
    };
    std::vector<std::thread> pool;
    for (size_t k = 0; k < T; k++) pool.emplace_back(work, k);
    for (auto &th : pool) th.join();
    for (int e : rc) if (e) return e;
    return 0;
}
