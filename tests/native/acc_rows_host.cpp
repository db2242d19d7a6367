// tests/native/acc_rows_host.cpp — the host's share of today's recipe for the public witness update, natively and on several threads, so that
// tests/perf/acc_public_timing.py can time the recipe whole: per holder d_A(y), d_D(y), f = d_A / d_D, s = 1 / d_D (one inversion per holder) and the row
// [s, s y, .., s y^(n-1)] (Omega::scaled_powers_of_y, vb_accumulator/src/batch_utils.rs:678-691), canonical words in and out, with the library's own host
// field (crypto_amd/csrc/host_field.hpp, acc_host_tables.hpp).  Built and loaded by that script.
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

extern "C" void acc_rows_host(const uint64_t *adds, size_t na, const uint64_t *rems, size_t nr, const uint64_t *ys, size_t m, size_t n, int threads,
                              uint64_t *f_out, uint64_t *rows) {
    std::vector<FrH> a(na), r(nr);
    for (size_t s = 0; s < na; s++) a[s] = acch::fr_in(adds + 4 * s, false);
    for (size_t s = 0; s < nr; s++) r[s] = acch::fr_in(rems + 4 * s, false);
    auto work = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            const FrH y = acch::fr_in(ys + 4 * i, false), my = fr_neg(y);
            FrH da = FrH::from_u64(1), dd = da;
            for (size_t s = 0; s < na; s++) da = da * acch::fr_plus(a[s], my);
            for (size_t s = 0; s < nr; s++) dd = dd * acch::fr_plus(r[s], my);
            FrH cur = dd.inv();
            (da * cur).to_canonical(f_out + 4 * i);
            for (size_t j = 0; j < n; j++) { cur.to_canonical(rows + 4 * (i * n + j)); cur = cur * y; }
        }
    };
    std::vector<std::thread> pool;
    const size_t T = threads < 1 ? 1 : (size_t)threads;
    for (size_t t = 0; t < T; t++) pool.emplace_back(work, m * t / T, m * (t + 1) / T);
    for (auto &th : pool) th.join();
}
