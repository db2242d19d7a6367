// tests/native/acc_issue_dev_host_shim.cpp — the __host__ __device__ Fr routines that issue accumulator witnesses (crypto_amd/csrc/acc_kernels.hip.h: d_chunk<1>,
// d_chunk<4>, d_times, issue_scalar) compiled for the host with -DFP29_CHECK (every product asserts its operand contract), driven the way k_acc_d /
// k_acc_d_combine / k_acc_issue_scalars and dock_accumulator.hip's passes drive them; and the host's inverses 1 / (y + alpha)
// (crypto_amd/csrc/acc_host_tables.hpp issue_inverses), share by share.  Built and loaded by tests/test_acc_issue_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/acc_kernels.hip.h"
#include "../../crypto_amd/csrc/acc_host_tables.hpp"
using namespace fr29;

static Fr load(const uint32_t *w, int stress) {
    Fr x; fr_from_words(x, w, false);                   // a product: < 2 r
    if (stress) {                                       // the same element pushed towards the top of its bound: + r, normalised
        constexpr uint32_t P_[NL] = FR29_R; Fr p; fr_const(p, P_);
        fr_add(x, x, p); fr_norm(x, x);
    }
    return x;
}

// one call: the members in passes of `pass`, every pass in K chunks (chunk c = [len c / K, len (c + 1) / K): empty for K > len), lane g of G = ceil(m / U)
// owning the non-members g + j G; K = 1 finishes in place, K > 1 through the chunk products; the running products live in `run` between passes
template <int U> static void d_call(size_t n, const uint32_t *member_words, size_t m, const uint32_t *y_words, size_t K, size_t pass, const uint32_t *d_in, uint32_t *d_out, uint8_t *nz,
                                    int stress) {
    const size_t G = (m + U - 1) / U;
    std::vector<Fr> y(m), run(m), part(K * m), tab;
    for (size_t i = 0; i < m; i++) y[i] = load(y_words + 8 * i, stress);
    for (size_t lo = 0;; lo += pass) {
        const size_t len = n - lo < pass ? n - lo : pass;
        const bool first = lo == 0, last = lo + len >= n;
        tab.resize(len);
        for (size_t e = 0; e < len; e++) tab[e] = load(member_words + 8 * (lo + e), stress);
        auto start = [&](Fr &D, size_t i) { if (!first) D = run[i]; else if (d_in) D = load(d_in + 8 * i, stress); else fr_one(D); };
        auto finish = [&](const Fr &D, size_t i) {
            if (!last) { run[i] = D; return; }
            fr_to_words(d_out + 8 * i, D, false); nz[i] = acck::is_zero(D) ? 0 : 1;
        };
        for (size_t c = 0; c < K; c++)
            for (size_t g = 0; g < G; g++) {
                const size_t left = (m - g + G - 1) / G;
                const int owned = (int)(left < (size_t)U ? left : (size_t)U);
                Fr yy[U], P[U];
                for (int j = 0; j < U; j++) { if (j < owned) yy[j] = y[g + j * G]; else fr_zero(yy[j]); }
                acck::d_chunk<U>(yy, owned, len * c / K, len * (c + 1) / K, [&](size_t s, Fr &a) { a = tab[s]; }, P);
                for (int j = 0; j < owned; j++) {
                    const size_t i = g + j * G;
                    if (K == 1) { Fr D; start(D, i); acck::d_times(D, P[j]); finish(D, i); }
                    else part[c * m + i] = P[j];
                }
                Fr one; fr_one(one);
                for (int j = owned; j < U; j++) if (memcmp(&P[j], &one, sizeof one)) __builtin_trap();      // a chain the lane does not own was skipped
            }
        if (K > 1)
            for (size_t i = 0; i < m; i++) {
                Fr D; start(D, i);
                for (size_t c = 0; c < K; c++) acck::d_times(D, part[c * m + i]);
                finish(D, i);
            }
        if (last) break;
    }
}

extern "C" {
// members: n x 8 canonical words; y: m x 8; d_in: m x 8 or NULL; d_out: m x 8 canonical words; nz: m bytes.  U = 1 or 4
void shim_d_for_batch(int U, size_t n, const uint32_t *members, size_t m, const uint32_t *y, size_t K, size_t pass, const uint32_t *d_in, uint32_t *d_out, uint8_t *nz, int stress) {
    if (U == 4) d_call<4>(n, members, m, y, K, pass, d_in, d_out, nz, stress);
    else d_call<1>(n, members, m, y, K, pass, d_in, d_out, nz, stress);
}
// sc: m x 8 canonical words, zero: m bytes; with_d = 0: d and fv are not read
void shim_issue_scalars(size_t m, const uint32_t *d, const uint32_t *t, const uint32_t *fv, int with_d, uint32_t *sc, uint8_t *zero, int stress) {
    for (size_t i = 0; i < m; i++) {
        Fr f, di, s; fr_zero(f); fr_zero(di);
        if (with_d) { f = load(fv, stress); di = load(d + 8 * i, stress); }
        zero[i] = acck::issue_scalar(s, with_d != 0, f, di, load(t + 8 * i, stress)) ? 1 : 0;
        fr_to_words(sc + 8 * i, s, false);
    }
}
// t_i = 1 / (y_i + alpha) as ark-ff Montgomery words (4 x u64 each), in `shares` shares as the host threads cut them; returns the first non-zero code
int shim_issue_inverses(const uint64_t *ys, size_t m, const uint64_t *alpha, int mont, size_t shares, uint64_t *t) {
    int rc = 0;
    for (size_t k = 0; k < shares; k++) {
        const int e = acch::issue_inverses(ys, m * k / shares, m * (k + 1) / shares, alpha, mont != 0, t);
        if (e && !rc) rc = e;
    }
    return rc;
}
}
