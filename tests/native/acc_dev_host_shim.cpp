// tests/native/acc_dev_host_shim.cpp — the accumulator witness update's __host__ __device__ Fr routines (crypto_amd/csrc/acc_kernels.hip.h: add_step,
// rem_step, eval_chunk, combine_step, finish_share) compiled for the host with -DFP29_CHECK (every product asserts its operand contract), driven the
// way k_acc_eval and k_acc_combine drive them: K chunks per element, the finishing step over strided lane shares; and the host's tables that depend on
// the secret key (crypto_amd/csrc/acc_host_tables.hpp), as dock_accumulator.hip builds them.
// Built and loaded by tests/test_acc_device_code_on_host.py.
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

extern "C" {
// tables: canonical words [a (na) | F (na) | r (nr) | G (nr) | Phi]; y: m elements; K chunks per element; G lanes in the finishing step (lane g owns
// the elements g, g + G, ...); f, g: m x 8 canonical words each
void shim_acc_update(size_t na, size_t nr, const uint32_t *tables, size_t m, const uint32_t *y_words, size_t K, size_t G, uint32_t *f_out, uint32_t *g_out, int stress) {
    const size_t ne = 2 * na + 2 * nr + 1;
    std::vector<Fr> tab(ne), y(m);
    for (size_t e = 0; e < ne; e++) tab[e] = load(tables + 8 * e, stress);
    for (size_t i = 0; i < m; i++) y[i] = load(y_words + 8 * i, stress);
    const Fr *a = tab.data(), *F = a + na, *r = F + na, *Gs = r + nr, phi = tab[ne - 1];
    auto ta = [&](size_t s, Fr &u, Fr &v) { u = a[s]; v = F[s]; };
    auto tr = [&](size_t s, Fr &u, Fr &v) { u = r[s]; v = Gs[s]; };
    std::vector<Fr> part(4 * K * m), scratch(4 * m);
    if (K > 1)
        for (size_t c = 0; c < K; c++)
            for (size_t i = 0; i < m; i++) {
                Fr *p = &part[4 * (c * m + i)];
                acck::eval_chunk(y[i], na * c / K, na * (c + 1) / K, nr * c / K, nr * (c + 1) / K, ta, tr, p[0], p[1], p[2], p[3]);
            }
    for (size_t g = 0; g < G && g < m; g++) {
        const size_t n = (m - g + G - 1) / G;
        acck::finish_share(n, phi,
            [&](size_t k, Fr &PA, Fr &SA, Fr &PD, Fr &SD) {
                const size_t i = g + k * G;
                if (K == 1) { acck::eval_chunk(y[i], 0, na, 0, nr, ta, tr, PA, SA, PD, SD); return; }
                fr_one(PA); PD = PA; fr_zero(SA); fr_zero(SD);
                for (size_t c = 0; c < K; c++) { const Fr *p = &part[4 * (c * m + i)]; acck::combine_step(PA, SA, PD, SD, p[0], p[1], p[2], p[3]); }
            },
            [&](size_t k, int q, Fr &v) { v = scratch[4 * (g + k * G) + q]; }, [&](size_t k, int q, const Fr &v) { scratch[4 * (g + k * G) + q] = v; },
            [&](size_t k, const Fr &f, const Fr &gg) { fr_to_words(f_out + 8 * (g + k * G), f, false); fr_to_words(g_out + 8 * (g + k * G), gg, false); });
    }
}
// the host's tables [a | F | r | G | Phi] as ark-ff Montgomery words (4 x u64 each) into out; returns build_tables' code
int shim_acc_host_tables(const uint64_t *additions, size_t na, const uint64_t *removals, size_t nr, const uint64_t *alpha, int mont, uint64_t *out) {
    acch::Tables t;
    const int rc = acch::build_tables(additions, na, removals, nr, alpha, mont != 0, t);
    if (!rc) memcpy(out, t.w.data(), t.w.size() * 8);
    return rc;
}
}
