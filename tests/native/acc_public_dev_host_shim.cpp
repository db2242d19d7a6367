// tests/native/acc_public_dev_host_shim.cpp — the __host__ __device__ Fr routines of the accumulator's update from public information
// (crypto_amd/csrc/acc_kernels.hip.h: omega_value, omega_pair, pub_chunk, pub_finish_share, pub_row_run) compiled for the host with -DFP29_CHECK (every
// product asserts its operand contract), driven the way k_acc_omega_eval / k_acc_omega_combine / k_acc_omega_coeffs, k_acc_pub_factors /
// k_acc_pub_combine and k_acc_pub_rows drive them.  Built and loaded by tests/test_acc_public_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/acc_kernels.hip.h"
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
// the raw finishing mode: v_AD at the N points, K chunks per point.  tables: canonical words [a (na) | F (na) | r (nr) | G (nr) | Phi]; out: N x 8 canonical words
void shim_omega_values(size_t na, size_t nr, const uint32_t *tables, size_t N, const uint32_t *pts, size_t K, uint32_t *out, int stress) {
    const size_t ne = 2 * na + 2 * nr + 1;
    std::vector<Fr> tab(ne);
    for (size_t e = 0; e < ne; e++) tab[e] = load(tables + 8 * e, stress);
    const Fr *a = tab.data(), *F = a + na, *r = F + na, *Gs = r + nr, phi = tab[ne - 1];
    auto ta = [&](size_t s, Fr &u, Fr &v) { u = a[s]; v = F[s]; };
    auto tr = [&](size_t s, Fr &u, Fr &v) { u = r[s]; v = Gs[s]; };
    for (size_t i = 0; i < N; i++) {
        const Fr y = load(pts + 8 * i, stress);
        Fr PA, SA, PD, SD, v;
        if (K == 1) acck::eval_chunk(y, 0, na, 0, nr, ta, tr, PA, SA, PD, SD);
        else {
            fr_one(PA); PD = PA; fr_zero(SA); fr_zero(SD);
            for (size_t c = 0; c < K; c++) {
                Fr p[4];
                acck::eval_chunk(y, na * c / K, na * (c + 1) / K, nr * c / K, nr * (c + 1) / K, ta, tr, p[0], p[1], p[2], p[3]);
                acck::combine_step(PA, SA, PD, SD, p[0], p[1], p[2], p[3]);
            }
        }
        acck::omega_value(v, SA, SD, phi);
        for (int l = 0; l < NL; l++) if (v.l[l] >> 29) __builtin_trap();      // a product, as the transform takes it
        fr_to_words(out + 8 * i, v, false);
    }
}
// the transform of size two with its scaling
void shim_omega_pair(const uint32_t *e0, const uint32_t *e1, const uint32_t *half, uint32_t *c0, uint32_t *c1, int stress) {
    Fr a, b;
    acck::omega_pair(a, b, load(e0, stress), load(e1, stress), load(half, stress));
    fr_to_words(c0, a, false); fr_to_words(c1, b, false);
}
// lists: canonical words [a (na) | r (nr)]; K chunks per holder; G lanes in the finishing step; f, s: m x 8 canonical words; ok: m bytes
void shim_pub_factors(size_t na, size_t nr, const uint32_t *lists, size_t m, const uint32_t *y_words, size_t K, size_t G, uint32_t *f_out, uint32_t *s_out, uint8_t *ok, int stress) {
    std::vector<Fr> tab(na + nr), y(m);
    for (size_t e = 0; e < na + nr; e++) tab[e] = load(lists + 8 * e, stress);
    for (size_t i = 0; i < m; i++) y[i] = load(y_words + 8 * i, stress);
    auto la = [&](size_t s, Fr &u) { u = tab[s]; };
    auto lr = [&](size_t s, Fr &u) { u = tab[na + s]; };
    std::vector<Fr> part(2 * K * m), scratch(4 * m);
    if (K > 1)
        for (size_t c = 0; c < K; c++)
            for (size_t i = 0; i < m; i++)
                acck::pub_chunk(y[i], na * c / K, na * (c + 1) / K, nr * c / K, nr * (c + 1) / K, la, lr, part[2 * (c * m + i)], part[2 * (c * m + i) + 1]);
    for (size_t g = 0; g < G && g < m; g++) {
        acck::pub_finish_share((m - g + G - 1) / G,
            [&](size_t k, Fr &PA, Fr &PD) {
                const size_t i = g + k * G;
                if (K == 1) { acck::pub_chunk(y[i], 0, na, 0, nr, la, lr, PA, PD); return; }
                fr_one(PA); PD = PA;
                for (size_t c = 0; c < K; c++) { fr_mul(PA, PA, part[2 * (c * m + i)]); fr_mul(PD, PD, part[2 * (c * m + i) + 1]); }
            },
            [&](size_t k, int q, Fr &v) { v = scratch[4 * (g + k * G) + q]; }, [&](size_t k, int q, const Fr &v) { scratch[4 * (g + k * G) + q] = v; },
            [&](size_t k, const Fr &f, const Fr &s, bool good) { fr_to_words(f_out + 8 * (g + k * G), f, false); fr_to_words(s_out + 8 * (g + k * G), s, false); ok[g + k * G] = good; });
    }
}
// rows[(i * n + j) * 8 ..] = s_i y_i^j, every row shared by ceil(n / run) lanes as in k_acc_pub_rows
void shim_pub_rows(size_t m, const uint32_t *y_words, const uint32_t *s_words, size_t n, size_t run, uint32_t *rows, int stress) {
    const size_t per_row = (n + run - 1) / run;
    for (size_t t = 0; t < m * per_row; t++) {
        const size_t i = t / per_row, j0 = (t % per_row) * run, cnt = n - j0 < run ? n - j0 : run;
        acck::pub_row_run(load(y_words + 8 * i, stress), load(s_words + 8 * i, stress), j0, cnt, [&](size_t j, const Fr &v) { fr_to_words(rows + (i * n + j) * 8, v, false); });
    }
}
}
