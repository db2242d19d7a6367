// tests/native/ps_dev_host_shim.cpp — the __host__ __device__ routines of PS (Coconut) signatures in bulk (crypto_amd/csrc/ps_kernels.hip.h: sign_scalar,
// pok_row_entry, col_scalars, g2_equal, status_of; bbs_routines.hip.h's row_value_fixed with ONE fixed column for the verification rows) compiled for the host
// with -DFP29_CHECK (every product asserts its operand contract) and driven the way k_ps_sign_rows, k_bbs_rows, k_ps_pok_rows, k_ps_col_scalars, k_ps_verdict and
// dock_ps.hip's chunks drive them.  Built and loaded by tests/test_ps_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/ps_kernels.hip.h"
using namespace fr29;

namespace {
Fr load(const uint32_t *w, int mont) { Fr x; fr_from_words(x, w, mont != 0); return x; }
}  // namespace

extern "C" {
// k_ps_sign_rows over the rows in chunks of `chunk` (dock_ps.hip sign_many): out[16 i ..] = r_i, out[16 i + 8 ..] = u_i.  sk: (1 + L) x 8 words
void shim_ps_sign_rows(const uint32_t *sk, const uint32_t *r, const uint32_t *msgs, int mont, size_t total, size_t L, size_t chunk, uint32_t *out) {
    for (size_t i0 = 0; i0 < total; i0 += chunk) {
        const size_t rows = total - i0 < chunk ? total - i0 : chunk;
        const uint32_t *cr = r + 8 * i0, *cm = msgs + 8 * L * i0;
        uint32_t *co = out + 16 * i0;
        for (size_t i = 0; i < rows; i++) {                               // one lane per row
            Fr u;
            const Fr ri = load(cr + 8 * i, mont);
            psk::sign_scalar(u, ri, L, [&](Fr &x) { x = load(sk, mont); }, [&](size_t j, Fr &x) { x = load(sk + 8 * (1 + j), mont); },
                             [&](size_t j, Fr &x) { x = load(cm + 8 * (i * L + j), mont); });
            fr_to_words(co + 16 * i, ri, false); fr_to_words(co + 16 * i + 8, u, false);
        }
    }
}
// k_bbs_rows with fixed = 1 and no multiplier: out[(i * n + k) * 8 ..] for i < rows, k < n = L + 1; s is never read
void shim_ps_verify_rows(const uint32_t *msgs, int mont, size_t rows, size_t n, uint32_t *out) {
    for (size_t lane = 0; lane < rows * n; lane++) {
        const size_t i = lane / n, k = lane % n;
        Fr v, one, o; fr_one(one);
        bbsk::row_value_fixed(v, i, k, 1, [&](size_t, Fr &) { __builtin_trap(); }, [&](size_t r, size_t j, Fr &x) { x = load(msgs + 8 * (r * (n - 1) + j), mont); });
        bbsk::row_entry(o, v, one);
        fr_to_words(out + 8 * lane, o, false);
    }
}
// k_ps_pok_rows: out: 2 rows x (L + 2) canonical words-of-8, the S rows first
void shim_ps_pok_rows(const uint32_t *resp, const uint32_t *vals, const uint8_t *rev, size_t L, int mont, size_t rows, uint32_t *out) {
    const size_t n = L + 2;
    for (size_t t = 0; t < 2 * rows * n; t++) {
        const size_t row = t / n, k = t % n;
        const int which = row >= rows ? 1 : 0;
        Fr o;
        psk::pok_row_entry(o, which, row - (which ? rows : 0), k, L, [&](size_t i, size_t j, Fr &x) { x = load(vals + 8 * (i * L + j), mont); },
                           [&](size_t i, Fr &x) { x = load(resp + 8 * i, mont); }, [&](size_t i, size_t j) { return rev[i * L + j] != 0; });
        fr_to_words(out + 8 * t, o, false);
    }
}
// k_ps_col_scalars over the rows in chunks of `chunk` (dock_ps.hip verify_batch): cols[(k * total + i) * 8 ..] for k < L + 2 (every chunk's columns are copied
// to their rows of the whole: the driver consumes them chunk by chunk)
void shim_ps_col_scalars(const uint32_t *msgs, const uint32_t *rho_words, int mont, size_t total, size_t L, size_t chunk, size_t run, uint32_t *cols) {
    const Fr rho = load(rho_words, mont);
    for (size_t i0 = 0; i0 < total; i0 += chunk) {
        const size_t rows = total - i0 < chunk ? total - i0 : chunk, nb = (rows + 256 * run - 1) / (256 * run);
        const uint32_t *cm = msgs + 8 * L * i0;
        std::vector<uint32_t> cc((L + 2) * chunk * 8, 0xA5A5A5A5u);
        for (size_t k = 0; k < L + 2; k++)
            for (size_t b = 0; b < nb; b++)
                for (unsigned t = 0; t < 256; t++) {
                    const size_t lo = (b * 256 + t) * run;
                    if (lo >= rows) continue;
                    const size_t cnt = rows - lo < run ? rows - lo : run;
                    psk::col_scalars(rho, i0 + lo, cnt, k, L, [&](size_t j, Fr &v) { v = load(cm + 8 * ((lo + j) * L + (k - 1)), mont); },
                                     [&](size_t j, const Fr &o) { fr_to_words(cc.data() + 8 * (k * chunk + lo + j), o, false); });
                }
        for (size_t k = 0; k < L + 2; k++) memcpy(cols + 8 * (k * total + i0), cc.data() + 8 * k * chunk, rows * 32);
    }
}
// the word routines of k_ps_verdict
int shim_ps_g2_equal(const uint32_t *a, int a_inf, const uint32_t *b, int b_inf) {
    auto words = [](const uint32_t *p) { return [p](int q, uint32_t w[4]) { memcpy(w, p + 4 * q, 16); }; };
    return psk::g2_equal(words(a), a_inf != 0, words(b), b_inf != 0) ? 1 : 0;
}
int shim_ps_status(int schnorr_ok, int s1_inf, int s2_inf, int pairing_ok) { return psk::status_of(schnorr_ok != 0, s1_inf != 0, s2_inf != 0, pairing_ok != 0); }
}
