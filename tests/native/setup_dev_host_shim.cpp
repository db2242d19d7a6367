// tests/native/setup_dev_host_shim.cpp — the key generator's __host__ __device__ Fr routines (crypto_amd/csrc/fr29.hip.h: fr_inv, fr_batch_inv,
// fr_fold_chunk) compiled for the host with -DFP29_CHECK (every product asserts its operand contract), driven the way setup_kernels.hip.h drives
// them: the batch inversion over strided lane shares, the segmented sum pass after pass until one chunk is left (setupk::launch_col_sum).
// Built and loaded by tests/test_setup_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/fr29.hip.h"
using namespace fr29;

static Fr load(const uint32_t *w, int stress) {
    Fr x; fr_from_words(x, w, false);                   // a product: < 2 r
    if (stress) {                                       // the same element pushed towards the top of its bound: + r, normalised
        constexpr uint32_t P_[NL] = FR29_R; Fr p; fr_const(p, P_);
        fr_add(x, x, p); fr_norm(x, x);
    }
    return x;
}
static void store(uint32_t *w, const Fr &x) { fr_to_words(w, x, false); }

extern "C" {
void shim_fr_inv(const uint32_t *in, uint32_t *out, int stress) { Fr x = load(in, stress), r; fr_inv(r, x); store(out, r); }
// n elements, G lanes: lane g inverts the elements g, g + G, ... with one fr_inv (k_lagrange's split)
void shim_batch_inv(size_t n, size_t G, const uint32_t *in, uint32_t *out, int stress) {
    std::vector<Fr> x(n), o(n);
    for (size_t i = 0; i < n; i++) x[i] = load(in + 8 * i, stress);
    for (size_t g = 0; g < G && g < n; g++) {
        const size_t m = (n - g + G - 1) / G;
        fr_batch_inv(m, [&](size_t k, Fr &v) { v = x[g + k * G]; }, [&](size_t k, Fr &v) { v = o[g + k * G]; }, [&](size_t k, const Fr &v) { o[g + k * G] = v; });
    }
    for (size_t i = 0; i < n; i++) store(out + 8 * i, o[i]);
}
// out[key] += sum of the values of that key, over a key-sorted list of n entries (nv keys), in passes of chunks of ch entries; returns the number of passes
// (-1: a key was completed twice)
int shim_fold(size_t n, const uint32_t *keys_in, const uint32_t *vals_in, size_t ch, size_t nv, uint32_t *out_words, int stress) {
    std::vector<uint32_t> keys(keys_in, keys_in + n);
    std::vector<Fr> vals(n), out(nv);
    std::vector<int> hits(nv, 0);
    for (size_t i = 0; i < n; i++) vals[i] = load(vals_in + 8 * i, stress);
    for (size_t j = 0; j < nv; j++) fr_zero(out[j]);
    int passes = 0;
    while (n) {
        const size_t nch = (n + ch - 1) / ch;
        const bool fin = nch == 1;
        std::vector<uint32_t> pk(2 * nch); std::vector<Fr> pv(2 * nch);
        for (size_t c = 0; c < nch; c++) {
            const size_t lo = c * ch, hi = lo + ch < n ? lo + ch : n;
            fr_fold_chunk(keys.data(), lo, hi, fin, [&](size_t k, Fr &v) { v = vals[k]; },
                          [&](uint32_t key, const Fr &s) { fr_add(out[key], out[key], s); fr_norm(out[key], out[key]); hits[key]++; },
                          [&](int which, uint32_t key, const Fr &s) { pk[2 * c + which] = key; pv[2 * c + which] = s; });
        }
        passes++;
        if (fin) break;
        keys.swap(pk); vals.swap(pv); n = 2 * nch;
    }
    for (size_t j = 0; j < nv; j++) { if (hits[j] > 1) return -1; store(out_words + 8 * j, out[j]); }
    return passes;
}
}
