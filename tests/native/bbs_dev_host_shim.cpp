// tests/native/bbs_dev_host_shim.cpp — the __host__ __device__ Fr routines of BBS+ in bulk (crypto_amd/csrc/bbs_kernels.hip.h: row_value, row_entry; col_sums.hip.h:
// pow_start, col_run, tree_step, col_finish, neg_product) compiled for the host with -DFP29_CHECK (every product asserts its operand contract), driven the way
// k_bbs_rows, k_bbs_col_sums / k_col_finish and dock_bbs.hip's chunks drive them (col_frame_host.hpp); and the host's inverses 1 / (x + e_i) with their zero flags
// (crypto_amd/csrc/acc_host_tables.hpp issue_inverses), share by share.  Built and loaded by tests/test_bbs_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/bbs_kernels.hip.h"
#include "col_frame_host.hpp"
#include "../../crypto_amd/csrc/acc_host_tables.hpp"
using namespace fr29;

static Fr load(const uint32_t *w, int mont) { Fr x; fr_from_words(x, w, mont != 0); return x; }

extern "C" {
// k_bbs_rows: out[(i * n + k) * 8 ..] for i < rows, k < n = L + 2.  s: rows x 8 words, msgs: rows x L x 8 words, t (ark-ff Montgomery words) or NULL
void shim_rows(const uint32_t *s, const uint32_t *msgs, const uint32_t *t, int mont, size_t rows, size_t n, uint32_t *out) {
    for (size_t lane = 0; lane < rows * n; lane++) {
        const size_t i = lane / n, k = lane % n;
        Fr v, mult, o;
        bbsk::row_value(v, i, k, [&](size_t r, Fr &x) { x = load(s + 8 * r, mont); }, [&](size_t r, size_t j, Fr &x) { x = load(msgs + 8 * (r * (n - 2) + j), mont); });
        if (t) mult = load(t + 8 * i, 1); else fr_one(mult);
        bbsk::row_entry(o, v, mult);
        fr_to_words(out + 8 * lane, o, false);
    }
}
// k_bbs_col_sums + k_col_finish over the rows in chunks of `chunk` (dock_bbs.hip verify_batch).  c: n x 8 canonical words of -c_k after the last chunk; wts, we: total x 8 words
void shim_columns(const uint32_t *e, const uint32_t *s, const uint32_t *msgs, const uint32_t *rho_words, int mont, size_t total, size_t n, size_t chunk, size_t run,
                  uint32_t *c, uint32_t *wts, uint32_t *we) {
    const Fr rho = load(rho_words, mont);
    col_frame_walk(total, chunk, 1, run, n, 0, n, [&](size_t i0, size_t, size_t k, size_t lo, size_t cnt, Fr &sum) {
        colk::col_run(rho, i0 + lo, cnt,
                      [&](size_t j, Fr &v) {
                          bbsk::row_value(v, i0 + lo + j, k, [&](size_t r, Fr &x) { x = load(s + 8 * r, mont); },
                                          [&](size_t r, size_t q, Fr &x) { x = load(msgs + 8 * (r * (n - 2) + q), mont); });
                      },
                      [&](size_t j, const Fr &w) {
                          if (k != 0) return;
                          Fr p; const Fr ei = load(e + 8 * (i0 + lo + j), mont);
                          fr_mul(p, ei, w);
                          fr_to_words(wts + 8 * (i0 + lo + j), w, false); fr_to_words(we + 8 * (i0 + lo + j), p, false);
                      },
                      sum);
    }, c);
}
// t_i = 1 / (x + e_i) as ark-ff Montgomery words (4 x u64 each) and zero[i] = (x + e_i == 0), in `shares` shares as the host threads cut them
int shim_inverses(const uint64_t *es, size_t m, const uint64_t *x, int mont, size_t shares, uint64_t *t, uint8_t *zero) {
    int rc = 0;
    for (size_t k = 0; k < shares; k++) {
        const int e = acch::issue_inverses(es, m * k / shares, m * (k + 1) / shares, x, mont != 0, t, zero);
        if (e && !rc) rc = e;
    }
    return rc;
}
}
