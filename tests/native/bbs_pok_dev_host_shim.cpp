// tests/native/bbs_pok_dev_host_shim.cpp — the __host__ __device__ routines of BBS+ proofs of knowledge in bulk (crypto_amd/csrc/bbs_pok_kernels.hip.h:
// pok_value, pok_row_entry, pok_own_scalar, pok_col_run, pok_col_term, pok_weights, with col_sums.hip.h's tree_step, col_finish and neg_product; and the
// base-field word routines fq_neg_words, g1_is_negation, pok_status) compiled for the host with -DFP29_CHECK (every product asserts its operand contract), driven
// the way k_bbs_pok_rows, k_bbs_pok_own, k_bbs_pok_col_sums / k_col_finish and dock_bbs.hip's chunks drive them (col_frame_host.hpp).  Built and loaded by
// tests/test_bbs_pok_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/bbs_pok_kernels.hip.h"
#include "col_frame_host.hpp"
using namespace fr29;

namespace {
struct In {
    const uint32_t *chal, *fixed, *vals; const uint8_t *rev; size_t L; int mont;
    Fr load(const uint32_t *w) const { Fr x; fr_from_words(x, w, mont != 0); return x; }
};
}  // namespace
#define FUNCTORS(in) [&](size_t r, Fr &x) { x = in.load(in.chal + 8 * r); }, [&](size_t r, unsigned t, Fr &x) { x = in.load(in.fixed + 8 * (4 * r + t)); }, \
                     [&](size_t r, size_t j, Fr &x) { x = in.load(in.vals + 8 * (r * in.L + j)); }, [&](size_t r, size_t j) { return in.rev[r * in.L + j] != 0; }

extern "C" {
// k_bbs_pok_rows and k_bbs_pok_own: out_rows[(i * (L + 2) + k) * 8 ..], own[(i * 7 + t) * 8 ..]
void shim_pok_rows(const uint32_t *chal, const uint32_t *fixed, const uint32_t *vals, const uint8_t *rev, int mont, size_t rows, size_t L, uint32_t *out_rows, uint32_t *own) {
    const In in{chal, fixed, vals, rev, L, mont};
    const size_t n = L + 2;
    for (size_t lane = 0; lane < rows * n; lane++) {
        Fr o;
        bbspk::pok_row_entry(o, lane / n, lane % n, FUNCTORS(in));
        fr_to_words(out_rows + 8 * lane, o, false);
    }
    for (size_t lane = 0; lane < rows * bbspk::POK_OWN; lane++) {
        Fr o;
        bbspk::pok_own_scalar(o, lane / bbspk::POK_OWN, (unsigned)(lane % bbspk::POK_OWN), [&](size_t r, Fr &x) { x = in.load(chal + 8 * r); },
                              [&](size_t r, unsigned t, Fr &x) { x = in.load(fixed + 8 * (4 * r + t)); });
        fr_to_words(own + 8 * lane, o, false);
    }
}
// k_bbs_pok_col_sums + k_col_finish over the rows in chunks of `chunk` (dock_bbs.hip pok_verify_batch).  c: (L + 2) x 8 canonical words of C_k after the last
// chunk; w5: total x 5 x 8; tp, tn: total x 8
void shim_pok_columns(const uint32_t *chal, const uint32_t *fixed, const uint32_t *vals, const uint8_t *rev, const uint32_t *rho_words, int mont, size_t total, size_t L,
                      size_t chunk, size_t run, uint32_t *c, uint32_t *w5, uint32_t *tp, uint32_t *tn) {
    const size_t n = L + 2;
    Fr rho; fr_from_words(rho, rho_words, mont != 0);
    col_frame_walk(total, chunk, 1, run, n, 0, 0, [&](size_t i0, size_t, size_t k, size_t lo, size_t cnt, Fr &sum) {
        // the chunk's arrays start at its first row, as the driver uploads them
        const In in{chal + 8 * i0, fixed + 32 * i0, vals + 8 * i0 * L, rev + i0 * L, L, mont};
        uint32_t *cw5 = w5 + 40 * i0, *ctp = tp + 8 * i0, *ctn = tn + 8 * i0;
        bbspk::pok_col_run(rho, i0 + lo, cnt, k == 0,
                           [&](size_t j, const Fr &u, const Fr &v, Fr &s) { bbspk::pok_col_term(s, lo + j, k, u, v, FUNCTORS(in)); },
                           [&](size_t j, const Fr &u, const Fr &v, const Fr &tw) {
                               const size_t i = lo + j;
                               bbspk::pok_weights(i, u, v, tw, [&](size_t r, Fr &x) { x = in.load(in.chal + 8 * r); },
                                                  [&](size_t r, unsigned q, Fr &x) { x = in.load(in.fixed + 8 * (4 * r + q)); },
                                                  [&](unsigned q, const Fr &x) {
                                                      if (q < (unsigned)bbspk::POK_PTS) fr_to_words(cw5 + 8 * (i * bbspk::POK_PTS + q), x, false);
                                                      else fr_to_words((q == 5 ? ctp : ctn) + 8 * i, x, false);
                                                  });
                           },
                           sum);
    }, c);
}
// the base-field word routines of k_bbs_pok_stage and k_bbs_pok_verdict
void shim_fq_neg(const uint32_t *y, uint32_t *out) { bbspk::fq_neg_words(out, y); }
int shim_is_negation(const uint32_t *a, int a_inf, const uint32_t *b, int b_inf) { return bbspk::g1_is_negation(a, a_inf != 0, b, b_inf != 0) ? 1 : 0; }
int shim_status(int a_inf, int first_ok, int second_ok, int pairing_ok) { return bbspk::pok_status(a_inf != 0, first_ok != 0, second_ok != 0, pairing_ok != 0); }
}
