// tests/native/bbs23_dev_host_shim.cpp — the __host__ __device__ routines of BBS (2023) in bulk compiled for the host with -DFP29_CHECK (every product asserts
// its operand contract): bbs_routines.hip.h's row_value_fixed with ONE fixed column, driven the way k_bbs_rows and k_bbs_col_sums / k_col_finish drive it for
// the signature calls, and crypto_amd/csrc/bbs23_kernels.hip.h (row_entry, own_scalar, col_run, col_term, row_weights, stage_src, fq_neg_words, g1_is_negation,
// status_of), driven the way k_bbs23_rows, k_bbs23_own, k_bbs23_stage, k_bbs23_verdict, k_bbs23_col_sums / k_col_finish and dock_bbs.hip's chunks drive
// them (col_frame_host.hpp).  Built and loaded by tests/test_bbs23_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/bbs23_kernels.hip.h"
#include "col_frame_host.hpp"
using namespace fr29;

namespace {
Fr load(const uint32_t *w, int mont) { Fr x; fr_from_words(x, w, mont != 0); return x; }
struct In {
    const uint32_t *chal, *resp, *vals; const uint8_t *rev; size_t L; int kind, mont;
    size_t nresp() const { return (size_t)bbs23k::shape_of(kind).resp; }
};
}  // namespace
#define CHAL(in) [&](size_t r, Fr &x) { x = load(in.chal + 8 * r, in.mont); }
#define RESP(in) [&](size_t r, unsigned q, Fr &x) { x = load(in.resp + 8 * (in.nresp() * r + q), in.mont); }
#define VALS(in) [&](size_t r, size_t j, Fr &x) { x = load(in.vals + 8 * (r * in.L + j), in.mont); }, [&](size_t r, size_t j) { return in.rev[r * in.L + j] != 0; }

extern "C" {
// k_bbs_rows with fixed = 1: out[(i * n + k) * 8 ..] for i < rows, k < n = L + 1.  msgs: rows x L x 8 words, t (ark-ff Montgomery words) or NULL; s is never read
void shim_bbs23_sig_rows(const uint32_t *msgs, const uint32_t *t, int mont, size_t rows, size_t n, uint32_t *out) {
    for (size_t lane = 0; lane < rows * n; lane++) {
        const size_t i = lane / n, k = lane % n;
        Fr v, mult, o;
        bbsk::row_value_fixed(v, i, k, 1, [&](size_t, Fr &) { __builtin_trap(); }, [&](size_t r, size_t j, Fr &x) { x = load(msgs + 8 * (r * (n - 1) + j), mont); });
        if (t) mult = load(t + 8 * i, 1); else fr_one(mult);
        bbsk::row_entry(o, v, mult);
        fr_to_words(out + 8 * lane, o, false);
    }
}
// k_bbs_col_sums + k_col_finish with fixed = 1 over the rows in chunks of `chunk` (dock_bbs.hip verify_batch): c: n x 8 canonical words of -c_k after the last
// chunk; wts, we: total x 8
void shim_bbs23_sig_columns(const uint32_t *e, const uint32_t *msgs, const uint32_t *rho_words, int mont, size_t total, size_t n, size_t chunk, size_t run, uint32_t *c,
                            uint32_t *wts, uint32_t *we) {
    const Fr rho = load(rho_words, mont);
    col_frame_walk(total, chunk, 1, run, n, 0, n, [&](size_t i0, size_t, size_t k, size_t lo, size_t cnt, Fr &sum) {
        const uint32_t *ce = e + 8 * i0, *cm = msgs + 8 * (n - 1) * i0;
        colk::col_run(rho, i0 + lo, cnt,
                      [&](size_t j, Fr &v) {
                          bbsk::row_value_fixed(v, lo + j, k, 1, [&](size_t, Fr &) { __builtin_trap(); },
                                                [&](size_t r, size_t q, Fr &x) { x = load(cm + 8 * (r * (n - 1) + q), mont); });
                      },
                      [&](size_t j, const Fr &w) {
                          if (k != 0) return;
                          Fr p; fr_mul(p, load(ce + 8 * (lo + j), mont), w);
                          fr_to_words(wts + 8 * (i0 + lo + j), w, false); fr_to_words(we + 8 * (i0 + lo + j), p, false);
                      },
                      sum);
    }, c);
}
// k_bbs23_rows and k_bbs23_own: rows x (L + 1) and rows x own canonical words-of-8
void shim_bbs23_rows(const uint32_t *chal, const uint32_t *resp, const uint32_t *vals, const uint8_t *rev, size_t L, int kind, int mont, size_t rows, uint32_t *out_rows,
                     uint32_t *own) {
    const In in{chal, resp, vals, rev, L, kind, mont};
    const size_t n = L + 1, n_own = (size_t)bbs23k::shape_of(kind).own;
    for (size_t lane = 0; lane < rows * n; lane++) {
        Fr o;
        bbs23k::row_entry(o, lane / n, lane % n, CHAL(in), VALS(in));
        fr_to_words(out_rows + 8 * lane, o, false);
    }
    for (size_t lane = 0; lane < rows * n_own; lane++) {
        Fr o;
        bbs23k::own_scalar(o, kind, lane / n_own, (unsigned)(lane % n_own), CHAL(in), RESP(in));
        fr_to_words(own + 8 * lane, o, false);
    }
}
// k_bbs23_stage on the host: the same slots, sources, flags and flip.  points: rows x pts x 24 words; own: rows x n_own x 24, pa / pb: rows x 24, skip: 2 rows
void shim_bbs23_stage(const uint32_t *points, int kind, size_t rows, uint32_t *own, uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    const bbs23k::Shape sh = bbs23k::shape_of(kind);
    const unsigned n_own = (unsigned)sh.own, n_slots = n_own + 2;
    for (size_t t = 0; t < rows * n_slots; t++) {
        const size_t i = t / n_slots;
        const unsigned slot = (unsigned)(t % n_slots), src = bbs23k::stage_src(kind, slot);
        uint32_t w[24];
        memcpy(w, points + (i * sh.pts + src) * 24, 96);
        uint32_t *dst = slot < n_own ? own + (i * n_own + slot) * 24 : (slot == n_own ? pa : pb) + i * 24;
        if (slot >= n_own) skip[(slot - n_own) * rows + i] = bbs23k::fq_zero_words(w, 24) ? 1 : 0;
        if (slot == n_own + 1) { uint32_t y[12]; bbs23k::fq_neg_words(y, w + 12); memcpy(w + 12, y, 48); }
        memcpy(dst, w, 96);
    }
}
// k_bbs23_col_sums + k_col_finish over the rows in chunks of `chunk` (dock_bbs.hip pok23_verify_batch).  c: (L + 1) x 8 canonical words after the last
// chunk; wts: total x pts x 8; tp, tn: total x 8
void shim_bbs23_columns(const uint32_t *chal, const uint32_t *resp, const uint32_t *vals, const uint8_t *rev, size_t L, const uint32_t *rho_words, int kind, int mont, size_t total,
                        size_t chunk, size_t run, uint32_t *c, uint32_t *wts, uint32_t *tp, uint32_t *tn) {
    const bbs23k::Shape shp = bbs23k::shape_of(kind);
    const size_t n = L + 1, np = (size_t)shp.pts, nr = (size_t)shp.resp;
    const Fr rho = load(rho_words, mont);
    col_frame_walk(total, chunk, 1, run, n, 0, 0, [&](size_t i0, size_t, size_t k, size_t lo, size_t cnt, Fr &sum) {
        // the chunk's arrays start at its first row, as the driver uploads them
        const In in{chal + 8 * i0, resp + 8 * nr * i0, vals + 8 * L * i0, rev + L * i0, L, kind, mont};
        uint32_t *cw = wts + 8 * np * i0, *ctp = tp + 8 * i0, *ctn = tn + 8 * i0;
        bbs23k::col_run(kind, rho, i0 + lo, cnt, k == 0,
                        [&](size_t j, const Fr &u, const Fr &v, Fr &s) { bbs23k::col_term(s, lo + j, k, kind == bbs23k::CDL ? v : u, CHAL(in), VALS(in)); },
                        [&](size_t j, const Fr &u, const Fr &v, const Fr &tw) {
                            const size_t i = lo + j;
                            bbs23k::row_weights(kind, i, u, v, tw, CHAL(in), RESP(in), [&](unsigned q, const Fr &x) {
                                if (q < (unsigned)np) fr_to_words(cw + 8 * (i * np + q), x, false);
                                else fr_to_words((q == (unsigned)np ? ctp : ctn) + 8 * i, x, false);
                            });
                        },
                        sum);
    }, c);
}
// the word routines of k_bbs23_stage and k_bbs23_verdict
void shim_bbs23_fq_neg(const uint32_t *y, uint32_t *out) { bbs23k::fq_neg_words(out, y); }
int shim_bbs23_is_negation(const uint32_t *a, int a_inf, const uint32_t *b, int b_inf) { return bbs23k::g1_is_negation(a, a_inf != 0, b, b_inf != 0) ? 1 : 0; }
int shim_bbs23_status(int a_inf, int first_ok, int second_ok, int pairing_ok) { return bbs23k::status_of(a_inf != 0, first_ok != 0, second_ok != 0, pairing_ok != 0); }
}
