// tests/native/acc_pok_dev_host_shim.cpp — the __host__ __device__ routines of accumulator proofs in bulk (crypto_amd/csrc/acc_pok_kernels.hip.h: own_scalar,
// col_run, col_term, row_weights, with col_sums.hip.h's tree_step, col_finish and neg_product; and the word routines fq_neg_words, stage_src, mem_status,
// nm_status) compiled for the host with -DFP29_CHECK (every product asserts its operand contract), driven the way k_acc_pok_own, k_acc_pok_stage,
// k_acc_pok_col_sums / k_col_finish and dock_acc_pok.hip's chunks drive them (col_frame_host.hpp).  Built and loaded by tests/test_acc_pok_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/acc_pok_kernels.hip.h"
#include "col_frame_host.hpp"
using namespace fr29;

namespace {
struct In {
    const uint32_t *chal, *resp; int kind, mont;
    Fr load(const uint32_t *w) const { Fr x; fr_from_words(x, w, mont != 0); return x; }
    size_t nresp() const { return (size_t)accpk::shape_of(kind).resp; }
};
}  // namespace
#define FUNCTORS(in) [&](size_t r, Fr &x) { x = in.load(in.chal + 8 * r); }, [&](size_t r, unsigned q, Fr &x) { x = in.load(in.resp + 8 * (in.nresp() * r + q)); }

extern "C" {
// k_acc_pok_own: own[(i * n_own + t) * 8 ..], one lane per scalar
void shim_acc_pok_own(const uint32_t *chal, const uint32_t *resp, int kind, int mont, size_t rows, uint32_t *own) {
    const In in{chal, resp, kind, mont};
    const size_t n_own = (size_t)accpk::shape_of(kind).own;
    for (size_t lane = 0; lane < rows * n_own; lane++) {
        Fr o;
        accpk::own_scalar(o, kind, lane / n_own, (unsigned)(lane % n_own), FUNCTORS(in));
        fr_to_words(own + 8 * lane, o, false);
    }
}
// k_acc_pok_stage on the host: the same slots, sources, flags and flip.  points: rows x pts x 24 words, shared: 3 x 24 words; own: rows x n_own x 24,
// pa / pb: rows x 24, skip: 3 rows
void shim_acc_pok_stage(const uint32_t *points, const uint32_t *shared, int kind, size_t rows, uint32_t *own, uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    const accpk::Shape sh = accpk::shape_of(kind);
    const unsigned n_own = (unsigned)sh.own, n_slots = n_own + 2;
    for (size_t t = 0; t < rows * n_slots; t++) {
        const size_t i = t / n_slots;
        const unsigned slot = (unsigned)(t % n_slots), src = accpk::stage_src(kind, slot);
        uint32_t w[24];
        memcpy(w, src >= 8 ? shared + 24 * (src - 8) : points + (i * sh.pts + src) * 24, 96);
        uint32_t *dst = slot < n_own ? own + (i * n_own + slot) * 24 : (slot == n_own ? pa : pb) + i * 24;
        if (slot >= n_own) skip[(slot - n_own) * rows + i] = accpk::fq_zero_words(w, 24) ? 1 : 0;
        if (slot == 1) skip[2 * rows + i] = (kind != accpk::MEMBERSHIP && accpk::fq_zero_words(w, 24)) ? 1 : 0;
        if (slot == n_own + 1) { uint32_t y[12]; accpk::fq_neg_words(y, w + 12); memcpy(w + 12, y, 48); }
        memcpy(dst, w, 96);
    }
}
// k_acc_pok_col_sums + k_col_finish over the rows in chunks of `chunk` (dock_acc_pok.hip verify_batch).  c: shared x 8 canonical words after the last chunk;
// wts: total x pts x 8; tp, tn: total x 8
void shim_acc_pok_columns(const uint32_t *chal, const uint32_t *resp, const uint32_t *rho_words, int kind, int mont, size_t total, size_t chunk, size_t run, uint32_t *c,
                          uint32_t *wts, uint32_t *tp, uint32_t *tn) {
    const accpk::Shape shp = accpk::shape_of(kind);
    const size_t n = (size_t)shp.shared, np = (size_t)shp.pts, nr = (size_t)shp.resp;
    Fr rho; fr_from_words(rho, rho_words, mont != 0);
    // the P of a non-membership proof (column 1) leaves negated
    col_frame_walk(total, chunk, 1, run, n, kind == accpk::MEMBERSHIP ? 0 : 1, kind == accpk::MEMBERSHIP ? 0 : 2, [&](size_t i0, size_t, size_t k, size_t lo, size_t cnt, Fr &sum) {
        // the chunk's arrays start at its first row, as the driver uploads them
        const In in{chal + 8 * i0, resp + 8 * nr * i0, kind, mont};
        uint32_t *cw = wts + 8 * np * i0, *ctp = tp + 8 * i0, *ctn = tn + 8 * i0;
        accpk::col_run(kind, rho, i0 + lo, cnt, k == 0,
                       [&](size_t j, const Fr &u, const Fr &v, Fr &s) {
                           accpk::col_term(s, kind, lo + j, k, u, v, [&](size_t r, unsigned q, Fr &x) { x = in.load(in.resp + 8 * (nr * r + q)); });
                       },
                       [&](size_t j, const Fr &u, const Fr &v, const Fr &tw) {
                           const size_t i = lo + j;
                           accpk::row_weights(kind, i, u, v, tw, FUNCTORS(in), [&](unsigned q, const Fr &x) {
                               if (q < (unsigned)np) fr_to_words(cw + 8 * (i * np + q), x, false);
                               else fr_to_words((q == (unsigned)np ? ctp : ctn) + 8 * i, x, false);
                           });
                       },
                       sum);
    }, c);
}
// the word routines of k_acc_pok_stage and k_acc_pok_verdict
void shim_acc_fq_neg(const uint32_t *y, uint32_t *out) { accpk::fq_neg_words(out, y); }
int shim_mem_status(int a_inf, int schnorr_ok, int pairing_ok) { return accpk::mem_status(a_inf != 0, schnorr_ok != 0, pairing_ok != 0); }
int shim_nm_status(int c_inf, int j_inf, int short_ok, int long_ok, int pairing_ok) {
    return accpk::nm_status(c_inf != 0, j_inf != 0, short_ok != 0, long_ok != 0, pairing_ok != 0);
}
}
