// tests/native/acc_gt_dev_host_shim.cpp — the __host__ __device__ routines of the accumulator proofs with a GT commitment in bulk
// (crypto_amd/csrc/acc_gt_kernels.hip.h: own_scalar, col_run, col_term, row_weights, with col_sums.hip.h's tree_step, col_finish and neg_product; and the word
// routines seg_end, stage_src, first_failure) compiled for the host with -DFP29_CHECK (every product asserts its operand contract), driven the way k_acc_gt_own,
// k_acc_gt_stage, k_acc_gt_sides, k_acc_gt_verdict, k_acc_gt_col_sums / k_col_finish and dock_acc_gt.hip's chunks drive them (col_frame_host.hpp).  Built and
// loaded by tests/test_acc_gt_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/acc_gt_kernels.hip.h"
#include "col_frame_host.hpp"
using namespace fr29;

namespace {
struct In {
    const uint32_t *chal, *resp; int kind, mont;
    Fr load(const uint32_t *w) const { Fr x; fr_from_words(x, w, mont != 0); return x; }
    size_t nresp() const { return (size_t)accgt::shape_of(kind).resp; }
};
}  // namespace
#define FUNCTORS(in) [&](size_t r, Fr &x) { x = in.load(in.chal + 8 * r); }, [&](size_t r, unsigned q, Fr &x) { x = in.load(in.resp + 8 * (in.nresp() * r + q)); }

extern "C" {
// the shape of a kind: pts, resp, own, segs, checks, g1cols, pcols, then the segs segment ends
void shim_acc_gt_shape(int kind, int out[16]) {
    const accgt::Shape s = accgt::shape_of(kind);
    const int v[7] = {s.pts, s.resp, s.own, s.segs, s.checks, s.g1cols, s.pcols};
    for (int k = 0; k < 7; k++) out[k] = v[k];
    for (int g = 0; g < s.segs; g++) out[7 + g] = (int)accgt::seg_end(kind, (unsigned)g);
}
// k_acc_gt_own: own[(i * n_own + t) * 8 ..], one lane per scalar
void shim_acc_gt_own(const uint32_t *chal, const uint32_t *resp, int kind, int mont, size_t rows, uint32_t *own) {
    const In in{chal, resp, kind, mont};
    const size_t n_own = (size_t)accgt::shape_of(kind).own;
    for (size_t lane = 0; lane < rows * n_own; lane++) {
        Fr o;
        accgt::own_scalar(o, kind, lane / n_own, (unsigned)(lane % n_own), FUNCTORS(in));
        fr_to_words(own + 8 * lane, o, false);
    }
}
// k_acc_gt_stage on the host: the same lanes and sources.  points: rows x pts x 24 words, shared: 6 x 24 words (V, X, Y, Z, K, P); bases: rows x n_own x 24
void shim_acc_gt_stage(const uint32_t *points, const uint32_t *shared, int kind, size_t rows, uint32_t *bases) {
    const accgt::Shape sh = accgt::shape_of(kind);
    const unsigned n_own = (unsigned)sh.own;
    for (size_t t = 0; t < rows * n_own; t++) {
        const size_t i = t / n_own;
        const unsigned src = accgt::stage_src(kind, (unsigned)(t % n_own));
        memcpy(bases + t * 24, src >= 16 ? shared + 24 * (src - 16) : points + (i * sh.pts + src) * 24, 96);
    }
}
// k_acc_gt_sides on the host: sums: rows x segs x 36 words, inf: rows x segs; pa / pb: rows x 24, skip: 2 rows
void shim_acc_gt_sides(const uint32_t *sums, const uint8_t *inf, int kind, size_t rows, uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    const unsigned segs = (unsigned)accgt::shape_of(kind).segs;
    for (size_t t = 0; t < 2 * rows; t++) {
        const size_t i = t >> 1;
        const unsigned side = (unsigned)(t & 1);
        const size_t j = i * segs + segs - 1 - side;
        const bool z = inf[j] != 0;
        uint32_t *o = (side ? pb : pa) + i * 24;
        if (z) memset(o, 0, 96); else memcpy(o, sums + j * 36, 96);
        skip[side * rows + i] = z ? 1 : 0;
    }
}
// k_acc_gt_verdict on the host: seg_inf: rows x segs, gt / r_e: rows x 144 words
void shim_acc_gt_verdict(const uint8_t *seg_inf, const uint32_t *gt, const uint32_t *r_e, int kind, size_t rows, uint8_t *status) {
    const unsigned segs = (unsigned)accgt::shape_of(kind).segs;
    for (size_t i = 0; i < rows; i++) {
        const bool eq = memcmp(gt + i * accgt::GTW, r_e + i * accgt::GTW, accgt::GTW * 4) == 0;
        status[i] = accgt::first_failure(kind, [&](int j) { return seg_inf[i * segs + j] != 0; }, eq);
    }
}
// k_acc_gt_col_sums + k_col_finish over the rows in chunks of `chunk` (dock_acc_gt.hip verify_batch).  c: columns x 8 canonical words after the last chunk;
// wts: total x pts x 8; wp, wq, tp: total x 8
void shim_acc_gt_columns(const uint32_t *chal, const uint32_t *resp, const uint32_t *rho_words, int kind, int mont, size_t total, size_t chunk, size_t run, uint32_t *c,
                         uint32_t *wts, uint32_t *wp, uint32_t *wq, uint32_t *tp) {
    const accgt::Shape shp = accgt::shape_of(kind);
    const size_t n = (size_t)accgt::cols_of(kind), np = (size_t)shp.pts, nr = (size_t)shp.resp;
    Fr rho; fr_from_words(rho, rho_words, mont != 0);
    // the columns of the two sides leave negated
    col_frame_walk(total, chunk, 1, run, n, (size_t)shp.g1cols, n, [&](size_t i0, size_t, size_t k, size_t lo, size_t cnt, Fr &sum) {
        // the chunk's arrays start at its first row, as the driver uploads them
        const In in{chal + 8 * i0, resp + 8 * nr * i0, kind, mont};
        uint32_t *cw = wts + 8 * np * i0, *cwp = wp + 8 * i0, *cwq = wq + 8 * i0, *ctp = tp + 8 * i0;
        accgt::col_run(kind, rho, i0 + lo, cnt, k == 0,
                       [&](size_t j, const accgt::RowWeights &W, Fr &s) { accgt::col_term(s, kind, lo + j, k, W, FUNCTORS(in)); },
                       [&](size_t j, const accgt::RowWeights &W) {
                           const size_t i = lo + j;
                           accgt::row_weights(kind, i, W, FUNCTORS(in), [&](unsigned q, const Fr &x) {
                               if (q < (unsigned)np) fr_to_words(cw + 8 * (i * np + q), x, false);
                               else fr_to_words((q == (unsigned)np ? cwp : q == (unsigned)np + 1 ? cwq : ctp) + 8 * i, x, false);
                           });
                       },
                       sum);
    }, c);
}
}
