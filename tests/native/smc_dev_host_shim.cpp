// tests/native/smc_dev_host_shim.cpp — the __host__ __device__ routines of range proofs over weak-BB signatures in bulk (crypto_amd/csrc/smc_kernels.hip.h:
// own_scalars, col_run, merge_weight, with col_sums.hip.h's tree_step, col_finish and neg_product; and the word routines fq_neg_words, stage_src,
// proof_verdict, ref_position) compiled for the host with -DFP29_CHECK (every product asserts its operand contract), driven the way k_smc_own, k_smc_stage,
// k_smc_merge_weights, k_smc_verdict, k_smc_col_sums / k_col_finish and dock_smc.hip's chunks drive them (col_frame_host.hpp).  Built and loaded by
// tests/test_smc_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/smc_kernels.hip.h"
#include "col_frame_host.hpp"
using namespace fr29;

namespace {
struct In {
    const uint32_t *chal, *zr, *z, *stmt; int sides, l, mont;
    Fr load(const uint32_t *w) const { Fr x; fr_from_words(x, w, mont != 0); return x; }
    size_t D() const { return smck::digit_count(sides, l); }
};
}  // namespace

extern "C" {
// k_smc_own: own[(e * 4 + t) * 8 ..], one lane per equation
void shim_smc_own(const uint32_t *chal, const uint32_t *zr, const uint32_t *z, const uint32_t *stmt, int sides, int l, int mont, size_t rows, uint32_t *own) {
    const In in{chal, zr, z, stmt, sides, l, mont};
    const size_t M = smck::eq_count(sides, l);
    for (size_t e = 0; e < rows * M; e++) {
        Fr o[smck::EQ_TERMS];
        smck::own_scalars(o, sides, l, e / M, (unsigned)(e % M), [&](size_t r, Fr &x) { x = in.load(in.chal + 8 * r); },
                          [&](size_t r, unsigned s, Fr &x) { x = in.load(in.zr + 8 * (r * (size_t)sides + s)); },
                          [&](size_t r, unsigned d, unsigned q, Fr &x) { x = in.load(in.z + 8 * ((r * in.D() + d) * 2 + q)); },
                          [&](unsigned j, Fr &x) { x = in.load(in.stmt + 8 * j); });
        for (int t = 0; t < smck::EQ_TERMS; t++) fr_to_words(own + 8 * (e * smck::EQ_TERMS + t), o[t], false);
    }
}
// k_smc_stage on the host: the same slots, sources, flags and flip.  commitments: rows x 24 words, side_points: rows x S x 24, digit_points: rows x S l x 3 x 24,
// shared: 3 x 24; bases: rows x M x 4 x 24, pa / pb: rows x S l x 24, skip: 2 rows S l
void shim_smc_stage(const uint32_t *commitments, const uint32_t *side_points, const uint32_t *digit_points, const uint32_t *shared, int sides, int l, size_t rows, uint32_t *bases,
                    uint32_t *pa, uint32_t *pb, uint8_t *skip) {
    const size_t M = smck::eq_count(sides, l), D = smck::digit_count(sides, l), slices = rows * D;
    for (size_t t = 0; t < rows * M * 6; t++) {
        const size_t e = t / 6, i = e / M;
        const unsigned slot = (unsigned)(t % 6), m = (unsigned)(e % M);
        const smck::StageSrc src = smck::stage_src(sides, m, slot);
        if (src.kind < 0) continue;
        const size_t slice = i * D + (m - (unsigned)sides);
        uint32_t w[24];
        memcpy(w, src.kind == 0 ? shared + 24 * src.index : src.kind == 1 ? commitments + 24 * i : src.kind == 2 ? side_points + 24 * (i * sides + src.index)
                                                                                                             : digit_points + 24 * (slice * 3 + src.index), 96);
        uint32_t *dst = slot < 4 ? bases + (e * 4 + slot) * 24 : (slot == 4 ? pa : pb) + slice * 24;
        if (slot >= 4) skip[(slot - 4) * slices + slice] = smck::fq_zero_words(w, 24) ? 1 : 0;
        if (slot == 5) { uint32_t y[12]; smck::fq_neg_words(y, w + 12); memcpy(w + 12, y, 48); }
        memcpy(dst, w, 96);
    }
}
// k_smc_verdict: (status, detail) per proof from the flags
void shim_smc_verdict(const uint8_t *seg_inf, const uint8_t *pairing, const uint8_t *skip, int sides, int l, int merged, size_t rows, uint8_t *status, int32_t *detail) {
    const size_t M = smck::eq_count(sides, l), D = smck::digit_count(sides, l);
    for (size_t i = 0; i < rows; i++)
        smck::proof_verdict(sides, l, merged != 0, merged && pairing[i] != 0, [&](unsigned m) { return seg_inf[i * M + m] != 0; }, [&](unsigned d) { return pairing[i * D + d] != 0; },
                            [&](unsigned d) { return skip[i * D + d] != 0; }, status[i], detail[i]);
}
// k_smc_merge_weights: tw[8 slice ..] = tw[8 (slices + slice) ..] = random_i^d
void shim_smc_merge_weights(const uint32_t *random, int sides, int l, int mont, size_t rows, uint32_t *tw) {
    const size_t D = smck::digit_count(sides, l), slices = rows * D;
    for (size_t t = 0; t < slices; t++) {
        Fr rnd, w;
        fr_from_words(rnd, random + 8 * (t / D), mont != 0);
        smck::merge_weight(w, rnd, (unsigned)(t % D));
        fr_to_words(tw + 8 * t, w, false); fr_to_words(tw + 8 * (slices + t), w, false);
    }
}
// k_smc_own + k_smc_col_sums + k_col_finish over the proofs in chunks of `chunk` (dock_smc.hip verify_batch): a lane takes `run` equations.  own: total x M x 4
// x 8 canonical words (shim_smc_own's); c: 3 x 8 canonical words after the last chunk; w_c: total x 8, w_d: total x S x 8, w_digit: total x S l x 3 x 8, tp /
// tn: total x S l x 8
void shim_smc_columns(const uint32_t *own, const uint32_t *rho_words, int sides, int l, int mont, size_t total, size_t chunk, size_t run, uint32_t *c, uint32_t *w_c, uint32_t *w_d,
                      uint32_t *w_digit, uint32_t *tp, uint32_t *tn) {
    const size_t M = smck::eq_count(sides, l), D = smck::digit_count(sides, l);
    Fr rho; fr_from_words(rho, rho_words, mont != 0);
    col_frame_walk(total, chunk, M, run, 3, 0, 0, [&](size_t i0, size_t, size_t k, size_t lo, size_t cnt, Fr &sum) {
        // the chunk's arrays start at its first proof, as the driver's do
        const uint32_t *cown = own + 8 * 4 * M * i0;
        uint32_t *cwc = w_c + 8 * i0, *cwd = w_d + 8 * sides * i0, *cwg = w_digit + 8 * 3 * D * i0, *ctp = tp + 8 * D * i0, *ctn = tn + 8 * D * i0;
        smck::col_run(sides, l, rho, i0 * M, i0 * D, lo, cnt, (int)k, k == 0, [&](size_t e, unsigned q, Fr &x) { fr_from_words(x, cown + 8 * (e * 4 + q), false); },
                      [&](int kind, size_t idx, const Fr &x) {
                          uint32_t *dst = kind == 0 ? cwc : kind == 1 ? cwd : kind == 2 ? cwg : kind == 3 ? ctp : ctn;
                          fr_to_words(dst + 8 * idx, x, false);
                      },
                      sum);
    }, c);
}
// the word routines of k_smc_stage and k_smc_verdict
void shim_smc_fq_neg(const uint32_t *y, uint32_t *out) { smck::fq_neg_words(out, y); }
unsigned shim_smc_ref_position(int sides, int l, unsigned d) { return smck::ref_position(sides, l, d); }
}
