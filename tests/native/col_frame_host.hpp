// tests/native/col_frame_host.hpp — the ONE host walk of the batch verifiers' column sums (crypto_amd/csrc/col_sums.hip.h), as the kernels and drivers do it:
// the `total` rows in chunks of `chunk`; per chunk and column the blocks of 256 lanes of `run` items each (items = rows * per: the rows themselves, or a row's
// equations), lane_run where a lane's range is not empty, the block's fixed tree and its reduction to a product (col_block_sum), then the second pass onto the
// running sums in block order with the columns in [neg_lo, neg_hi) leaving negated (k_col_finish).  Compiled with -DFP29_CHECK by every scheme's shim, so the
// frame's operand contracts are asserted for each of them.
//   lane_run(i0, rows, k, lo, cnt, Fr &sum)   the scheme's run of column k over the items [lo, lo + cnt) of the chunk of `rows` rows that starts at row i0
//   c                                         ncols x 8 canonical words: the sums (or minus them) as they stand after the last chunk
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../crypto_amd/csrc/col_sums.hip.h"

template <class LaneRun>
void col_frame_walk(size_t total, size_t chunk, size_t per, size_t run, size_t ncols, size_t neg_lo, size_t neg_hi, LaneRun lane_run, uint32_t *c) {
    using namespace fr29;
    std::vector<Fr> run_sums(ncols);
    for (size_t i0 = 0; i0 < total; i0 += chunk) {
        const size_t rows = total - i0 < chunk ? total - i0 : chunk, count = rows * per, nb = (count + 256 * run - 1) / (256 * run);
        std::vector<Fr> part(ncols * nb);
        for (size_t k = 0; k < ncols; k++)
            for (size_t b = 0; b < nb; b++) {
                Fr sh[256];
                for (unsigned t = 0; t < 256; t++) {
                    const size_t lo = (b * 256 + t) * run, cnt = lo >= count ? 0 : (count - lo < run ? count - lo : run);
                    fr_zero(sh[t]);
                    if (cnt) lane_run(i0, rows, k, lo, cnt, sh[t]);
                }
                for (unsigned d = 128; d >= 1; d >>= 1)
                    for (unsigned t = 0; t < d; t++) colk::tree_step(t, d, [&](unsigned q, Fr &x) { x = sh[q]; }, [&](unsigned q, const Fr &x) { sh[q] = x; });
                Fr one; fr_one(one);
                fr_mul(part[k * nb + b], sh[0], one);
            }
        for (size_t k = 0; k < ncols; k++) {
            Fr start, ck, o;
            if (i0 == 0) fr_zero(start); else start = run_sums[k];
            colk::col_finish(start, nb, [&](size_t b, Fr &v) { v = part[k * nb + b]; }, ck);
            run_sums[k] = ck;
            if (k >= neg_lo && k < neg_hi) colk::neg_product(o, ck); else o = ck;
            fr_to_words(c + 8 * k, o, false);
        }
    }
}
