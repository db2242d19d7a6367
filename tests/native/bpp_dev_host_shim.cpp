// tests/native/bpp_dev_host_shim.cpp — the __host__ __device__ routines of Bulletproofs++ range proofs in bulk (crypto_amd/csrc/bpp_kernels.hip.h: bpp_consts,
// bpp_shared, batch_weight_index, shape_ok / make_shape, with col_sums.hip.h's col_run, tree_step, col_finish and neg_product) compiled for the host with
// -DFP29_CHECK (every product asserts its operand contract), driven the way k_bpp_consts, k_bpp_shared, k_bpp_col_sums / k_col_finish and dock_bpp.hip's
// chunks drive them (col_frame_host.hpp).  Built and loaded by tests/test_bpp_device_code_on_host.py.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/bpp_kernels.hip.h"
#include "col_frame_host.hpp"
using namespace fr29;

namespace {
// k_bpp_consts + k_bpp_shared over `rows` proofs: the record lives here
void scalars(const bppk::Shape &s, const uint32_t *chal, const uint32_t *l_n, int mont, size_t rows, size_t own_stride, uint32_t *shared, uint32_t *own, uint8_t *bad) {
    const size_t nc = (size_t)(bppk::N_CHAL + s.K), n = (size_t)(bppk::SHARED0 + s.NG);
    std::vector<Fr> rec(bppk::REC_N);
    for (size_t i = 0; i < rows; i++) {
        for (auto &x : rec) fr_zero(x);
        const bool b = bppk::bpp_consts(s, own_stride > (size_t)s.own, [&](int k, Fr &x) { fr_from_words(x, chal + 8 * (i * nc + (size_t)k), mont != 0); },
                                        [&](int k, Fr &x) { fr_from_words(x, l_n + 8 * (i * 2 + (size_t)k), mont != 0); }, [&](int idx, Fr &x) { x = rec[idx]; },
                                        [&](int idx, const Fr &x) { rec[idx] = x; }, [&](int slot, const Fr &x) { fr_to_words(own + 8 * (i * own_stride + (size_t)slot), x, false); });
        bad[i] = b ? 1 : 0;
        for (size_t slot = 0; slot < n; slot++) {
            Fr o;
            bppk::bpp_shared(s, (unsigned)slot, [&](int idx, Fr &x) { x = rec[idx]; }, o);
            fr_to_words(shared + 8 * (i * n + slot), o, false);
        }
    }
}
}  // namespace

extern "C" {
// 0 for a shape the calls refuse, else NG, K, own
int shim_bpp_shape(unsigned base, unsigned num_bits, unsigned m, int *NG, int *K, int *own) {
    if (!bppk::shape_ok(base, num_bits, m)) return 0;
    const bppk::Shape s = bppk::make_shape(base, num_bits, m);
    *NG = s.NG; *K = s.K; *own = s.own;
    return 1;
}
// chal: rows x (7 + K) x 8 words, l_n: rows x 2 x 8 -> shared: rows x (9 + NG) x 8 canonical words, own: rows x own_stride x 8, bad: rows
void shim_bpp_scalars(unsigned base, unsigned num_bits, unsigned m, const uint32_t *chal, const uint32_t *l_n, int mont, size_t rows, size_t own_stride, uint32_t *shared, uint32_t *own,
                      uint8_t *bad) {
    scalars(bppk::make_shape(base, num_bits, m), chal, l_n, mont, rows, own_stride, shared, own, bad);
}
// k_bpp_col_sums + k_col_finish over the proofs in chunks of `chunk` (dock_bpp.hip verify_batch): a lane takes `run` proofs.  shared / own: shim_bpp_scalars's
// with own_stride = own, of all `total` proofs.  c: (9 + NG) x 8 canonical words after the last chunk; wts: total x own x 8, every chunk's part in the order
// [over values | over round points | over wnla points] of that chunk
void shim_bpp_columns(unsigned base, unsigned num_bits, unsigned m, const uint32_t *shared, const uint32_t *own, const uint32_t *rho_words, int mont, size_t total, size_t chunk, size_t run,
                      uint32_t *c, uint32_t *wts) {
    const bppk::Shape s = bppk::make_shape(base, num_bits, m);
    const size_t n = (size_t)(bppk::SHARED0 + s.NG);
    Fr rho; fr_from_words(rho, rho_words, mont != 0);
    col_frame_walk(total, chunk, 1, run, n, 0, 0, [&](size_t i0, size_t rows, size_t k, size_t lo, size_t cnt, Fr &sum) {
        const uint32_t *csh = shared + 8 * n * i0, *cown = own + 8 * (size_t)s.own * i0;
        uint32_t *cw = wts + 8 * (size_t)s.own * i0;
        colk::col_run(rho, i0 + lo, cnt, [&](size_t j, Fr &v) { fr_from_words(v, csh + 8 * ((lo + j) * n + k), false); },
                      [&](size_t j, const Fr &w) {
                          if (k != 0) return;
                          for (int q = 0; q < s.own; q++) {
                              Fr a, p;
                              fr_from_words(a, cown + 8 * ((lo + j) * (size_t)s.own + (size_t)q), false);
                              fr_mul(p, a, w);
                              fr_to_words(cw + 8 * bppk::batch_weight_index(s, rows, lo + j, (unsigned)q), p, false);
                          }
                      },
                      sum);
    }, c);
}
}
