// tests/native/wm_block_host_shim.cpp — host build (g++) of the DEVICE block witness map (crypto_amd/csrc/wm_block_kernels.hip.h: wm_block, the body
// k_wm_block launches) with the FP29_CHECK operand asserts of fr29.hip.h: every product of the fused chain (sparse rows, three transforms back to
// back, the pointwise step) checks its limbs and its value bound on the actual operands.  The executor runs the lanes of a block one after another,
// phase by phase, which is what the barriers of the device executor allow.  The domain's tables are built here the way dock_qap.hip get_domain
// builds them (powers, per-stage twiddle tables, bit-reversed coset factors).  Test-only: tests/test_witness_map_many_device_code_on_host.py
// compares the words with the oracle; an assertion that fires inside means a lazy-limb overflow is possible for some input.
#define FP29_CHECK 1
#include "../../crypto_amd/csrc/wm_block_kernels.hip.h"
#include <string.h>
#include <vector>
using namespace ntt;

namespace {
struct HostLanes {
    uint32_t n;
    template <class F> void lanes(F fn) { for (uint32_t t = 0; t < n; t++) fn(t, n); }
    void sync() {}
};
Fr from_canon(const uint64_t *w) { uint32_t v[8]; memcpy(v, w, 32); Fr x; fr_from_words(x, v, false); return x; }
// out[k] = base^k * scale, limb-major with stride count (k_fr_powers)
void powers(const Fr &base, const Fr &scale, size_t count, uint32_t *out) {
    for (size_t k = 0; k < count; k++) {
        Fr b = base, acc = scale;
        for (size_t e = k; e; e >>= 1) { if (e & 1) fr_mul(acc, acc, b); fr_mul(b, b, b); }
        st(out, count, k, acc);
    }
}
// the per-stage tables behind T_0 (k_tw_compact)
void compact(uint32_t *tw, size_t H) {
    for (int sigma = 1; (H >> sigma) >= 1 && H > 1; sigma++) {
        const size_t hs = H >> sigma;
        uint32_t *dst = tw + tw_stage_offset(H, sigma);
        for (size_t j = 0; j < hs; j++) for (int l = 0; l < NL; l++) dst[(size_t)l * hs + j] = tw[(size_t)l * H + (j << sigma)];
    }
}
}  // namespace

extern "C" {
// consts: w, w^-1, g, g^-1, 1/D, 1, 1/Z(g) as canonical words.  mats: rowptr / cols / vals (canonical or Fr limbs by `mont`) of A, B, C.  z: nrows rows of
// row_stride scalars.  out: nrows * D * 4 words.  Returns the number of blocks run.
int shim_wm_many(int logn, uint32_t rows_per_block, uint32_t nlanes, uint32_t nrows, const uint64_t *consts,
                 const uint64_t *a_rp, const uint32_t *a_cl, const uint64_t *a_vl, const uint64_t *b_rp, const uint32_t *b_cl, const uint64_t *b_vl,
                 const uint64_t *c_rp, const uint32_t *c_cl, const uint64_t *c_vl, size_t num_constraints, size_t num_inputs, size_t num_vars,
                 const uint64_t *z, size_t row_stride, int mont, int out_mont, uint64_t *out) {
    const size_t D = (size_t)1 << logn, H = D >> 1 ? D >> 1 : 1;
    Fr w = from_canon(consts), wi = from_canon(consts + 4), g = from_canon(consts + 8), gi = from_canon(consts + 12), dinv = from_canon(consts + 16), one = from_canon(consts + 20);
    std::vector<uint32_t> tw_f(2 * H * NL), tw_i(2 * H * NL), pw_f(D * NL), pw_i(D * NL), pwr_f(D * NL), pwr_i(D * NL);
    powers(w, one, H, tw_f.data()); powers(wi, one, H, tw_i.data()); compact(tw_f.data(), H); compact(tw_i.data(), H);
    powers(g, dinv, D, pw_f.data()); powers(gi, dinv, D, pw_i.data());
    for (size_t p = 0; p < D; p++) for (int l = 0; l < NL; l++) { const size_t k = bitrev((uint32_t)p, logn); pwr_f[l * D + p] = pw_f[l * D + k]; pwr_i[l * D + p] = pw_i[l * D + k]; }
    const uint64_t *rp[3] = {a_rp, b_rp, c_rp}; const uint32_t *cl[3] = {a_cl, b_cl, c_cl}; const uint64_t *vl[3] = {a_vl, b_vl, c_vl};
    std::vector<uint32_t> vals[3];
    WmCircuit c;
    for (int k = 0; k < 3; k++) {
        const size_t nnz = rp[k][num_constraints], stride = nnz ? nnz : 1;
        vals[k].assign(stride * NL, 0);
        for (size_t i = 0; i < nnz; i++) { uint32_t v[8]; memcpy(v, vl[k] + 4 * i, 32); Fr x; fr_from_words(x, v, mont != 0); st(vals[k].data(), stride, i, x); }   // k_fr_load
        c.rowptr[k] = rp[k]; c.cols[k] = cl[k]; c.vals[k] = vals[k].data(); c.nnz[k] = stride;
    }
    c.rows = num_constraints; c.extra = num_inputs;
    (void)num_vars;
    uint32_t zinv_words[8]; memcpy(zinv_words, consts + 24, 32);
    const WmTables tb{tw_f.data(), tw_i.data(), pwr_f.data(), pwr_i.data(), zinv_words};
    const WmJob j{(const uint32_t *)z, row_stride * 8, mont, nrows, (uint32_t *)out, out_mont, logn, rows_per_block};
    std::vector<uint32_t> lds((size_t)3 * NL * rows_per_block * D);
    const uint32_t blocks = (nrows + rows_per_block - 1) / rows_per_block;
    HostLanes x{nlanes};
    for (uint32_t b = 0; b < blocks; b++) wm_block(x, lds.data(), b, c, tb, j);
    return (int)blocks;
}
}
