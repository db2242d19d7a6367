// crypto_amd/csrc/wm_block_kernels.hip.h — the whole R1CS -> QAP witness map of a SMALL circuit inside one block (dgpu_witness_map_r1cs_many).
//
// For a domain below 2^10 the single call (dock_qap.hip witness_map_device) is three k_csr_eval launches and one launch per stage of each of its
// seven transforms, each moving a few kilobytes.  Here a block keeps a, b and c of its statement(s) in LDS from the sparse rows to the h scalars:
//     a, b, c <- rows of A, B, C against z (csr_row: the row body of k_csr_eval, a_{m+j} = z_j included)
//     iFFT (decimation in frequency, natural in, bit-reversed out)  ->  * g^k / D on the way into the coset FFT (decimation in time, bit-reversed in,
//     natural out)  ->  a <- (a b - c) / Z(g)  ->  coset iFFT of a  ->  * g^-k / D, un-reversed, canonical (or Fr-limb) words to HBM
// Nothing is bit-reversed in memory, as in ntt_kernels.hip.h, and the lane bodies are the ones of ntt_lanes.hip.h in the order k_ntt_r4 runs them: an odd
// log2(D) starts with one radix-2 stage, the rest are radix-4 units whose only carry passes are the ones inside r4_dif / r4_dit (the FP29_CHECK
// operand asserts hold over the three transforms and the pointwise step without a further one: tests/test_witness_map_many_device_code_on_host.py).
// LDS: limb-major, word l of element e of array k at lds[(k * NL + l) * T + e], T = rows_per_block * D <= 2^10 elements: 120 B per element, 120 KB
// at the most.  A lane takes work items w, w + blockDim, ..: consecutive lanes touch consecutive words in the loads of the sparse phase, the
// pointwise step and the early DIT / late DIF stages; the unit's stride-4 element pattern of the other stages costs what it costs k_ntt_r4's flat pass.
// The body is a template over the executor X (lanes(fn): fn(lane, nlanes) for every lane of the block; sync(): the block's barrier), so that the
// host shim runs it as it is, phase by phase.
#pragma once
#include "ntt_lanes.hip.h"
#include "wm_block_args.hip.h"

namespace ntt {

// all log2(D) stages of one transform over the first `narr` arrays of the tile; pre != nullptr: every element is multiplied by pre[position]
// (limb-major, stride D) as the first stage loads it
template <bool DIF, class X>
FRD void wm_transform(X &x, uint32_t *lds, uint32_t T, int logn, uint32_t narr, const uint32_t *__restrict__ tw, const uint32_t *__restrict__ pre) {
    const uint32_t D = 1u << logn, H = D >> 1;
    auto lld = [&](Fr &v, uint32_t k, uint32_t e) {
#pragma unroll
        for (int l = 0; l < NL; l++) v.l[l] = lds[(size_t)(k * NL + l) * T + e];
    };
    auto lst = [&](uint32_t k, uint32_t e, const Fr &v) {
#pragma unroll
        for (int l = 0; l < NL; l++) lds[(size_t)(k * NL + l) * T + e] = v.l[l];
    };
    auto twiddle = [&](Fr &w, int st, uint32_t j) {
        const int sigma = DIF ? st : (logn - 1 - st);
        ld(w, tw + tw_stage_offset(H, sigma), H >> sigma, j);
    };
    auto load = [&](Fr &v, bool first, uint32_t k, uint32_t base, uint32_t m) {
        lld(v, k, base + m);
        if (first && pre) { Fr g; ld(g, pre, D, m); fr_mul(v, v, g); }
    };
    int st = 0;
    if (logn & 1) {                                        // one radix-2 stage: D / 2 butterflies per array and statement
        const uint32_t per = T >> 1, half_m = DIF ? H : 1u;
        x.lanes([&](uint32_t lane, uint32_t nlanes) {
            for (uint32_t w = lane; w < narr * per; w += nlanes) {
                const uint32_t k = w / per, u = w - k * per, rr = u >> (logn - 1), b = u & (H - 1), base = rr << logn;
                const uint32_t jm = b & (half_m - 1), m0 = ((b - jm) << 1) + jm, m1 = m0 + half_m;
                Fr tw0, a, c; twiddle(tw0, 0, jm);
                load(a, true, k, base, m0); load(c, true, k, base, m1);
                butterfly<DIF>(a, c, tw0);
                lst(k, base + m0, a); lst(k, base + m1, c);
            }
        });
        x.sync();
        st = 1;
    }
    for (; st + 1 < logn; st += 2) {                       // radix-4 units: D / 4 per array and statement
        const uint32_t per = T >> 2;
        const bool first = (st == 0);
        x.lanes([&](uint32_t lane, uint32_t nlanes) {
            for (uint32_t w = lane; w < narr * per; w += nlanes) {
                const uint32_t k = w / per, u = w - k * per, rr = u >> (logn - 2), q = u & ((D >> 2) - 1), base = rr << logn;
                Fr x00, x01, x10, x11;
                if (DIF) {
                    const int pos = logn - 2 - st;         // bit position of hb
                    const uint32_t hb = 1u << pos, ha = hb << 1;
                    const uint32_t jm = q & (hb - 1), m00 = ((q >> pos) << (pos + 2)) | jm;
                    Fr wa0, wa1, wb;
                    twiddle(wa0, st, jm); twiddle(wa1, st, jm + hb); twiddle(wb, st + 1, jm);
                    load(x00, first, k, base, m00); load(x10, first, k, base, m00 + ha);
                    load(x01, first, k, base, m00 + hb); load(x11, first, k, base, m00 + ha + hb);
                    r4_dif(x00, x01, x10, x11, wa0, wa1, wb);
                    lst(k, base + m00, x00); lst(k, base + m00 + hb, x01);
                    lst(k, base + m00 + ha, x10); lst(k, base + m00 + ha + hb, x11);
                } else {
                    const uint32_t ha = 1u << st, hb = ha << 1;
                    const uint32_t jm = q & (ha - 1), m00 = ((q >> st) << (st + 2)) | jm;
                    Fr wa, wb0, wb1;
                    twiddle(wa, st, jm); twiddle(wb0, st + 1, jm); twiddle(wb1, st + 1, jm + ha);
                    load(x00, first, k, base, m00); load(x01, first, k, base, m00 + ha);
                    load(x10, first, k, base, m00 + hb); load(x11, first, k, base, m00 + ha + hb);
                    r4_dit(x00, x01, x10, x11, wa, wb0, wb1);
                    lst(k, base + m00, x00); lst(k, base + m00 + ha, x01);
                    lst(k, base + m00 + hb, x10); lst(k, base + m00 + ha + hb, x11);
                }
            }
        });
        x.sync();
    }
}

// block `block` of a launch: statements [block * rows_per_block, ..) of the job; lds: 3 * NL * rows_per_block * D words
template <class X>
FRD void wm_block(X &x, uint32_t *lds, uint32_t block, const WmCircuit &c, const WmTables &tb, const WmJob &j) {
    const int logn = j.logn;
    const uint32_t D = 1u << logn, T = j.rows_per_block * D, row0 = block * j.rows_per_block;
    // 1. sparse rows (a statement past the end of the job is all zeros: it runs through the barriers with the others and writes nothing)
    x.lanes([&](uint32_t lane, uint32_t nlanes) {
        for (uint32_t w = lane; w < 3 * T; w += nlanes) {
            const uint32_t k = w / T, e = w - k * T, row = row0 + (e >> logn), i = e & (D - 1);
            Fr acc;
            if (row < j.nrows) csr_row(acc, c.rowptr[k], c.cols[k], c.vals[k], c.nnz[k], j.z_words + (size_t)row * j.row_words, j.z_mont != 0, c.rows, k == 0 ? c.extra : 0, i);
            else fr_zero(acc);
#pragma unroll
            for (int l = 0; l < NL; l++) lds[(size_t)(k * NL + l) * T + e] = acc.l[l];
        }
    });
    x.sync();
    // 2. - 4. iFFT (x D), then * g^k / D on the way into the coset FFT
    wm_transform<true>(x, lds, T, logn, 3, tb.tw_i, nullptr);
    wm_transform<false>(x, lds, T, logn, 3, tb.tw_f, tb.pwr_f);
    // 5. a <- (a b - c) / Z(g)
    x.lanes([&](uint32_t lane, uint32_t nlanes) {
        uint32_t zw[8];
#pragma unroll
        for (int k = 0; k < 8; k++) zw[k] = tb.zinv[k];
        Fr zi; fr_from_words(zi, zw, false);
        for (uint32_t e = lane; e < T; e += nlanes) {
            Fr a, b, cc, t;
#pragma unroll
            for (int l = 0; l < NL; l++) { a.l[l] = lds[(size_t)l * T + e]; b.l[l] = lds[(size_t)(NL + l) * T + e]; cc.l[l] = lds[(size_t)(2 * NL + l) * T + e]; }
            pointwise_lane(t, a, b, cc, zi);
#pragma unroll
            for (int l = 0; l < NL; l++) lds[(size_t)l * T + e] = t.l[l];
        }
    });
    x.sync();
    // 6. coset iFFT of a alone
    wm_transform<true>(x, lds, T, logn, 1, tb.tw_i, nullptr);
    // 7. * g^-k / D, un-reversed, as 4 x 64-bit scalars
    x.lanes([&](uint32_t lane, uint32_t nlanes) {
        for (uint32_t e = lane; e < T; e += nlanes) {
            const uint32_t row = row0 + (e >> logn), p = e & (D - 1);
            if (row >= j.nrows) continue;
            Fr v, g;
#pragma unroll
            for (int l = 0; l < NL; l++) v.l[l] = lds[(size_t)l * T + e];
            ld(g, tb.pwr_i, D, p);
            fr_mul(v, v, g);
            uint32_t w[8]; fr_to_words(w, v, j.out_mont != 0);
            st_words(j.out_words, (size_t)row * D + bitrev(p, logn), w);
        }
    });
}

#if defined(__HIPCC__)
struct WmBlockLanes {
    template <class F> __device__ __forceinline__ void lanes(F fn) { fn(threadIdx.x, blockDim.x); }
    __device__ __forceinline__ void sync() { __syncthreads(); }
};
__global__ void __launch_bounds__(WM_BLOCK_THREADS) k_wm_block(WmCircuit c, WmTables tb, WmJob j) {
    extern __shared__ uint32_t wm_lds[];
    WmBlockLanes x;
    wm_block(x, wm_lds, blockIdx.x, c, tb, j);
}
#endif

}  // namespace ntt
