// crypto_amd/csrc/msm_host_fold.hpp — the host-side group arithmetic around the MSM pipelines: the folds of window sums and of partial results, the
// small linear combinations.  Host-only (host_field.hpp, the ABI header, the standard library): tests/native/msm_host_fold_driver.cpp builds it alone.
#pragma once
#include <vector>
#include "../../include/dock_gpu.h"
#include "host_field.hpp"

namespace dock {

// point I/O of the folds: an XYZZ point from four field elements of ABI words (the identity when flagged), a normalised Jacobian triple out
template <class HF> inline hostf::HXyzz<HF> load_xyzz(const uint64_t *src, bool inf) {
    hostf::HXyzz<HF> t = hostf::HXyzz<HF>::identity();
    if (inf) return t;
    const size_t FWORDS = sizeof(HF) / 8;
    t.inf = false; memcpy(&t.x, src, sizeof(HF)); memcpy(&t.y, src + FWORDS, sizeof(HF)); memcpy(&t.zz, src + 2 * FWORDS, sizeof(HF)); memcpy(&t.zzz, src + 3 * FWORDS, sizeof(HF));
    return t;
}
template <class HF> inline void store_jacobian(const hostf::HXyzz<HF> &p, uint64_t *out_xyz) {
    HF xyz[3]; p.to_normalised_jacobian(xyz[0], xyz[1], xyz[2]);
    memcpy(out_xyz, xyz, sizeof(xyz));
}
template <class HF> void write_identity(uint64_t *out_xyz) { store_jacobian(hostf::HXyzz<HF>::identity(), out_xyz); }
inline bool jac_is_identity(const uint64_t *xyz, size_t JW) { uint64_t z = 0; for (size_t k = 2 * JW / 3; k < JW; k++) z |= xyz[k]; return z == 0; }

// host tail: Horner over window sums (ABI XYZZ form), normalised Jacobian out
template <class HF>
void host_fold(const uint64_t *win_abi, const uint8_t *win_inf, int W, int c, uint64_t *out_xyz) {
    typedef hostf::HXyzz<HF> PT;
    PT acc = PT::identity();
    for (int w = W - 1; w >= 0; w--) {
        if (!acc.inf) for (int k = 0; k < c; k++) acc.dbl_in_place();
        if (!win_inf[w]) acc.add_in_place(load_xyzz<HF>(win_abi + (size_t)w * 4 * (sizeof(HF) / 8), false));
    }
    store_jacobian(acc, out_xyz);
}

// sum_j A_j + 2^lb * sum_j j S_j over the PW pseudo-windows (bucket b = j 2^lb + k of the one bucket set weighs b + 1 = (k + 1) + j 2^lb)
template <class HF>
void host_fold_shared(const uint64_t *a_abi, const uint8_t *a_inf, const uint64_t *s_abi, const uint8_t *s_inf, int PW, int lb, uint64_t *out_xyz) {
    typedef hostf::HXyzz<HF> PT;
    const size_t PWORDS = 4 * sizeof(HF) / 8;
    PT suffix = PT::identity(), weighted = PT::identity(), total = PT::identity();
    for (int j = PW - 1; j >= 1; j--) { suffix.add_in_place(load_xyzz<HF>(s_abi + (size_t)j * PWORDS, s_inf[j] != 0)); weighted.add_in_place(suffix); }   // sum_{j>=1} j S_j
    for (int k = 0; k < lb; k++) weighted.dbl_in_place();
    for (int j = 0; j < PW; j++) total.add_in_place(load_xyzz<HF>(a_abi + (size_t)j * PWORDS, a_inf[j] != 0));
    total.add_in_place(weighted);
    store_jacobian(total, out_xyz);
}

// P + 2^shift * sum_t 2^t M_t (reduce_kernels.hip.h): pts[0] = P, pts[1 + t] = M_t, nm marginals
template <class HF>
void host_fold_marginals(const uint64_t *pts, const uint8_t *inf, int nm, int shift, uint64_t *out_xyz) {
    typedef hostf::HXyzz<HF> PT;
    auto load = [&](int i) { return load_xyzz<HF>(pts + (size_t)i * 4 * (sizeof(HF) / 8), inf[i] != 0); };
    PT acc = PT::identity();
    for (int t = nm - 1; t >= 0; t--) { if (!acc.inf) acc.dbl_in_place(); acc.add_in_place(load(1 + t)); }
    if (!acc.inf) for (int k = 0; k < shift; k++) acc.dbl_in_place();
    acc.add_in_place(load(0));
    store_jacobian(acc, out_xyz);
}

// sum of k Jacobian triples (host): partial results gathered from the other ranks
template <class HF>
int32_t host_fold_jacobian(const uint64_t *xyz, size_t k, uint64_t *out_xyz) {
    if (!out_xyz || (k && !xyz)) return DGPU_E_BADARG;
    typedef hostf::HXyzz<HF> PT;
    PT acc = PT::identity();
    for (size_t i = 0; i < k; i++) {
        HF J[3]; memcpy(J, xyz + i * 3 * (sizeof(HF) / 8), sizeof(J));
        if (J[2].is_zero()) continue;
        PT t; t.inf = false; t.x = J[0]; t.y = J[1]; t.zz = J[2] * J[2]; t.zzz = t.zz * J[2];   // Jacobian (X, Y, Z) == XYZZ (X, Y, Z^2, Z^3)
        acc.add_in_place(t);
    }
    store_jacobian(acc, out_xyz);
    return DGPU_OK;
}

// sum_i s_i P_i over k <= DGPU_MAX_LINCOMB affine points on the HOST (4-bit windows, one table of 15 multiples per point, joint doublings).
// This is not the MSM path: it is the O(1) group arithmetic around it that the reference does with `mul_bigint` / FixedBase on the CPU — the
// r delta, s g_a + r g1_b, -rs delta - v eta/delta of a proof (prover.rs:309-313, 350-355, 585-594) — next to
// dgpu_fold_* and dgpu_final_exponentiation.  A 2..4-term product costs 0.15 - 0.35 ms of one host core and no device launch; the same
// through the bucket pipeline is ~0.75 ms of launch latency per call and queues behind the accumulation kernels of the large MSMs.
template <class HF>
int32_t host_lincomb(const uint64_t *points_xy, const uint8_t *is_inf, const uint64_t *scalars, size_t k, uint64_t *out_xyz) {
    if (!out_xyz || k > DGPU_MAX_LINCOMB || (k && (!points_xy || !scalars))) return DGPU_E_BADARG;
    typedef hostf::HXyzz<HF> PT;
    const size_t FWORDS = sizeof(HF) / 8;
    std::vector<PT> tab(k * 15);
    std::vector<uint8_t> live(k, 0);
    for (size_t i = 0; i < k; i++) {
        HF XY[2]; memcpy(XY, points_xy + i * 2 * FWORDS, sizeof(XY));
        const uint64_t *sc = scalars + 4 * i;
        uint64_t any = 0; for (size_t w = 0; w < 2 * FWORDS; w++) any |= points_xy[i * 2 * FWORDS + w];      // all-zero coordinates: the ABI's other spelling of the identity
        if ((is_inf && is_inf[i]) || !any || !(sc[0] | sc[1] | sc[2] | sc[3])) continue;
        live[i] = 1;
        PT p; p.inf = false; p.x = XY[0]; p.y = XY[1]; p.zz = HF::one(); p.zzz = HF::one();
        tab[i * 15] = p;
        for (int m = 1; m < 15; m++) { PT t = tab[i * 15 + m - 1]; if (m == 1) t.dbl_in_place(); else t.add_in_place(p); tab[i * 15 + m] = t; }
    }
    PT acc = PT::identity();
    for (int w = 63; w >= 0; w--) {
        for (int d = 0; d < 4; d++) acc.dbl_in_place();
        for (size_t i = 0; i < k; i++) {
            if (!live[i]) continue;
            const unsigned nib = (unsigned)(scalars[4 * i + (w >> 4)] >> ((w & 15) * 4)) & 15u;
            if (nib) acc.add_in_place(tab[i * 15 + nib - 1]);
        }
    }
    store_jacobian(acc, out_xyz);
    return DGPU_OK;
}

}  // namespace dock
