// crypto_amd/csrc/many_kernels.hip.h — MANY small MSMs over one resident base set in one call: m rows of n <= 2^13 scalars against the small path's
// table of a handle (small_kernels.hip.h: the eight multiples of P, 2^64 P, 2^128 P, 2^192 P per base).
//
// The reference issues its small MSMs in batches over one base vector (verifiable_encryption/src/tz_21/dkgith.rs:174-192 and :368, rdkgith.rs:140-147,
// bbs_plus/src/setup.rs:128-146, kvac/src/bbdt_2016/setup.rs:109, schnorr_pok/src/pok_generalized_pedersen.rs:97,153).  One row through k_small_tree is a
// launch of 16 trees over 4 n leaves on an empty chip plus a 60-doubling fold on a host core; here the rows of a chunk share two launches:
//
//   k_many_tree : the tree of k_small_tree<A, 4> with a row index.  grid = (blocks per row, 16 super-windows, row blocks); row r reads its scalars at
//                 scalars + 8 r row_stride words and owns its window counters, partials and 16 window sums with their flags.  Short rows are PACKED,
//                 several to a block, as segments whose folds stop at the row boundary (many_fold.hip.h many_geometry): neighbouring groups then gather
//                 from neighbouring rows of the same small table, which stays in L2.  The window sums stay on the device, in the accumulator's own form.
//   k_many_fold : per row, on four members like the tree: Horner over the 16 window sums (four doublings between them), one inversion
//                 (fp_safegcd.hip.h), the ABI words of the normalised Jacobian point host_fold would have produced, and the identity flag.
//
// A scalar >= 2^255 anywhere in the launch raises ONE flag word (the refusal covers the whole call).
#pragma once
#include "small_kernels.hip.h"
#include "many_fold.hip.h"

namespace msm {

static_assert(MANY_SUB == SMALL_S && MANY_WIN == SMALL_W / SMALL_S && MANY_MAX_N == SMALL_MSM_MAX_N, "the resident table's layout");

// count[row * 16 + v] must be zero at launch when gridDim.x > 1 (low 16 bits: blocks done)
template <class A>
__global__ void __launch_bounds__(256 * A::LPP) k_many_tree(const uint32_t *__restrict__ tab, const uint8_t *__restrict__ tab_inf, const uint32_t *__restrict__ scalars, size_t n,
                                                             size_t row_stride, size_t rows, uint32_t *__restrict__ partial, uint8_t *__restrict__ partial_inf, uint32_t *__restrict__ count,
                                                             uint32_t *__restrict__ win, uint8_t *__restrict__ win_inf, uint32_t *__restrict__ bad_flag, ManyGeom geo) {
    typedef typename A::F F;
    constexpr int LPP = A::LPP, GL = 4 * LPP, PW_ = 4 * SN, S = SMALL_S, WPS = SMALL_W / S;
    __shared__ uint32_t xs[64 * LPP * PW_];
    __shared__ uint8_t fl[64];
    __shared__ uint32_t last_flag;
    const int t = (int)threadIdx.x, gi = t / GL, h = t % LPP;
    const int seg = geo.seg, gs = gi & (seg - 1);
    const QuadLanes<LPP> q4;
    const unsigned j = blockIdx.x, v = blockIdx.y, nblk = gridDim.x;
    const size_t row = (size_t)blockIdx.z * geo.rows_per_block + (size_t)(gi / seg);
    const bool live = row < rows;                                  // (a block's last segments may be padding: they follow the barriers and write nothing)
    const uint32_t *const sc = scalars + (live ? row : 0) * row_stride * 8;
    const size_t L = n * S;
    uint32_t bad = 0;
    auto zero = [](Xyzz<F> &p) __attribute__((always_inline)) { fzero(p.x); fzero(p.y); fzero(p.zz); fzero(p.zzz); };
    auto leaf = [&](Xyzz<F> &p, bool &pinf, size_t l) __attribute__((always_inline)) {
        pinf = true; zero(p);
        if (!live || l >= L) return;
        const unsigned sub = (uint32_t)l / (uint32_t)n;
        const size_t i = l - (size_t)sub * n;
        uint32_t mag; bool neg;
        small_digit(sc + i * 8, (int)(WPS * sub + v), mag, neg, bad);
        if (mag == 0) return;
        const size_t at = (i * S + sub) * SMALL_E + (mag - 1);
        if (tab_inf[at]) return;
        load_soa<A>(p, tab, 0, at);
        pinf = false;
        if (neg) neg_in_place(p.y);
    };
    // o = the point of group gi + d when that group belongs to the same segment (k_small_tree's exchange: member r parks coordinate r)
    auto from_group = [&](Xyzz<F> &o, bool &oinf, const Xyzz<F> &x, bool xinf, int d, int width) __attribute__((always_inline)) {
        __syncthreads();
        { const uint32_t *wx = reinterpret_cast<const uint32_t *>(&x);
          const int r = q4.role;
          uint32_t *dst = xs + ((gi * 4 + r) * LPP + h) * SN;
#pragma unroll
          for (int k = 0; k < SN; k++) dst[k] = pick4(r, wx[k], wx[SN + k], wx[2 * SN + k], wx[3 * SN + k]);
          if (t % GL == 0) fl[gi] = xinf; }
        __syncthreads();
        const int sg = gi + d;
        oinf = true;
        if (many_pairs(width, gi & (width - 1), d)) {
            uint32_t *ov = reinterpret_cast<uint32_t *>(&o);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t *sv = xs + ((sg * 4 + c) * LPP + h) * SN;
#pragma unroll
                for (int k = 0; k < SN; k++) ov[c * SN + k] = sv[k];
            }
            oinf = fl[sg] != 0;
        } else o = x;
    };
    auto tree = [&](Xyzz<F> &a, bool &ainf, int width) __attribute__((always_inline)) {
#pragma unroll 1
        for (int d = width >> 1; d >= 1; d >>= 1) {
            Xyzz<F> o; bool oinf; from_group(o, oinf, a, ainf, d, width);
            xyzz_add_rounds(a, ainf, o, oinf, q4);
        }
    };
    auto write_window = [&](const Xyzz<F> &a, bool ainf) __attribute__((always_inline)) {      // the first group of a segment: the row's window sum
        if (gs != 0 || !live) return;
        const size_t at = row * WPS + v;
        if (q4.role == 0) store_soa<A>(win, 0, at, a);
        if (t % GL == 0) win_inf[at] = ainf;
    };
    // (the lambdas above are forced inline: an outlined one takes the accumulator by reference, i.e. through scratch memory — small_kernels.hip.h)
    Xyzz<F> acc, o; bool ainf, oinf;
    leaf(acc, ainf, many_leaf(geo, j, gs, 0));
#pragma unroll 1
    for (int k = 1; k < geo.per_group; k++) { leaf(o, oinf, many_leaf(geo, j, gs, k)); xyzz_add_rounds(acc, ainf, o, oinf, q4); }
    tree(acc, ainf, seg);
    const uint32_t block_bad = (uint32_t)__syncthreads_or((int)bad);
    if (block_bad && t == 0) atomicOr(bad_flag, 1u);
    if (nblk == 1) { write_window(acc, ainf); return; }
    // several blocks per row and window (seg == 64: the whole block is one row): the last one to finish folds the partials
    const size_t slot = (row * WPS + v) * nblk;
    if (gi == 0 && live) {
        if (q4.role == 0) store_soa<A>(partial, 0, slot + j, acc);
        if (t == 0) partial_inf[slot + j] = ainf;
    }
    __threadfence();
    __syncthreads();
    if (t == 0) last_flag = live ? atomicAdd(&count[row * WPS + v], 1u) + 1u : 0u;
    __syncthreads();
    if (last_flag != nblk) return;
    __threadfence();
    ainf = true; zero(acc);
    if ((unsigned)gi < nblk) {
        ainf = partial_inf[slot + gi] != 0;
        if (!ainf) load_soa<A>(acc, partial, 0, slot + gi);
    }
    int width = 1; while ((unsigned)width < nblk) width <<= 1;
    tree(acc, ainf, width);
    write_window(acc, ainf);
}

// the tail of one row / segment on its four members: Horner over the `nwin` window sums at win[at0 .. at0 + nwin) (the accumulator's own form), one inversion,
// then out_xyz[row] = the normalised Jacobian point (X, Y, 1) in ABI words, (1, 1, 0) and out_inf[row] = 1 for the identity — word for word what host_fold
// writes.  No barrier: whole groups run it together.
template <class A>
__device__ __forceinline__ void many_fold_row(const uint32_t *__restrict__ win, const uint8_t *__restrict__ win_inf, size_t at0, int nwin, size_t row,
                                              uint32_t *__restrict__ out_xyz, uint8_t *__restrict__ out_inf) {
    typedef typename A::F F;
    constexpr int LPP = A::LPP, GL = 4 * LPP, OW = 3 * 12 * LPP;
    const int t = (int)threadIdx.x, h = t % LPP;
    const QuadLanes<LPP> q4;
    F ox, oy, oz; bool ainf;
    many_tail(ox, oy, oz, ainf, nwin, [&](Xyzz<F> &s, int v) __attribute__((always_inline)) {
        const size_t at = at0 + v;
        const bool sinf = win_inf[at] != 0;
        fzero(s.x); fzero(s.y); fzero(s.zz); fzero(s.zzz);
        if (!sinf) load_soa<A>(s, win, 0, at);
        return sinf;
    }, q4);
    if (t % GL == 0) out_inf[row] = ainf;
    const int r = q4.role;                                            // member r < 3 converts coordinate r (G2: each lane its half)
    const Fs *fx = reinterpret_cast<const Fs *>(&ox), *fy = reinterpret_cast<const Fs *>(&oy), *fz = reinterpret_cast<const Fs *>(&oz);
    Fs mine;
#pragma unroll
    for (int k = 0; k < SN; k++) mine.l[k] = pick4(r, fx->l[k], fy->l[k], fz->l[k], fz->l[k]);
    if (r < 3) fs_to_abi(out_xyz + row * OW + 12 * (LPP * r + h), mine);
}

// row r: the tail over its 16 super-window sums.  One group of four members per row; whole groups leave together.
template <class A>
__global__ void __launch_bounds__(256 * A::LPP) k_many_fold(const uint32_t *__restrict__ win, const uint8_t *__restrict__ win_inf, size_t rows,
                                                             uint32_t *__restrict__ out_xyz, uint8_t *__restrict__ out_inf) {
    constexpr int GL = 4 * A::LPP, WPS = SMALL_W / SMALL_S;
    const size_t row = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / GL;
    if (row >= rows) return;
    many_fold_row<A>(win, win_inf, row * WPS, WPS, row, out_xyz, out_inf);
}

// launchers (instantiated by k_g1_many.hip / k_g2_many.hip; declared in msm_launch.hip.h)
template <class C> void launch_many_tree(hipStream_t s, const uint32_t *tab, const uint8_t *tab_inf, const uint32_t *scalars, size_t n, size_t row_stride, size_t rows, uint32_t *partial,
                                         uint8_t *partial_inf, uint32_t *count, uint32_t *win, uint8_t *win_inf, uint32_t *bad_flag) {
    typedef typename C::ACC A;
    const ManyGeom g = many_geometry(n);
    const unsigned zb = (unsigned)((rows + g.rows_per_block - 1) / g.rows_per_block);
    hipLaunchKernelGGL((k_many_tree<A>), dim3(g.nblk, SMALL_W / SMALL_S, zb), dim3(256 * A::LPP), 0, s, tab, tab_inf, scalars, n, row_stride, rows, partial, partial_inf, count, win, win_inf, bad_flag, g);
}
template <class C> void launch_many_fold(hipStream_t s, const uint32_t *win, const uint8_t *win_inf, size_t rows, uint32_t *out_xyz, uint8_t *out_inf) {
    typedef typename C::ACC A;
    hipLaunchKernelGGL((k_many_fold<A>), dim3((unsigned)((rows + 63) / 64)), dim3(256 * A::LPP), 0, s, win, win_inf, rows, out_xyz, out_inf);
}

}  // namespace msm
