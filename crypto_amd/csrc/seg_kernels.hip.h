// crypto_amd/csrc/seg_kernels.hip.h — MANY small MSMs, each over its OWN bases, in one call: a batch of N terms cut into segments of ragged lengths
// (each at most 2^13 terms), one result per segment.
//
// The reference issues such batches back to back: saver/src/encryption.rs:710-740 (chunks + 2 msm_bigint calls, one per ciphertext column),
// legogroth16/src/link/utils.rs:85-120 (one sum per matrix column), the paired halving MSMs of legogroth16/src/aggregation/utils.rs:51-81 and the per-proof
// MSMs of bbs_plus/src/proof.rs:580.  One segment through the small path (small_kernels.hip.h) is a table launch and a tree launch on an empty chip plus a
// 252-doubling fold on a host core; here the segments of a chunk share
//
//   k_small_table : the existing kernel over ALL the chunk's bases: eight multiples per base (the S = 1 table)
//   k_seg_tree    : the tree of k_small_tree<A, 1> / k_many_tree with a per-group DESCRIPTOR instead of a row index (seg_layout.hip.h: segment, first term,
//                   leaf count, width, position).  grid = (blocks, 64 windows).  Short segments are packed several to a block at offsets aligned to their
//                   own width and a tree level only pairs groups of one segment; a segment of more than 512 terms owns whole blocks, and the last of them
//                   to finish folds their partials (k_small_tree's counter scheme).  The window sums leave in the accumulator's own form (for k_seg_fold)
//                   or in the form host_fold reads (for the host threads' fold: few segments)
//   k_seg_fold    : per segment, on four members: Horner over the 64 window sums, one inversion, the ABI words and the identity flag (many_fold_row)
//
// A scalar >= 2^255 anywhere in the launch raises ONE flag word (the refusal covers the whole call).
#pragma once
#include "many_kernels.hip.h"
#include "seg_layout.hip.h"

namespace msm {

static_assert(SEG_WIN == SMALL_W && SEG_MAX_N == SMALL_MSM_MAX_N && sizeof(SegDesc) == 16, "the S = 1 table's layout");

// desc: 64 descriptors per block.  count[pslot * 64 + v] of every multi-block segment must be zero at launch (low 16 bits: blocks done).
// abi == 0: win[(seg * 64 + v)] in the accumulator's form (store_soa); abi != 0: 4 * 12 * LPP ABI words per window sum (k_small_tree's write_window)
template <class A>
__global__ void __launch_bounds__(256 * A::LPP) k_seg_tree(const uint32_t *__restrict__ tab, const uint8_t *__restrict__ tab_inf, const uint32_t *__restrict__ scalars,
                                                            const uint4 *__restrict__ desc, uint32_t *__restrict__ partial, uint8_t *__restrict__ partial_inf, uint32_t *__restrict__ count,
                                                            uint32_t *__restrict__ win, uint8_t *__restrict__ win_inf, int abi, uint32_t *__restrict__ bad_flag) {
    typedef typename A::F F;
    constexpr int LPP = A::LPP, GL = 4 * LPP, PW_ = 4 * SN;
    __shared__ uint32_t xs[64 * LPP * PW_];
    __shared__ uint8_t fl[64];
    __shared__ uint32_t last_flag;
    const int t = (int)threadIdx.x, gi = t / GL, h = t % LPP;
    const QuadLanes<LPP> q4;
    const unsigned v = blockIdx.y;
    const uint4 dv = desc[(size_t)blockIdx.x * 64 + gi];
    const uint32_t seg = dv.x, first = dv.y, n = seg_n(dv.z);
    const int per_group = seg_per_group(dv.z), width = seg_width(dv.z), gs = gi & (width - 1);
    const unsigned j = seg_block(dv.z), nblk = seg_nblk(dv.z);      // (nblk > 1: the whole block is one segment)
    const bool live = seg != SEG_NONE;
    uint32_t bad = 0;
    auto zero = [](Xyzz<F> &p) __attribute__((always_inline)) { fzero(p.x); fzero(p.y); fzero(p.zz); fzero(p.zzz); };
    auto leaf = [&](Xyzz<F> &p, bool &pinf, uint32_t l) __attribute__((always_inline)) {
        pinf = true; zero(p);
        if (!live || l >= n) return;
        const size_t i = (size_t)first + l;
        uint32_t mag; bool neg;
        small_digit(scalars + i * 8, (int)v, mag, neg, bad);
        if (mag == 0) return;
        const size_t at = i * SMALL_E + (mag - 1);
        if (tab_inf[at]) return;
        load_soa<A>(p, tab, 0, at);
        pinf = false;
        if (neg) neg_in_place(p.y);
    };
    // o = the point of group gi + d when that group belongs to the same segment (k_small_tree's exchange: member r parks coordinate r)
    auto from_group = [&](Xyzz<F> &o, bool &oinf, const Xyzz<F> &x, bool xinf, int d, int w) __attribute__((always_inline)) {
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
        if (seg_pairs(w, gi & (w - 1), d)) {
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
    // `levels`: the widest segment of the block (block-uniform: everybody meets every barrier; seg_layout writes it into every descriptor); w: this group's own segment
    auto tree = [&](Xyzz<F> &a, bool &ainf, int levels, int w) __attribute__((always_inline)) {
#pragma unroll 1
        for (int d = levels >> 1; d >= 1; d >>= 1) {
            Xyzz<F> o; bool oinf; from_group(o, oinf, a, ainf, d, w);
            xyzz_add_rounds(a, ainf, o, oinf, q4);
        }
    };
    auto write_window = [&](const Xyzz<F> &a, bool ainf) __attribute__((always_inline)) {      // the first group of a segment (of the block, when the segment owns it): its window sum
        if (gs != 0 || !live) return;
        const size_t at = (size_t)seg * SMALL_W + v;
        if (t % GL == 0) win_inf[at] = ainf;
        if (!abi) { if (q4.role == 0) store_soa<A>(win, 0, at, a); return; }
        const int r = q4.role;                                        // member r converts coordinate r (G2: each lane its half)
        const Fs *fa = reinterpret_cast<const Fs *>(&a);
        constexpr int WS = 4 * 12 * LPP;
        Fs mine;
#pragma unroll
        for (int k = 0; k < SN; k++) mine.l[k] = pick4(r, fa[0].l[k], fa[1].l[k], fa[2].l[k], fa[3].l[k]);
        if (!ainf) fs_to_abi(win + at * WS + 12 * (LPP * r + h), mine);
    };
    // (the lambdas above are forced inline: an outlined one takes the accumulator by reference, i.e. through scratch memory — small_kernels.hip.h)
    const int levels = seg_levels(dv.z);                             // the widest segment of the block: the same in all its descriptors
    Xyzz<F> acc, o; bool ainf, oinf;
    leaf(acc, ainf, seg_leaf(per_group, width, j, gs, 0));
#pragma unroll 1
    for (int k = 1; k < per_group; k++) { leaf(o, oinf, seg_leaf(per_group, width, j, gs, k)); xyzz_add_rounds(acc, ainf, o, oinf, q4); }
    tree(acc, ainf, levels, width);
    const uint32_t block_bad = (uint32_t)__syncthreads_or((int)bad);
    if (block_bad && t == 0) atomicOr(bad_flag, 1u);
    if (nblk == 1) { write_window(acc, ainf); return; }
    // several blocks for this segment and window (width == 64): the last one to finish folds the partials
    const size_t slot = (size_t)dv.w * SMALL_W + (size_t)v * nblk;   // the segment's partials of window v: nblk neighbours
    if (gi == 0) {
        if (q4.role == 0) store_soa<A>(partial, 0, slot + j, acc);
        if (t == 0) partial_inf[slot + j] = ainf;
    }
    __threadfence();
    __syncthreads();
    if (t == 0) last_flag = atomicAdd(&count[(size_t)dv.w * SMALL_W + v], 1u) + 1u;
    __syncthreads();
    if (last_flag != nblk) return;
    __threadfence();
    ainf = true; zero(acc);
    if ((unsigned)gi < nblk) {
        ainf = partial_inf[slot + gi] != 0;
        if (!ainf) load_soa<A>(acc, partial, 0, slot + gi);
    }
    int pw = 1; while ((unsigned)pw < nblk) pw <<= 1;
    tree(acc, ainf, pw, pw);
    write_window(acc, ainf);
}

// segment g: the tail over its 64 window sums (many_kernels.hip.h many_fold_row).  One group of four members per segment: on the device the fold is one
// dependent chain of 252 doublings, so it pays when many segments fold side by side.
template <class A>
__global__ void __launch_bounds__(256 * A::LPP) k_seg_fold(const uint32_t *__restrict__ win, const uint8_t *__restrict__ win_inf, size_t nseg,
                                                            uint32_t *__restrict__ out_xyz, uint8_t *__restrict__ out_inf) {
    constexpr int GL = 4 * A::LPP;
    const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / GL;
    if (g >= nseg) return;
    many_fold_row<A>(win, win_inf, g * SMALL_W, SMALL_W, g, out_xyz, out_inf);
}

// launchers (instantiated by k_g1_seg.hip / k_g2_seg.hip; declared in msm_launch.hip.h)
template <class C> void launch_seg_tree(hipStream_t s, const uint32_t *tab, const uint8_t *tab_inf, const uint32_t *scalars, const void *desc, size_t blocks, uint32_t *partial,
                                        uint8_t *partial_inf, uint32_t *count, uint32_t *win, uint8_t *win_inf, bool abi, uint32_t *bad_flag) {
    typedef typename C::ACC A;
    hipLaunchKernelGGL((k_seg_tree<A>), dim3((unsigned)blocks, SMALL_W), dim3(256 * A::LPP), 0, s, tab, tab_inf, scalars, (const uint4 *)desc, partial, partial_inf, count, win, win_inf, abi ? 1 : 0, bad_flag);
}
template <class C> void launch_seg_fold(hipStream_t s, const uint32_t *win, const uint8_t *win_inf, size_t nseg, uint32_t *out_xyz, uint8_t *out_inf) {
    typedef typename C::ACC A;
    // 16 segments per block: the chain is latency, so a block per few segments spreads them over the chip
    hipLaunchKernelGGL((k_seg_fold<A>), dim3((unsigned)((nseg + 15) / 16)), dim3(64 * A::LPP), 0, s, win, win_inf, nseg, out_xyz, out_inf);
}

}  // namespace msm
