// crypto_amd/csrc/seg_layout.hip.h — the pieces of the segmented small MSM (seg_kernels.hip.h: many small MSMs, each over its OWN bases, in one call) that do
// not depend on the device: the geometry of one segment, the layout of a chunk of ragged segments over blocks of 64 groups with its descriptor array, and the
// per-segment tail (Horner over the 64 window sums, normalisation: many_fold.hip.h many_horner / many_normalise).  The kernels instantiate the tail with the
// signed 30-bit field on four lanes per segment (QuadLanes); the host build under FP29_CHECK (tests/native/seg_dev_host_shim.cpp) runs the same functions with
// QuadSerial and walks the same descriptors, so one host run under the bound tracker covers both.
#pragma once
#include "many_fold.hip.h"
#include <vector>

namespace bls29 {

constexpr int SEG_WIN = 64;                         // windows of the S = 1 table (small_kernels.hip.h SMALL_W): the tail's Horner runs over all of them
constexpr size_t SEG_MAX_N = 8192;                  // the small path's reach: 16 blocks of 64 groups of 8 leaves

// ---- one segment ---------------------------------------------------------------------------------------------------------------------------
// A segment of n terms has n leaves per window (leaf = term).  A group of four members sums `per_group` leaves serially (2 .. 8), the segment's groups are
// folded by a tree over `width` groups (a power of two, at least 2):
//   nblk == 1: the segment fits one block and takes `width` <= 64 of its 64 groups, at an offset that is a multiple of `width`
//   nblk  > 1: n > 512: per_group = 8, width = 64, the segment owns nblk <= 16 WHOLE blocks and the last of them to finish folds their partials
// An empty segment takes two groups whose leaves are all padding: its window sums are the identity like anybody else's.
struct SegGeom { int per_group, width; unsigned nblk; };
FD SegGeom seg_geometry(size_t n) {
    SegGeom g;
    size_t pg = (n + 63) / 64;
    pg = pg < 2 ? 2 : (pg > 8 ? 8 : pg);
    g.per_group = (int)pg;
    const size_t groups = (n + pg - 1) / pg;
    g.nblk = 1;
    if (groups <= 64) {
        int w = 2; while ((size_t)w < groups) w <<= 1;
        g.width = w;
    } else {
        g.width = 64;
        g.nblk = (unsigned)((n + 64 * pg - 1) / (64 * pg));
    }
    return g;
}
// the k-th leaf (k < per_group) of group `gs` (< width) of block j of the segment: the leaves of one step are neighbours, so neighbouring groups read
// neighbouring scalars and table rows.  Values >= n are padding (the identity).
FD uint32_t seg_leaf(int per_group, int width, unsigned j, int gs, int k) { return j * 64u * (uint32_t)per_group + (uint32_t)gs + (uint32_t)width * (uint32_t)k; }

// ---- the descriptor of one group of one block ---------------------------------------------------------------------------------------------------
// seg: the segment (index within the chunk), SEG_NONE: the group is padding.  first: the segment's first term within the chunk.  pslot: the segment's first
// partial slot (multi-block segments; its counter has the same index).  pack: n (14 bits) | per_group (4) | log2 width (3) | block j of the segment (4) | nblk - 1 (4) |
// log2 of the widest segment of the BLOCK (3: the same in all 64 descriptors of a block — the tree levels every group of the block runs).
struct SegDesc { uint32_t seg, first, pack, pslot; };
constexpr uint32_t SEG_NONE = 0xffffffffu;
FD uint32_t seg_pack(uint32_t n, int per_group, int width, unsigned j, unsigned nblk) {
    uint32_t lw = 0; while ((1 << lw) < width) lw++;
    return n | (uint32_t)per_group << 14 | lw << 18 | j << 21 | (nblk - 1) << 25;
}
FD uint32_t seg_n(uint32_t pack) { return pack & 0x3fffu; }
FD int seg_per_group(uint32_t pack) { return (int)(pack >> 14 & 15u); }
FD int seg_width(uint32_t pack) { return 1 << (pack >> 18 & 7u); }
FD unsigned seg_block(uint32_t pack) { return pack >> 21 & 15u; }
FD unsigned seg_nblk(uint32_t pack) { return (pack >> 25 & 15u) + 1u; }
FD int seg_levels(uint32_t pack) { return 1 << (pack >> 29); }
// does group `gs` of a segment `width` groups wide take part, as the receiving side, in the tree level at distance d?  Its partner gs + d is a group of the
// same segment: a fold never crosses a segment boundary.  (Levels with d >= width pair nobody of that segment: a block runs the levels of its widest one, seg_levels.)
FD bool seg_pairs(int width, int gs, int d) { return gs + d < width; }

// ---- a chunk of segments over blocks ------------------------------------------------------------------------------------------------------------
// Segments [s0, s1) of seg_end (segment g = the terms [seg_end[g - 1], seg_end[g]), seg_end[-1] = 0), every one of at most SEG_MAX_N terms, in input
// order: a single-block segment goes to the next offset of the current block that is a multiple of its width, or opens a new block when it does not fit;
// a multi-block segment opens a new block and owns nblk whole ones.  The groups skipped on the way are padding: no block is reserved for a short segment.
struct SegLayout {
    std::vector<SegDesc> desc;      // 64 per block
    size_t blocks = 0, pslots = 0;  // pslots: partial slots (= blocks of multi-block segments)
};
inline void seg_layout(const uint64_t *seg_end, size_t s0, size_t s1, SegLayout &out) {
    const uint64_t t0 = s0 ? seg_end[s0 - 1] : 0;
    const SegDesc none{SEG_NONE, 0, seg_pack(0, 2, 2, 0, 1), 0};
    out.desc.clear(); out.blocks = 0; out.pslots = 0;
    size_t cursor = 64;                                             // next free group of the last block (64: open a new one)
    auto new_block = [&]() { out.desc.resize((out.blocks + 1) * 64, none); out.blocks++; cursor = 0; };
    for (size_t s = s0; s < s1; s++) {
        const uint64_t lo = s ? seg_end[s - 1] : 0;
        const uint32_t n = (uint32_t)(seg_end[s] - lo), first = (uint32_t)(lo - t0);
        const SegGeom g = seg_geometry(n);
        if (g.nblk > 1) {
            for (unsigned j = 0; j < g.nblk; j++) {
                new_block();
                SegDesc *d = &out.desc[(out.blocks - 1) * 64];
                for (int gi = 0; gi < 64; gi++) d[gi] = SegDesc{(uint32_t)(s - s0), first, seg_pack(n, g.per_group, 64, j, g.nblk), (uint32_t)out.pslots};
            }
            out.pslots += g.nblk;
            cursor = 64;
            continue;
        }
        size_t pos = (cursor + g.width - 1) & ~(size_t)(g.width - 1);
        if (pos + g.width > 64) { new_block(); pos = 0; }
        SegDesc *d = &out.desc[(out.blocks - 1) * 64 + pos];
        for (int gi = 0; gi < g.width; gi++) d[gi] = SegDesc{(uint32_t)(s - s0), first, seg_pack(n, g.per_group, g.width, 0, 1), 0};
        cursor = pos + g.width;
    }
    for (size_t b = 0; b < out.blocks; b++) {                         // the block's widest segment, into every descriptor of the block
        SegDesc *d = &out.desc[b * 64];
        uint32_t lw = 1;
        for (int gi = 0; gi < 64; gi++) if (d[gi].seg != SEG_NONE) lw = lw > (d[gi].pack >> 18 & 7u) ? lw : (d[gi].pack >> 18 & 7u);
        for (int gi = 0; gi < 64; gi++) d[gi].pack |= lw << 29;
    }
}

// ---- the tail of a segment ------------------------------------------------------------------------------------------------------------------------
// many_fold.hip.h many_tail over SEG_WIN window sums: 252 doublings in one dependent chain and one inversion per segment.

}  // namespace bls29
