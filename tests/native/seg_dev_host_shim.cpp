// tests/native/seg_dev_host_shim.cpp — the device code of the segmented small MSM that does not depend on the device (crypto_amd/csrc/seg_layout.hip.h: the
// geometry of a segment, the layout of a ragged batch over blocks with its descriptors; many_fold.hip.h: the Horner fold over a window count, the inversion,
// the normalisation) compiled for the host with the FP29_CHECK worst-case bound tracker.  k_seg_fold runs many_tail with four lanes per segment (QuadLanes)
// where this build uses QuadSerial: same field operations on the same value classes.  walk() does with the descriptors exactly what k_seg_tree does with
// them — the same accessors, the same leaf and pairing functions, the same block-wide level count — on integers instead of points.
#define FP29_CHECK 1
#include "../../crypto_amd/csrc/seg_layout.hip.h"
#include <vector>
#include <string.h>
using namespace bls29;

static void load1(Xyzz<Fs> &p, const uint32_t *w) { fs_from_abi(p.x, w); fs_from_abi(p.y, w + 12); fs_from_abi(p.zz, w + 24); fs_from_abi(p.zzz, w + 36); }
static void load2(Xyzz<Fs2> &p, const uint32_t *w) {
    fs_from_abi(p.x.c0, w); fs_from_abi(p.x.c1, w + 12); fs_from_abi(p.y.c0, w + 24); fs_from_abi(p.y.c1, w + 36);
    fs_from_abi(p.zz.c0, w + 48); fs_from_abi(p.zz.c1, w + 60); fs_from_abi(p.zzz.c0, w + 72); fs_from_abi(p.zzz.c1, w + 84);
}
static void store1(uint32_t *o, const Fs &a) { fs_to_abi(o, a); }
static void store1(uint32_t *o, const Fs2 &a) { fs_to_abi(o, a.c0); fs_to_abi(o + 12, a.c1); }

// what k_seg_fold does for one segment: the tail over the 64 window sums (XYZZ in ABI words, identity flags)
template <class F, int FW, class Load>
static int fold_segment(const uint32_t *win, const uint8_t *win_inf, uint32_t *out, Load load) {
    QuadSerial q4;
    F ox, oy, oz; bool ainf;
    many_tail(ox, oy, oz, ainf, SEG_WIN, [&](Xyzz<F> &s, int v) {
        const bool sinf = win_inf[v] != 0;
        fzero(s.x); fzero(s.y); fzero(s.zz); fzero(s.zzz);
        if (!sinf) load(s, win + (size_t)v * 4 * FW);
        return sinf;
    }, q4);
    store1(out, ox); store1(out + FW, oy); store1(out + 2 * FW, oz);
    return ainf ? 1 : 0;
}

// k_seg_tree over segments [s0, s1) with the group sums as wrapping 64-bit integers: val[t] is term t's contribution.  sums[g] receives segment g's window
// sum.  Returns 0, or which property failed: 1 a term read twice or by a foreign segment, 2 a term never read, 3 a tree level pairs groups of two segments or
// leaves the block, 4 a width that is no power of two in 2 .. 64 or an offset that is no multiple of it, 5 a multi-block segment that does not own whole
// blocks in a row, 6 a segment without a first group or with two, 7 descriptor fields that disagree with the segment.
static int walk(const uint64_t *seg_end, size_t s0, size_t s1, const uint64_t *val, uint64_t *sums) {
    SegLayout lay;
    seg_layout(seg_end, s0, s1, lay);
    const uint64_t t0 = s0 ? seg_end[s0 - 1] : 0, T = seg_end[s1 - 1] - t0;
    const size_t ns = s1 - s0;
    if (lay.desc.size() != lay.blocks * 64) return 7;
    std::vector<uint8_t> seen(T, 0), written(ns, 0);
    std::vector<uint64_t> partial(lay.pslots, 0);
    std::vector<unsigned> done(lay.pslots, 0);
    auto tree = [&](uint64_t *a, const SegDesc *d, const int *w, int levels) -> int {
        for (int dist = levels >> 1; dist >= 1; dist >>= 1) {
            uint64_t o[64]; memcpy(o, a, sizeof o);                 // (every group reads what its partner held BEFORE the level: the LDS exchange)
            for (int gi = 0; gi < 64; gi++) {
                if (!seg_pairs(w[gi], gi & (w[gi] - 1), dist)) continue;
                if (gi + dist >= 64 || (d && d[gi + dist].seg != d[gi].seg)) return 3;
                a[gi] += o[gi + dist];
            }
        }
        return 0;
    };
    for (size_t b = 0; b < lay.blocks; b++) {
        const SegDesc *d = &lay.desc[b * 64];
        uint64_t acc[64]; int w[64]; int wor = 0;
        for (int gi = 0; gi < 64; gi++) {
            const uint32_t pack = d[gi].pack, n = seg_n(pack);
            const int width = seg_width(pack), pg = seg_per_group(pack), gs = gi & (width - 1);
            const unsigned j = seg_block(pack), nblk = seg_nblk(pack);
            w[gi] = width; wor |= width;
            acc[gi] = 0;
            if (width < 2 || width > 64 || (width & (width - 1))) return 4;
            if (d[gi].seg == SEG_NONE) continue;
            if (d[gi].seg >= ns) return 7;
            const size_t s = s0 + d[gi].seg;
            const uint64_t lo = s ? seg_end[s - 1] : 0;
            if (n != seg_end[s] - lo || d[gi].first != lo - t0 || pg < 2 || pg > 8 || j >= nblk) return 7;
            // the segment's groups are `width` neighbours starting at a multiple of width: all of them carry this segment
            const int base = gi - gs;
            for (int k = 0; k < width; k++) if (d[base + k].seg != d[gi].seg || d[base + k].pack != pack) return 4;
            if (nblk > 1) {
                if (width != 64 || b < j || b - j + nblk > lay.blocks) return 5;
                for (unsigned k = 0; k < nblk; k++) {
                    const SegDesc &o = lay.desc[(b - j + k) * 64 + gi];
                    if (o.seg != d[gi].seg || seg_block(o.pack) != k || o.pslot != d[gi].pslot || d[gi].pslot + nblk > lay.pslots) return 5;
                }
            }
            for (int k = 0; k < pg; k++) {
                const uint32_t l = seg_leaf(pg, width, j, gs, k);
                if (l >= n) continue;
                if (seen[d[gi].first + l]++) return 1;
                acc[gi] += val[t0 + d[gi].first + l];
            }
        }
        int widest = 1; while (widest * 2 <= wor) widest *= 2;      // the highest bit of the OR of the widths
        const int levels = seg_levels(d[0].pack);                   // what the kernel runs: the same in every descriptor of the block, and no more than the widest segment needs
        for (int gi = 0; gi < 64; gi++) if (seg_levels(d[gi].pack) != levels) return 4;
        bool any = false; for (int gi = 0; gi < 64; gi++) any |= d[gi].seg != SEG_NONE;
        if (!any || levels > widest) return 4;
        { int need = 2; for (int gi = 0; gi < 64; gi++) if (d[gi].seg != SEG_NONE && w[gi] > need) need = w[gi]; if (levels != need) return 4; }
        if (int e = tree(acc, d, w, levels)) return e;
        for (int gi = 0; gi < 64; gi++) {
            if (d[gi].seg == SEG_NONE || (gi & (w[gi] - 1)) != 0) continue;
            const unsigned nblk = seg_nblk(d[gi].pack);
            if (nblk == 1) { if (written[d[gi].seg]++) return 6; sums[s0 + d[gi].seg] = acc[gi]; continue; }
            if (gi != 0) continue;
            partial[d[gi].pslot + seg_block(d[gi].pack)] = acc[0];
            if (++done[d[gi].pslot] != nblk) continue;
            uint64_t fin[64]; int pw[64]; int p2 = 1; while ((unsigned)p2 < nblk) p2 <<= 1;
            for (int k = 0; k < 64; k++) { fin[k] = (unsigned)k < nblk ? partial[d[gi].pslot + k] : 0; pw[k] = p2; }
            if (int e = tree(fin, nullptr, pw, p2)) return e;
            if (written[d[gi].seg]++) return 6;
            sums[s0 + d[gi].seg] = fin[0];
        }
    }
    for (uint64_t t = 0; t < T; t++) if (seen[t] != 1) return 2;
    for (size_t g = 0; g < ns; g++) if (written[g] != 1) return 6;
    return 0;
}

extern "C" {
int shim_seg_fold_g1(const uint32_t *win, const uint8_t *win_inf, uint32_t *out) { return fold_segment<Fs, 12>(win, win_inf, out, load1); }
int shim_seg_fold_g2(const uint32_t *win, const uint8_t *win_inf, uint32_t *out) { return fold_segment<Fs2, 24>(win, win_inf, out, load2); }
void shim_seg_geometry(size_t n, int *out) { const SegGeom g = seg_geometry(n); out[0] = g.per_group; out[1] = g.width; out[2] = (int)g.nblk; }
int shim_seg_walk(const uint64_t *seg_end, size_t s0, size_t s1, const uint64_t *val, uint64_t *sums) { return walk(seg_end, s0, s1, val, sums); }
// the descriptors of segments [s0, s1): 4 words per group, 64 groups per block -> the number of blocks (the array is cut at cap_blocks); *pslots
size_t shim_seg_layout(const uint64_t *seg_end, size_t s0, size_t s1, uint32_t *desc, size_t cap_blocks, size_t *pslots) {
    SegLayout lay;
    seg_layout(seg_end, s0, s1, lay);
    const size_t nb = lay.blocks < cap_blocks ? lay.blocks : cap_blocks;
    if (nb) memcpy(desc, lay.desc.data(), nb * 64 * sizeof(SegDesc));
    *pslots = lay.pslots;
    return lay.blocks;
}
}
