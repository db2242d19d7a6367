// crypto_amd/csrc/many_fold.hip.h — the pieces of the many-row small MSM (many_kernels.hip.h) that do not depend on the device: the launch geometry
// with its row packing, and the per-row tail (Horner over the 16 super-window sums, normalisation to the ABI's representative) written over the
// field F and the product policy Q4 of ec29.hip.h.  The kernels instantiate it with the signed 30-bit field on four lanes per row (QuadLanes); the host
// build under FP29_CHECK (tests/native/many_dev_host_shim.cpp) with the same field and QuadSerial — same field operations on the same value classes, so one
// host run under the bound tracker covers both.
#pragma once
#include "ec29.hip.h"
#include "fp30s.hip.h"
#include "fs2_pair.hip.h"
#include "fp_safegcd.hip.h"

namespace bls29 {

// ---- geometry ------------------------------------------------------------------------------------------------------------------------------
// A row of n terms has L = 4 n leaves per super-window (leaf l = (sub-table l / n, term l mod n): small_kernels.hip.h).  A block is 64 groups of four
// members; a group sums `per_group` leaves (2 .. 8: with many rows in flight the chip is full, so the serial leaves of a group cost nothing the tree
// levels they replace would not) and the groups of a row are folded by a tree.
//   nblk > 1 : the row needs several blocks per super-window (seg = 64, one row per block); the last block to finish folds the partials
//   nblk == 1: the row needs g = ceil(L / per_group) <= 64 groups.  Rows of 4 .. 30 terms would leave most of a block idle, so the block is cut into
//              SEGMENTS of seg = g rounded up to a power of two groups and holds 64 / seg rows: group gi belongs to row gi / seg of the block and is
//              group gi % seg of that row, and a tree level at distance d only pairs groups of one segment (many_pairs).
struct ManyGeom { int per_group, seg, rows_per_block; unsigned nblk; };
constexpr int MANY_SUB = 4, MANY_WIN = 16;          // sub-tables of the resident table, super-windows (small_kernels.hip.h SMALL_S, SMALL_W / SMALL_S)
constexpr size_t MANY_MAX_N = 8192;                 // the small path's reach: 4 * 8192 leaves = 64 blocks of 64 groups of 8
FD ManyGeom many_geometry(size_t n) {
    ManyGeom g;
    const size_t L = n * MANY_SUB;
    size_t pg = (L + 63) / 64;
    pg = pg < 2 ? 2 : (pg > 8 ? 8 : pg);
    g.per_group = (int)pg;
    g.nblk = (unsigned)((L + 64 * pg - 1) / (64 * pg));
    g.seg = 64;
    if (g.nblk <= 1) {
        g.nblk = 1;
        const size_t groups = (L + pg - 1) / pg;
        int s = 1; while ((size_t)s < groups) s <<= 1;
        g.seg = s < 2 ? 2 : s;
    }
    g.rows_per_block = 64 / g.seg;
    return g;
}
// the k-th leaf (k < per_group) of group `gs` of its segment, in block j of the row: the leaves of one step are neighbours, so neighbouring groups
// read neighbouring scalars and table rows.  Values >= L are padding (the identity).
FD size_t many_leaf(const ManyGeom &g, unsigned j, int gs, int k) { return (size_t)j * 64 * g.per_group + (size_t)gs + (size_t)g.seg * k; }
// does group `gs` of a segment take part, as the receiving side, in the tree level at distance d (d = seg / 2 .. 1)?  Its partner gs + d is in the same
// segment: a fold never crosses the row boundary
FD bool many_pairs(int seg, int gs, int d) { return gs + d < seg; }

// ---- 1 / a -----------------------------------------------------------------------------------------------------------------------------------
// The division-step inversion is written for the 14 x 29-bit field: across and back (fp30s.hip.h).  a: class B.
FD void finv(Fs &r, const Fs &a) { Fp z, i; fp_from_fs(z, a); fp_inv_safegcd(i, z); fs_from_fp(r, i); }
// (a0 + a1 u)^-1 = (a0 - a1 u) / (a0^2 + a1^2)
FD void finv(Fs2 &r, const Fs2 &a) {
    Fs s0, s1, n, nb, ni, t;
    fs_sqr(s0, a.c0); fs_sqr(s1, a.c1);
    fs_add(n, s0, s1); fs_bal(nb, n);
    finv(ni, nb);
    fs_mul(r.c0, a.c0, ni);
    fs_mul(t, a.c1, ni); fs_neg(r.c1, t);
}
#if defined(__HIPCC__)
// the same on a lane pair: each lane squares its half, the norm is the sum of both, both lanes invert it (one chain either way)
__device__ __forceinline__ void finv(Fs2H &r, const Fs2H &a) {
    Fs s, so, n, nb, ni, t;
    fs_sqr(s, a.v); xchg(so, s);
    fs_add(n, s, so); fs_bal(nb, n);
    finv(ni, nb);
    fs_mul(t, a.v, ni);
    fs_cond_neg(r.v, t, spair_odd());
}
#endif

// ---- the tail of a row --------------------------------------------------------------------------------------------------------------------------
// One Horner step: acc <- 16 acc + S (four doublings between super-windows; none in front of the top one).  The doublings are xyzz_dbl_rounds, whose limb
// bounds close over a chain (k_small_subtable runs 192 of them in a row); on an identity accumulator they work on whatever the coordinates hold and the
// flag says so — xyzz_add_rounds then takes the addend.  Both curves have odd order: the double of a point is never the identity.
template <class F, class Q4> FD void many_horner_step(Xyzz<F> &acc, bool &ainf, const Xyzz<F> &s, bool sinf, bool top, const Q4 &q4) {
    if (!top) {
        Xyzz<F> d;
        xyzz_dbl_rounds(d, acc, q4); xyzz_dbl_rounds(acc, d, q4);
        xyzz_dbl_rounds(d, acc, q4); xyzz_dbl_rounds(acc, d, q4);
    }
    xyzz_add_rounds(acc, ainf, s, sinf, q4);
}
// Horner over `nwin` window sums, the most significant first: acc = sum_v 16^v S_v.  load(s, v) fills s with S_v and returns its identity flag (the
// coordinates of an identity are never read: leave them zero).  The many-row fold runs it over 16 super-windows, the segmented one (seg_layout.hip.h) over 64.
template <class F, class Q4, class L> FD void many_horner(Xyzz<F> &acc, bool &ainf, int nwin, const L &load, const Q4 &q4) {
    ainf = true;
    fzero(acc.x); fzero(acc.y); fzero(acc.zz); fzero(acc.zzz);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int v = nwin - 1; v >= 0; v--) {
        Xyzz<F> s;
        const bool sinf = load(s, v);
        many_horner_step(acc, ainf, s, sinf, v == nwin - 1, q4);
    }
}
// (X / ZZ, Y / ZZZ) with 1 / ZZ = (ZZ / ZZZ)^2: the affine coordinates, i.e. the Jacobian representative with Z = 1 the ABI returns
// (host_field.hpp to_normalised_jacobian).  acc is not the identity.
template <class F> FD void many_normalise(F &x, F &y, const Xyzz<F> &acc) {
    F z3, i3, z2, t, i2, xn, yn;
    fnorm(z3, acc.zzz); finv(i3, z3);
    fnorm(z2, acc.zz); fmul(t, z2, i3); fsqr(i2, t);
    fnorm(xn, acc.x); fnorm(yn, acc.y);
    fmul(x, xn, i2); fmul(y, yn, i3);
}

// the whole tail: (ox, oy, oz) = the ABI's representative of sum_v 16^v S_v over nwin window sums: (X, Y, 1) normalised; (1, 1, 0) and ainf for the identity
template <class F, class Q4, class L> FD void many_tail(F &ox, F &oy, F &oz, bool &ainf, int nwin, const L &load, const Q4 &q4) {
    Xyzz<F> acc;
    many_horner(acc, ainf, nwin, load, q4);
    if (ainf) { fset_one(ox); fset_one(oy); fzero(oz); }
    else { many_normalise(ox, oy, acc); fset_one(oz); }
}

}  // namespace bls29
