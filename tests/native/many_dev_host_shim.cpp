// tests/native/many_dev_host_shim.cpp — the device code of the many-row small MSM that does not depend on the device (crypto_amd/csrc/many_fold.hip.h:
// the launch geometry with its row packing, the Horner step, the inversion and the normalisation) compiled for the host with the FP29_CHECK worst-case bound
// tracker.  The kernels run the same functions with four lanes per row (QuadLanes) where this build uses QuadSerial: same field operations on the same value
// classes, so every assertion that could fire for SOME input of those classes fires here.
#define FP29_CHECK 1
#include "../../crypto_amd/csrc/many_fold.hip.h"
#include <vector>
#include <string.h>
using namespace bls29;

static void load1(Xyzz<Fs> &p, const uint32_t *w) { fs_from_abi(p.x, w); fs_from_abi(p.y, w + 12); fs_from_abi(p.zz, w + 24); fs_from_abi(p.zzz, w + 36); }
static void load2(Xyzz<Fs2> &p, const uint32_t *w) {
    fs_from_abi(p.x.c0, w); fs_from_abi(p.x.c1, w + 12); fs_from_abi(p.y.c0, w + 24); fs_from_abi(p.y.c1, w + 36);
    fs_from_abi(p.zz.c0, w + 48); fs_from_abi(p.zz.c1, w + 60); fs_from_abi(p.zzz.c0, w + 72); fs_from_abi(p.zzz.c1, w + 84);
}
static void aff1(Xyzz<Fs> &p, const uint32_t *w) { fs_from_abi(p.x, w); fs_from_abi(p.y, w + 12); fset_one(p.zz); fset_one(p.zzz); }
static void aff2(Xyzz<Fs2> &p, const uint32_t *w) { fs_from_abi(p.x.c0, w); fs_from_abi(p.x.c1, w + 12); fs_from_abi(p.y.c0, w + 24); fs_from_abi(p.y.c1, w + 36); fset_one(p.zz); fset_one(p.zzz); }
static void store1(uint32_t *o, const Fs &a) { fs_to_abi(o, a); }
static void store1(uint32_t *o, const Fs2 &a) { fs_to_abi(o, a.c0); fs_to_abi(o + 12, a.c1); }
template <class F> static void zero_pt(Xyzz<F> &p) { fzero(p.x); fzero(p.y); fzero(p.zz); fzero(p.zzz); }

// what k_many_fold does for one row: Horner over the 16 window sums (XYZZ in ABI words, identity flags), normalisation, the ABI's representative
template <class F, int FW, class Load>
static int fold_row(const uint32_t *win, const uint8_t *win_inf, uint32_t *out, Load load) {
    QuadSerial q4;
    Xyzz<F> acc, s; bool ainf = true;
    zero_pt(acc);
    for (int v = MANY_WIN - 1; v >= 0; v--) {
        const bool sinf = win_inf[v] != 0;
        zero_pt(s);
        if (!sinf) load(s, win + (size_t)v * 4 * FW);
        many_horner_step(acc, ainf, s, sinf, v == MANY_WIN - 1, q4);
    }
    F ox, oy, oz;
    if (ainf) { fset_one(ox); fset_one(oy); fzero(oz); }
    else { many_normalise(ox, oy, acc); fset_one(oz); }
    store1(out, ox); store1(out + FW, oy); store1(out + 2 * FW, oz);
    return ainf ? 1 : 0;
}

// what a block of k_many_tree does for one super-window: 64 groups, `rows` rows packed as segments (many_geometry), group gs of a segment sums its
// per_group leaves (many_leaf), the tree levels pair groups of one segment only (many_pairs); several blocks per row: their partials through the same
// tree.  leaves: rows x L affine points (all-zero words: the identity).  out: rows XYZZ sums; returns the number of leaves read (each exactly once).
template <class F, int FW, class Aff_, class Store>
static long tree_rows(const uint32_t *leaves, size_t n, size_t rows, uint32_t *out, uint8_t *out_inf, Aff_ aff, Store store) {
    const ManyGeom g = many_geometry(n);
    const size_t L = n * MANY_SUB;
    QuadSerial q4;
    long reads = 0;
    std::vector<uint8_t> seen(rows * L, 0);
    auto leaf = [&](Xyzz<F> &p, bool &pinf, size_t row, size_t l) {
        pinf = true; zero_pt(p);
        if (row >= rows || l >= L) return;
        reads++; seen[row * L + l]++;
        const uint32_t *w = leaves + (row * L + l) * 2 * FW;
        uint32_t any = 0; for (int k = 0; k < 2 * FW; k++) any |= w[k];
        if (!any) return;
        aff(p, w); pinf = false;
    };
    auto tree = [&](std::vector<Xyzz<F>> &a, std::vector<char> &f, int width) {
        for (int d = width >> 1; d >= 1; d >>= 1) {
            std::vector<Xyzz<F>> o(a); std::vector<char> of(f);           // (every group reads what its partner held BEFORE the level: the LDS exchange)
            for (int gi = 0; gi < 64; gi++) {
                Xyzz<F> x = o[gi]; bool xinf = true;
                if (many_pairs(width, gi & (width - 1), d)) { x = o[gi + d]; xinf = of[gi + d] != 0; }
                bool ai = f[gi] != 0; xyzz_add_rounds(a[gi], ai, x, xinf, q4); f[gi] = ai;
            }
        }
    };
    const size_t zb = (rows + g.rows_per_block - 1) / g.rows_per_block;
    for (size_t z = 0; z < zb; z++) {
        std::vector<std::vector<Xyzz<F>>> part(g.nblk);
        std::vector<std::vector<char>> pf(g.nblk);
        for (unsigned j = 0; j < g.nblk; j++) {
            std::vector<Xyzz<F>> acc(64); std::vector<char> inf(64);
            for (int gi = 0; gi < 64; gi++) {
                const int gs = gi & (g.seg - 1); const size_t row = z * g.rows_per_block + gi / g.seg;
                bool ai; leaf(acc[gi], ai, row, many_leaf(g, j, gs, 0));
                for (int k = 1; k < g.per_group; k++) { Xyzz<F> o; bool oi; leaf(o, oi, row, many_leaf(g, j, gs, k)); xyzz_add_rounds(acc[gi], ai, o, oi, q4); }
                inf[gi] = ai;
            }
            tree(acc, inf, g.seg);
            part[j] = acc; pf[j] = inf;
        }
        std::vector<Xyzz<F>> fin = part[0]; std::vector<char> ff = pf[0];
        if (g.nblk > 1) {                                               // seg == 64, one row per block: group gi takes block gi's partial
            for (int gi = 0; gi < 64; gi++) { if ((unsigned)gi < g.nblk) { fin[gi] = part[gi][0]; ff[gi] = pf[gi][0]; } else { zero_pt(fin[gi]); ff[gi] = 1; } }
            int width = 1; while ((unsigned)width < g.nblk) width <<= 1;
            tree(fin, ff, width);
        }
        for (int r = 0; r < g.rows_per_block; r++) {
            const size_t row = z * g.rows_per_block + r;
            if (row >= rows) continue;
            const int gi = r * g.seg;
            out_inf[row] = ff[gi] != 0;
            if (!ff[gi]) store(out + row * 4 * FW, fin[gi]); else memset(out + row * 4 * FW, 0, 16 * FW);
        }
    }
    for (uint8_t c : seen) if (c != 1) return -1;
    return reads;
}
static void st1(uint32_t *o, const Xyzz<Fs> &a) { fs_to_abi(o, a.x); fs_to_abi(o + 12, a.y); fs_to_abi(o + 24, a.zz); fs_to_abi(o + 36, a.zzz); }
static void st2(uint32_t *o, const Xyzz<Fs2> &a) { store1(o, a.x); store1(o + 24, a.y); store1(o + 48, a.zz); store1(o + 72, a.zzz); }

extern "C" {
int shim_many_fold_g1(const uint32_t *win, const uint8_t *win_inf, uint32_t *out) { return fold_row<Fs, 12>(win, win_inf, out, load1); }
int shim_many_fold_g2(const uint32_t *win, const uint8_t *win_inf, uint32_t *out) { return fold_row<Fs2, 24>(win, win_inf, out, load2); }
long shim_many_tree_g1(const uint32_t *leaves, size_t n, size_t rows, uint32_t *out, uint8_t *out_inf) { return tree_rows<Fs, 12>(leaves, n, rows, out, out_inf, aff1, st1); }
long shim_many_tree_g2(const uint32_t *leaves, size_t n, size_t rows, uint32_t *out, uint8_t *out_inf) { return tree_rows<Fs2, 24>(leaves, n, rows, out, out_inf, aff2, st2); }
void shim_many_geometry(size_t n, int *out) { const ManyGeom g = many_geometry(n); out[0] = g.per_group; out[1] = g.seg; out[2] = g.rows_per_block; out[3] = (int)g.nblk; }
void shim_many_inv_g2(const uint32_t *a, uint32_t *out) { Fs2 x, r; fs_from_abi(x.c0, a); fs_from_abi(x.c1, a + 12); finv(r, x); store1(out, r); }
}
