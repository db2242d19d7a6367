// crypto_amd/csrc/acc_gt_kernels.hip.h — the scalar, staging and verdict half of verifying the accumulator proofs with a GT commitment in bulk on gfx950
// (dock_acc_gt.hip drives it).
//
// Device side of MembershipProof::verify and NonMembershipProof::verify of vb_accumulator/src/proofs.rs (verify_schnorr_proofs :890-940,
// get_g1_for_pairing_checks :942-996, verify_proof :697-724, the non-membership front :1516-1580) for many proofs against ONE accumulator value V and one
// key (pk = Q~, P~; the proving key X, Y, Z [, K]; params.P for non-membership).
//   points     E_C, T_sigma, T_rho, R_sigma, R_rho, R_delta_sigma, R_delta_rho [, E_d, E_d_inv, R_A, R_B]          7 (11) a proof, and its GT element R_E
//   responses  s_sigma, s_rho, s_delta_sigma, s_delta_rho, s_y [, s_u, s_v, s_w]                                    5 (8) a proof
//   the reference's checks in its order (c: the proof's challenge); every one is a segment of the segmented small MSM whose sum must be the identity, the last
//   two segments of a row are the two sides of its pairing:
//     non-membership only   [P, K, E_d, R_A] . (s_u, s_v, -c, -1)                            [K, E_d_inv, P, R_B] . (s_w, s_u, -c, -1)
//     both                  [X, T_sigma, R_sigma] . (s_sigma, -c, -1)                        [Y, T_rho, R_rho] . (s_rho, -c, -1)
//                           [T_sigma, X, R_delta_sigma] . (s_y, -s_delta_sigma, -1)          [T_rho, Y, R_delta_rho] . (s_y, -s_delta_rho, -1)
//     p (against P~)        [E_C, Z, V] . (s_y, -(s_delta_sigma + s_delta_rho), -c)          non-membership: [E_C, Z, V, E_d, K] . (.., c, -s_v)
//     q (against pk)        [Z, E_C] . (-(s_sigma + s_rho), c)
//   and e(p, P~) e(q, pk) = R_E.
// The scalar field has to
//   write the own scalars where the segmented small MSM reads them                                                                     k_acc_gt_own
//   one verdict: the coefficients of the shared points (in the one G1 equation: X, Y [, P, K]; in the two sides: Z, V [, K] and Z) and the weights over the
//   proofs' own points — check j of proof i weighs rho^(J i + j), J = 4 (6); the pairing and R_E of proof i weigh t_i = rho^i       k_acc_gt_col_sums, k_col_finish
// and three kernels move words only: k_acc_gt_stage lays the points out for the segment MSM, k_acc_gt_sides turns the last two sums of a row into the sides of
// its pairing, k_acc_gt_verdict folds a row's checks — the identity flags of its Schnorr sums, its pairing value against its own R_E — into its status byte.
// The per-lane routines are FRD functions over load / store functors, as acc_pok_kernels.hip.h's are: the same text runs on the host under -DFP29_CHECK
// (tests/native/acc_gt_dev_host_shim.cpp).  Operand classes as in col_sums.hip.h.
//
// Bounds of the batch sums.  A row adds at most TWO products to a lane's sum, each with a carry pass: a run of COL_RUN = 16 rows is at most
// 32 terms, value < 64 r, limbs <= 2^29 + 1.  The fixed tree of a block of 256 adds sums of equal depth: a slot holds at most 256 x 32 products, value
// < 2^14 r — a first operand of fr_mul (limbs < 2^31, value x 2 r far below 2^34 r^2).  The sum of two responses is one addition and one carry pass: value
// < 4 r, limbs <= 2^29 + 1 — either operand of a product, and what neg_product's subtraction takes (512 r - v).
#pragma once
#include "col_sums.hip.h"

namespace accgt {
using namespace fr29;
using colk::neg_product;
using colk::pow_start;

constexpr int FQW = 12;           // u32 words of a base-field element
constexpr int GTW = 144;          // u32 words of a GT element of the ABI
constexpr int MEMBERSHIP = 0, NON_MEMBERSHIP = 1;
// the shape of a proof kind: points and responses per proof, own scalars (= bases of its segments) per row, segments per row (the last two: p and q), Schnorr
// checks J, columns of the batch (`g1cols` of them close the G1 equation, `pcols` the side against P~, one the side against pk)
struct Shape { int pts, resp, own, segs, checks, g1cols, pcols; };
FRD Shape shape_of(int kind) { return kind == MEMBERSHIP ? Shape{7, 5, 17, 6, 4, 2, 2} : Shape{11, 8, 27, 8, 6, 4, 3}; }
FRD int cols_of(int kind) { const Shape s = shape_of(kind); return s.g1cols + s.pcols + 1; }
constexpr int MAX_OWN = 27, MAX_PTS = 11, MAX_SEGS = 8, MAX_COLS = 8;
// the shared points as the stage kernel is handed them
constexpr int SH_V = 0, SH_X = 1, SH_Y = 2, SH_Z = 3, SH_K = 4, SH_P = 5, N_SHARED = 6;
// the responses
constexpr int RS_SIGMA = 0, RS_RHO = 1, RS_DSIGMA = 2, RS_DRHO = 3, RS_Y = 4, RS_U = 5, RS_V = 6, RS_W = 7;

// the end of segment g of a row, in own scalars: membership 3, 3, 3, 3, 3, 2 terms; non-membership 4, 4, 3, 3, 3, 3, 5, 2
FRD unsigned seg_end(int kind, unsigned g) {
    return (unsigned)((kind == MEMBERSHIP ? 0x110F0C090603ull : 0x1B1914110E0B0804ull) >> (8 * g)) & 255u;
}
// own scalar t of a row as a code: bits 0..3 the source (0 .. 7 a response, 8 the challenge, 9 one, 10 s_delta_sigma + s_delta_rho, 11 s_sigma + s_rho),
// bit 4: negated
FRD unsigned own_code(int kind, unsigned t) {
    constexpr uint8_t FOUR[12] = {0, 0x18, 0x19, 1, 0x18, 0x19, 4, 0x12, 0x19, 4, 0x13, 0x19};
    if (kind == MEMBERSHIP) {
        constexpr uint8_t TAIL[5] = {4, 0x1A, 0x18, 0x1B, 8};
        return t < 12 ? FOUR[t] : TAIL[t - 12];
    }
    constexpr uint8_t HEAD[8] = {5, 6, 0x18, 0x19, 7, 5, 0x18, 0x19};
    constexpr uint8_t TAIL[7] = {4, 0x1A, 0x18, 8, 0x16, 0x1B, 8};
    return t < 8 ? HEAD[t] : t < 20 ? FOUR[t - 8] : TAIL[t - 20];
}
// where base t of a row comes from: 0 .. 10 a point of the proof, 16 + k the shared point k
FRD unsigned stage_src(int kind, unsigned t) {
    constexpr uint8_t FOUR[12] = {16 + SH_X, 1, 3, 16 + SH_Y, 2, 4, 1, 16 + SH_X, 5, 2, 16 + SH_Y, 6};
    if (kind == MEMBERSHIP) {
        constexpr uint8_t TAIL[5] = {0, 16 + SH_Z, 16 + SH_V, 16 + SH_Z, 0};
        return t < 12 ? FOUR[t] : TAIL[t - 12];
    }
    constexpr uint8_t HEAD[8] = {16 + SH_P, 16 + SH_K, 7, 9, 16 + SH_K, 8, 16 + SH_P, 10};
    constexpr uint8_t TAIL[7] = {0, 16 + SH_Z, 16 + SH_V, 7, 16 + SH_K, 16 + SH_Z, 0};
    return t < 8 ? HEAD[t] : t < 20 ? FOUR[t - 8] : TAIL[t - 20];
}

// o = a + b after one carry pass.  a, b: products
FRD void sum2(Fr &o, const Fr &a, const Fr &b) { fr_add(o, a, b); fr_norm(o, o); }
// sum += a b, one carry pass.  a: a product or a sum2; b: a product
FRD void add_product(Fr &sum, const Fr &a, const Fr &b) {
    Fr p; fr_mul(p, a, b);                            // 4 r * 2 r
    fr_add(sum, sum, p); fr_norm(sum, sum);
}
// own scalar t of row i (own_code).  chal(i, Fr &) and resp(i, q, Fr &) load products
template <class Cc, class Rs> FRD void own_scalar(Fr &o, int kind, size_t i, unsigned t, Cc chal, Rs resp) {
    const unsigned code = own_code(kind, t), src = code & 15u;
    Fr v, w;
    if (src < 8) resp(i, src, v);
    else if (src == 8) chal(i, v);
    else if (src == 9) fr_one(v);
    else { resp(i, src == 10 ? RS_DSIGMA : RS_SIGMA, v); resp(i, src == 10 ? RS_DRHO : RS_RHO, w); sum2(v, v, w); }
    if (code & 16u) neg_product(o, v);
    else { Fr one; fr_one(one); fr_mul(o, v, one); }  // (a sum of two leaves as a product)
}

// The weights of one row of a batch: w[j] = rho^(J i + j) on Schnorr check j, nw[j] = -w[j], t = rho^i on the pairing and R_E
struct RowWeights { Fr w[6], nw[6], t; };
// One lane's run of a column of the batch: rows j < cnt of the run see the weights of row e0 + j.  term(j, W, sum) adds the column's products of that row to
// the lazy sum; weights(j, W) is called for the lanes of column 0 (with_weights).  The sum leaves reduced to a product.  rho: a product, so is everything
// derived from it.
template <class T, class Wt> FRD void col_run(int kind, const Fr &rho, size_t e0, size_t cnt, bool with_weights, T term, Wt weights, Fr &sum) {
    const int J = shape_of(kind).checks;
    Fr rho_j, base;
    RowWeights W;
    pow_start(rho_j, rho, (size_t)J);
    pow_start(base, rho_j, e0);                       // rho^(J e0)
    pow_start(W.t, rho, e0);
    fr_zero(sum);
    for (size_t j = 0; j < cnt; j++) {
        W.w[0] = base;
        // (unrolled: the weights are registers, not an indexed array in scratch)
#pragma unroll
        for (int k = 1; k < 6; k++) if (k < J) fr_mul(W.w[k], W.w[k - 1], rho);
#pragma unroll
        for (int k = 0; k < 6; k++) if (k < J) neg_product(W.nw[k], W.w[k]);
        term(j, W, sum);
        if (with_weights) weights(j, W);
        if (j + 1 < cnt) { fr_mul(base, W.w[J - 1], rho); fr_mul(W.t, W.t, rho); }
    }
    Fr one; fr_one(one);
    fr_mul(sum, sum, one);
}
// what column k adds for row i (o: 0, non-membership 2 — where the four common checks start).  The columns that close the G1 equation:
//   non-membership   P: w0 s_u - w1 c          K: w0 s_v + w1 s_w
//   both             X: w[o] s_sigma - w[o+2] s_delta_sigma          Y: w[o+1] s_rho - w[o+3] s_delta_rho
// then the columns of the two sides, which leave NEGATED when they are finished:
//   Z (p): t (s_delta_sigma + s_delta_rho)     V: t c     non-membership K (p): t s_v     Z (q): t (s_sigma + s_rho)
template <class Cc, class Rs> FRD void col_term(Fr &sum, int kind, size_t i, size_t k, const RowWeights &W, Cc chal, Rs resp) {
    const Shape sh = shape_of(kind);
    const int o = sh.checks - 4;
    Fr a, b;
    if ((int)k < o) {
        if (k == 0) { resp(i, RS_U, a); add_product(sum, a, W.w[0]); chal(i, a); add_product(sum, a, W.nw[1]); }
        else { resp(i, RS_V, a); add_product(sum, a, W.w[0]); resp(i, RS_W, a); add_product(sum, a, W.w[1]); }
        return;
    }
    if ((int)k < sh.g1cols) {
        // (two branches, not an index that depends on k: the weights stay in registers)
        if ((int)k == o) { resp(i, RS_SIGMA, a); add_product(sum, a, W.w[o]); resp(i, RS_DSIGMA, a); add_product(sum, a, W.nw[o + 2]); }
        else { resp(i, RS_RHO, a); add_product(sum, a, W.w[o + 1]); resp(i, RS_DRHO, a); add_product(sum, a, W.nw[o + 3]); }
        return;
    }
    const int s = (int)k - sh.g1cols;                 // 0: Z (p), 1: V, [2: K (p),] last: Z (q)
    if (s == 0) { resp(i, RS_DSIGMA, a); resp(i, RS_DRHO, b); sum2(a, a, b); }
    else if (s == 1) chal(i, a);
    else if (s < sh.pcols) resp(i, RS_V, a);
    else { resp(i, RS_SIGMA, a); resp(i, RS_RHO, b); sum2(a, a, b); }
    add_product(sum, a, W.t);
}
// o = a x + b y as a product.  a, b, x, y: products
FRD void two_products(Fr &o, const Fr &a, const Fr &x, const Fr &b, const Fr &y) {
    Fr p, q, one; fr_one(one);
    fr_mul(p, a, x); fr_mul(q, b, y);
    sum2(p, p, q);
    fr_mul(o, p, one);
}
// the weights of row i over its own points in the one G1 equation, in the order of its points:
//   E_C 0;  T_sigma -w[o] c + w[o+2] s_y;  T_rho -w[o+1] c + w[o+3] s_y;  R_sigma -w[o];  R_rho -w[o+1];  R_delta_sigma -w[o+2];  R_delta_rho -w[o+3]
//   non-membership: E_d -w0 c;  E_d_inv w1 s_u;  R_A -w0;  R_B -w1
// then (q = pts, pts + 1, pts + 2) the weight of E_C in the side against P~, t s_y; of E_C in the side against pk — and of E_d against P~ — t c; and t itself,
// the exponent of R_E.  st(q, Fr) stores weight q (a product)
template <class Cc, class Rs, class ST> FRD void row_weights(int kind, size_t i, const RowWeights &W, Cc chal, Rs resp, ST st) {
    const Shape sh = shape_of(kind);
    const int o = sh.checks - 4;
    Fr c, sy, x;
    chal(i, c); resp(i, RS_Y, sy);
    fr_zero(x); st(0, x);
    two_products(x, c, W.nw[o], sy, W.w[o + 2]); st(1, x);
    two_products(x, c, W.nw[o + 1], sy, W.w[o + 3]); st(2, x);
#pragma unroll
    for (int k = 0; k < 4; k++) st(3 + k, W.nw[o + k]);
    if (kind != MEMBERSHIP) {
        Fr su; resp(i, RS_U, su);
        fr_mul(x, c, W.nw[0]); st(7, x);
        fr_mul(x, su, W.w[1]); st(8, x);
        st(9, W.nw[0]); st(10, W.nw[1]);
    }
    fr_mul(x, sy, W.t); st(sh.pts, x);
    fr_mul(x, c, W.t); st(sh.pts + 1, x);
    st(sh.pts + 2, W.t);
}

// ---- words only ----
FRD bool words_zero(const uint32_t *w, int k) { uint32_t o = 0; for (int i = 0; i < k; i++) o |= w[i]; return o == 0; }
// the first failure in the order the reference returns them: Schnorr check j (its sum is not the identity) is j + 1 — non-membership 1 E_d, 2 E_d_inv, then
// for both sigma, rho, delta_sigma, delta_rho — and the pairing J + 1.  0: verified.  seg_ok(j): the sum of segment j is the identity
template <class S> FRD uint8_t first_failure(int kind, S seg_ok, bool pairing_ok) {
    const int J = shape_of(kind).checks;
    for (int j = 0; j < J; j++) if (!seg_ok(j)) return (uint8_t)(j + 1);
    return pairing_ok ? 0 : (uint8_t)(J + 1);
}

#if defined(__HIPCC__)
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
using colk::ld_words;
using colk::st_words;
// what the kernels below load: chal: rows x 8 words, resp: rows x (5 | 8) x 8 words
struct ProofIn {
    const uint32_t *__restrict__ chal, *__restrict__ resp; int kind; bool mont;
    __device__ __forceinline__ void c(size_t i, Fr &x) const { ld_words(x, chal, i, mont); }
    __device__ __forceinline__ void r(size_t i, unsigned q, Fr &x) const { ld_words(x, resp, i * (kind == MEMBERSHIP ? 5 : 8) + q, mont); }
};
#define ACCGT_FUNCTORS(in) [&](size_t r_, Fr &x_) { in.c(r_, x_); }, [&](size_t r_, unsigned q_, Fr &x_) { in.r(r_, q_, x_); }
// own[(i * n_own + t) * 8 ..] = the canonical words of the row's own scalars (own_scalar), one lane per scalar
__global__ void __launch_bounds__(256) k_acc_gt_own(ProofIn in, size_t rows, uint32_t *__restrict__ own) {
    const unsigned n_own = (unsigned)shape_of(in.kind).own;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n_own;
    if (i >= rows) return;
    Fr o;
    own_scalar(o, in.kind, i, (unsigned)(t % n_own), ACCGT_FUNCTORS(in));
    st_words(own, t, o);
}
// One lane per (row, base): bases[(i * n_own + t) * 24 ..] = the point stage_src names.  points: rows x pts x 24 words; shared: V, X, Y, Z, K, P
struct SharedPoints { uint32_t w[N_SHARED][2 * FQW]; };
__global__ void __launch_bounds__(256) k_acc_gt_stage(const uint32_t *__restrict__ points, SharedPoints shared, int kind, size_t rows, uint32_t *__restrict__ bases) {
    const Shape sh = shape_of(kind);
    const unsigned n_own = (unsigned)sh.own;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n_own;
    if (i >= rows) return;
    const unsigned src = stage_src(kind, (unsigned)(t % n_own));
    uint4 *o = reinterpret_cast<uint4 *>(bases + t * 2 * FQW);
    if (src >= 16) {
        const uint32_t *w = shared.w[src - 16];
        for (int k = 0; k < 6; k++) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else {
        const uint4 *q = reinterpret_cast<const uint4 *>(points + (i * (size_t)sh.pts + src) * 2 * FQW);
        for (int k = 0; k < 6; k++) o[k] = q[k];
    }
}
// One lane per (row, side): the last two segment sums of a row as the segment MSM left them — sums[36 j ..] normalised (x, y, z), inf[j] their identity flags,
// j = segs i + segs - 2 the sum p, j + 1 the sum q — as the pairing's operands: pa[24 i ..] = q (against pk), pb[24 i ..] = p (against P~), the identity as
// zero words, skip[i] / skip[rows + i] = that side is the identity
__global__ void __launch_bounds__(256) k_acc_gt_sides(const uint32_t *__restrict__ sums, const uint8_t *__restrict__ inf, int kind, size_t rows, uint32_t *__restrict__ pa,
                                                      uint32_t *__restrict__ pb, uint8_t *__restrict__ skip) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t >> 1;
    if (i >= rows) return;
    const unsigned side = (unsigned)(t & 1), segs = (unsigned)shape_of(kind).segs;      // side 0: q, side 1: p
    const size_t j = i * segs + segs - 1 - side;
    const bool z = inf[j] != 0;
    const uint4 *q = reinterpret_cast<const uint4 *>(sums + j * 3 * FQW);
    uint4 *o = reinterpret_cast<uint4 *>((side ? pb : pa) + i * 2 * FQW);
    for (int k = 0; k < 6; k++) o[k] = z ? make_uint4(0, 0, 0, 0) : q[k];
    skip[side * rows + i] = z ? 1 : 0;
}
// One lane per row: seg_inf[segs i ..] are the identity flags of the row's segment sums (a Schnorr check holds iff its sum is the identity), gt[144 i ..] the
// value of its pairing and r_e[144 i ..] its own R_E, both in the ABI's form (canonical Montgomery words: what k_final_exp writes is what the caller uploads)
__global__ void __launch_bounds__(256) k_acc_gt_verdict(const uint8_t *__restrict__ seg_inf, const uint32_t *__restrict__ gt, const uint32_t *__restrict__ r_e, int kind,
                                                        size_t rows, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const unsigned segs = (unsigned)shape_of(kind).segs;
    const uint4 *a = reinterpret_cast<const uint4 *>(gt + i * GTW), *b = reinterpret_cast<const uint4 *>(r_e + i * GTW);
    uint32_t diff = 0;
    for (int k = 0; k < GTW / 4; k++) { const uint4 x = a[k], y = b[k]; diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w); }
    status[i] = first_failure(kind, [&](int j) { return seg_inf[i * segs + j] != 0; }, diff == 0);
}
// grid (columns, blocks): block (k, b) sums column k over the rows [b * 256 * run, ..) of the chunk (col_sums.hip.h's frame).  Column 0 also writes the rows'
// weights as canonical words: wts[(pts i + q) * 8 ..] over the own points, wp[8 i ..] = t s_y, wq[8 i ..] = t c, tp[8 i ..] = t = rho^(i0 + i)
// (KIND is a template parameter: the two proof shapes are two kernels, so neither carries the other's branches and registers)
template <int KIND>
__global__ void __launch_bounds__(256) k_acc_gt_col_sums(ProofIn in, colk::RhoWords rho_words, size_t rows, size_t i0, size_t run, uint32_t *__restrict__ part,
                                                         uint32_t *__restrict__ wts, uint32_t *__restrict__ wp, uint32_t *__restrict__ wq, uint32_t *__restrict__ tp) {
    in.kind = KIND;
    const unsigned n_pts = (unsigned)shape_of(KIND).pts;
    const size_t k = blockIdx.x;
    Fr rho;
    fr_from_words(rho, rho_words.w, in.mont);
    colk::col_block_sum(k, rows, run, part, [&](size_t lo, size_t cnt, Fr &sum) {
        col_run(KIND, rho, i0 + lo, cnt, k == 0,
                [&](size_t j, const RowWeights &W, Fr &s) { col_term(s, KIND, lo + j, k, W, ACCGT_FUNCTORS(in)); },
                [&](size_t j, const RowWeights &W) {
                    const size_t i = lo + j;
                    row_weights(KIND, i, W, ACCGT_FUNCTORS(in), [&](unsigned q, const Fr &x) {
                        if (q < n_pts) st_words(wts, i * n_pts + q, x); else st_words(q == n_pts ? wp : q == n_pts + 1 ? wq : tp, i, x);
                    });
                },
                sum);
    });
}
#endif

}  // namespace accgt
