// crypto_amd/csrc/acc_pok_kernels.hip.h — the scalar and staging half of verifying accumulator proofs in bulk on gfx950 (dock_acc_pok.hip drives it).
//
// Device side of the CDH proofs of the VB accumulator (vb_accumulator/src/proofs_cdh.rs: MembershipProof::verify :138-149, NonMembershipProof::verify with
// verify_except_pairing :365-387, :481-523; short_group_sig/src/weak_bb_sig_pok_cdh.rs:145-287) for many proofs against ONE accumulator value V and one key.
//   membership      points A', Abar, T; responses z1 (over V), z2 (over -A'); challenge c
//                   z1 V - z2 A' - c Abar - T = O                                            one 4-term segment  [V, A', Abar, T] . (z1, -z2, -c, -1)
//   non-membership  points C', Cbar, J, T1, T2; responses s_r, s_y, s_d; challenge c; the shared P and Q
//                   s_d Q - c J - T2 = O                                                     a 3-term segment    [Q, J, T2] . (s_d, -c, -1)
//                   s_r V - s_y C' - s_d P - c Cbar - T1 = O                                 a 5-term segment    [V, C', P, Cbar, T1] . (s_r, -s_y, -s_d, -c, -1)
// and for both the pairing e(W', pk) e(-Wbar, P~) = 1 over the proof's first two points.  The scalar field has to
//   write the own scalars where the segmented small MSM reads them                                                        k_acc_pok_own
//   one verdict: the coefficients of the shared points and the weights over the proofs' own points (weights u_i on the long check, v_i on the short one,
//   t_i on the pairing; membership: u_i = t_i = rho^i; non-membership: u_i = rho^2i, v_i = rho^(2i+1), t_i = rho^i)     k_acc_pok_col_sums, k_col_finish
// and two kernels move words only: k_acc_pok_stage lays the points out for the segment MSM and the pairing (-Wbar by a flip of y), k_acc_pok_verdict folds a
// row's checks into its status byte.  The per-lane routines are FRD functions over load / store functors, as bbs_pok_kernels.hip.h's are: the same text runs
// on the host under -DFP29_CHECK (tests/native/acc_pok_dev_host_shim.cpp).  Operand classes as in col_sums.hip.h: "product" (limbs < 2^29, value < 2 r),
// "lazy sum" (one carry pass after every addition of a product).
//
// Bounds of the batch sums.  A lane's run of COL_RUN = 16 rows adds ONE product per row to its sum: at most 16 terms, value < 32 r, limbs
// <= 2^29 + 1 after each carry pass.  The fixed tree of a block of 256 adds sums of equal depth: after its eight levels a slot holds at most 256 x 16 products,
// value < 2^13 r — a first operand of fr_mul (limbs < 2^31, value x 2 r far below 2^34 r^2).  The second pass adds products, one per block, with a carry pass
// each.  A weight is a product, the negation of a product (neg_product: 512 r - v < 514 r as a first operand) or -(a b) of two products.
#pragma once
#include "col_sums.hip.h"

namespace accpk {
using namespace fr29;
using colk::neg_product;
using colk::pow_start;

constexpr int FQW = 12;           // u32 words of a base-field element
constexpr int MEMBERSHIP = 0, NON_MEMBERSHIP = 1;
// the shape of a proof kind: points and responses per proof, own scalars (= bases of its segments) per row, segments per row, shared points, columns of the batch
struct Shape { int pts, resp, own, segs, shared; };
FRD Shape shape_of(int kind) { return kind == MEMBERSHIP ? Shape{3, 2, 4, 1, 1} : Shape{5, 3, 8, 2, 3}; }
constexpr int MAX_OWN = 8, MAX_PTS = 5, MAX_SHARED = 3;

// sum += a b, one carry pass.  a, b: products
FRD void add_product(Fr &sum, const Fr &a, const Fr &b) {
    Fr p; fr_mul(p, a, b);                            // 2 r * 2 r
    fr_add(sum, sum, p); fr_norm(sum, sum);
}
// o = -(a b) as a product.  a, b: products
FRD void neg_mul(Fr &o, const Fr &a, const Fr &b) {
    Fr p; fr_mul(p, a, b);                            // 2 r * 2 r
    neg_product(o, p);
}
// own scalar t of row i.  chal(i, Fr &) and resp(i, q, Fr &) load products; resp: z1, z2 (membership) / s_r, s_y, s_d (non-membership)
//   membership      (z1, -z2, -c, -1) over [V, A', Abar, T]
//   non-membership  (s_d, -c, -1) over [Q, J, T2], then (s_r, -s_y, -s_d, -c, -1) over [V, C', P, Cbar, T1]
template <class Cc, class Rs> FRD void own_scalar(Fr &o, int kind, size_t i, unsigned t, Cc chal, Rs resp) {
    Fr v;
    if (kind == MEMBERSHIP) {
        if (t == 0) { resp(i, 0, o); return; }
        if (t == 1) resp(i, 1, v); else if (t == 2) chal(i, v); else fr_one(v);
    } else {
        if (t == 0) { resp(i, 2, o); return; }
        if (t == 3) { resp(i, 0, o); return; }
        if (t == 1 || t == 6) chal(i, v); else if (t == 4) resp(i, 1, v); else if (t == 5) resp(i, 2, v); else fr_one(v);
    }
    neg_product(o, v);
}
// One lane's run of a column of the batch: rows j < cnt of the run see the weights of row e0 + j — membership: u = v = t = rho^(e0 + j); non-membership:
// u = rho^(2 (e0 + j)), v = u rho and, for the lanes of column 0 (with_weights), t = rho^(e0 + j).  term(j, u, v, sum) adds the column's product of that row
// to the lazy sum (add_product); weights(j, u, v, t) is called for the lanes of column 0.  The sum leaves reduced to a product.  rho: a product, so is
// everything derived from it.
template <class T, class W> FRD void col_run(int kind, const Fr &rho, size_t e0, size_t cnt, bool with_weights, T term, W weights, Fr &sum) {
    // the lanes that write weights carry t and square it (u = t^2); the others carry u alone and step it by rho^2: one chain either way
    const bool chain_t = kind != MEMBERSHIP && with_weights;
    Fr step, u, v, t;
    if (kind == MEMBERSHIP || chain_t) step = rho; else fr_mul(step, rho, rho);
    pow_start(u, step, e0);
    fr_zero(sum);
    for (size_t j = 0; j < cnt; j++) {
        t = u;
        if (chain_t) fr_mul(u, t, t);
        if (kind == MEMBERSHIP) v = u; else fr_mul(v, u, rho);
        term(j, u, v, sum);
        if (with_weights) weights(j, u, v, t);
        if (j + 1 < cnt) fr_mul(u, t, step);
    }
    Fr one; fr_one(one);
    fr_mul(sum, sum, one);
}
// what column k adds for row i: membership: S_V: u z1;  non-membership: S_V: u s_r;  S_P: u s_d (negated when the column is finished);  S_Q: v s_d
template <class Rs> FRD void col_term(Fr &sum, int kind, size_t i, size_t k, const Fr &u, const Fr &v, Rs resp) {
    Fr a;
    if (kind == MEMBERSHIP || k == 0) { resp(i, 0, a); add_product(sum, a, u); }
    else { resp(i, 2, a); if (k == 1) add_product(sum, a, u); else add_product(sum, a, v); }      // (no select between the two references: it would put u and v in memory)
}
// the weights of row i over its own points in the one G1 equation — membership (A', Abar, T): -u z2, -u c, -u; non-membership (C', Cbar, J, T1, T2):
// -u s_y, -u c, -v c, -u, -v — then t and -t for the two sides of the pairing.  st(q, Fr) stores weight q < pts + 2 (a product)
template <class Cc, class Rs, class ST> FRD void row_weights(int kind, size_t i, const Fr &u, const Fr &v, const Fr &t, Cc chal, Rs resp, ST st) {
    Fr a, w;
    resp(i, 1, a); neg_mul(w, a, u); st(0, w);
    chal(i, a); neg_mul(w, a, u); st(1, w);
    if (kind == MEMBERSHIP) {
        neg_product(w, u); st(2, w);
        st(3, t); st(4, w);                           // (t = u)
        return;
    }
    neg_mul(w, a, v); st(2, w);
    neg_product(w, u); st(3, w);
    neg_product(w, v); st(4, w);
    st(5, t);
    neg_product(w, t); st(6, w);
}

// ---- base-field words: comparisons and one subtraction from p (affine Montgomery words of the ABI; -y of y != 0 is p - y in either form) ----
#define ACCPK_P_WORDS {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau}
FRD bool fq_zero_words(const uint32_t *w, int k) { uint32_t o = 0; for (int i = 0; i < k; i++) o |= w[i]; return o == 0; }
// o = p - y for 0 < y < p; zero stays zero
FRD void fq_neg_words(uint32_t o[FQW], const uint32_t y[FQW]) {
    constexpr uint32_t P_[FQW] = ACCPK_P_WORDS;
    if (fq_zero_words(y, FQW)) { for (int i = 0; i < FQW; i++) o[i] = 0; return; }
    uint64_t br = 0;
    for (int i = 0; i < FQW; i++) { const uint64_t d = (uint64_t)P_[i] - y[i] - br; o[i] = (uint32_t)d; br = (d >> 32) & 1; }
}
// where slot `slot` of a row takes its point from: 0 .. 4 a point of the proof, 8 + k the shared point k (V, P, Q).  Slots below `own` are the bases of the
// row's segments, the last two the sides of its pairing (the proof's first point, then its second, whose y is flipped)
//   membership      [V, A', Abar, T | A', Abar]                     non-membership  [Q, J, T2 | V, C', P, Cbar, T1 | C', Cbar]
FRD unsigned stage_src(int kind, unsigned slot) {
    return (unsigned)((kind == MEMBERSHIP ? 0x102108ull : 0x103190842Aull) >> (4 * slot)) & 15u;
}
// the first failure in the order the reference returns them.  Membership (weak_bb_sig_pok_cdh.rs:195-217, :270-287): 1 A' is the identity, 2 the Schnorr
// check, 3 the pairing.  Non-membership (proofs_cdh.rs:481-523, :375-385): 1 C' is the identity, 2 J is, 3 the check of J over Q, 4 the five-term check,
// 5 the pairing.  0: verified
FRD uint8_t mem_status(bool a_inf, bool schnorr_ok, bool pairing_ok) { return a_inf ? 1 : !schnorr_ok ? 2 : !pairing_ok ? 3 : 0; }
FRD uint8_t nm_status(bool c_inf, bool j_inf, bool short_ok, bool long_ok, bool pairing_ok) {
    return c_inf ? 1 : j_inf ? 2 : !short_ok ? 3 : !long_ok ? 4 : !pairing_ok ? 5 : 0;
}

#if defined(__HIPCC__)
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
using colk::ld_words;
using colk::st_words;
// what the kernels below load: chal: rows x 8 words, resp: rows x (2 | 3) x 8 words
struct ProofIn {
    const uint32_t *__restrict__ chal, *__restrict__ resp; int kind; bool mont;
    __device__ __forceinline__ void c(size_t i, Fr &x) const { ld_words(x, chal, i, mont); }
    __device__ __forceinline__ void r(size_t i, unsigned q, Fr &x) const { ld_words(x, resp, i * (kind == MEMBERSHIP ? 2 : 3) + q, mont); }
};
#define ACCPK_FUNCTORS(in) [&](size_t r_, Fr &x_) { in.c(r_, x_); }, [&](size_t r_, unsigned q_, Fr &x_) { in.r(r_, q_, x_); }
// own[(i * n_own + t) * 8 ..] = the canonical words of the row's own scalars (own_scalar), one lane per scalar
__global__ void __launch_bounds__(256) k_acc_pok_own(ProofIn in, size_t rows, uint32_t *__restrict__ own) {
    const unsigned n_own = (unsigned)shape_of(in.kind).own;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n_own;
    if (i >= rows) return;
    Fr o;
    own_scalar(o, in.kind, i, (unsigned)(t % n_own), ACCPK_FUNCTORS(in));
    st_words(own, t, o);
}
// One lane per (row, slot), slot < own + 2: the bases of the row's segments, own[(i * n_own + slot) * 24 ..] (stage_src), and the two sides of its pairing,
// pa[24 i ..] = the proof's first point, pb[24 i ..] = minus its second (y flipped), with skip[i] / skip[rows + i] = that point is the identity (zero words)
// and skip[2 rows + i] = J is (non-membership; membership: 0).  points: rows x pts x 24 words; shared: V, P, Q
struct SharedPoints { uint32_t w[MAX_SHARED][2 * FQW]; };
__global__ void __launch_bounds__(256) k_acc_pok_stage(const uint32_t *__restrict__ points, SharedPoints shared, int kind, size_t rows, uint32_t *__restrict__ own,
                                                       uint32_t *__restrict__ pa, uint32_t *__restrict__ pb, uint8_t *__restrict__ skip) {
    const Shape sh = shape_of(kind);
    const unsigned n_own = (unsigned)sh.own, n_slots = n_own + 2;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n_slots;
    const unsigned slot = (unsigned)(t % n_slots);
    if (i >= rows) return;
    const unsigned src = stage_src(kind, slot);
    uint32_t w[2 * FQW];
    if (src >= 8) { for (int k = 0; k < 2 * FQW; k++) w[k] = shared.w[src - 8][k]; }
    else {
        const uint4 *q = reinterpret_cast<const uint4 *>(points + (i * (size_t)sh.pts + src) * 2 * FQW);
        for (int k = 0; k < 6; k++) { const uint4 a = q[k]; w[4 * k] = a.x; w[4 * k + 1] = a.y; w[4 * k + 2] = a.z; w[4 * k + 3] = a.w; }
    }
    uint32_t *dst = slot < n_own ? own + (i * n_own + slot) * 2 * FQW : (slot == n_own ? pa : pb) + i * 2 * FQW;
    if (slot >= n_own) skip[(slot - n_own) * rows + i] = fq_zero_words(w, 2 * FQW) ? 1 : 0;
    if (slot == 1) skip[2 * rows + i] = (kind != MEMBERSHIP && fq_zero_words(w, 2 * FQW)) ? 1 : 0;
    if (slot == n_own + 1) { uint32_t y[FQW]; fq_neg_words(y, w + FQW); for (int k = 0; k < FQW; k++) w[FQW + k] = y[k]; }
    uint4 *o = reinterpret_cast<uint4 *>(dst);
    for (int k = 0; k < 6; k++) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
// One lane per row: seg_inf[segs i ..] are the identity flags of the row's segment sums (a check holds iff its sum is the identity), pairing[i] the pairing's
// verdict byte, skip as k_acc_pok_stage wrote it
__global__ void __launch_bounds__(256) k_acc_pok_verdict(const uint8_t *__restrict__ seg_inf, const uint8_t *__restrict__ pairing, const uint8_t *__restrict__ skip, int kind,
                                                         size_t rows, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    status[i] = kind == MEMBERSHIP ? mem_status(skip[i] != 0, seg_inf[i] != 0, pairing[i] != 0)
                                   : nm_status(skip[i] != 0, skip[2 * rows + i] != 0, seg_inf[2 * i] != 0, seg_inf[2 * i + 1] != 0, pairing[i] != 0);
}
// grid (shared, blocks): block (k, b) sums column k over the rows [b * 256 * run, ..) of the chunk as k_bbs_pok_col_sums does (a lane's own start powers, a
// fixed tree in LDS, part[(k * gridDim.y + b) * NL ..] in the internal form).  Column 0 also writes the rows' weights as canonical words: wts[(pts i + q) * 8 ..]
// over the own points (q < pts), tp[8 i ..] = rho^(i0 + i), tn[8 i ..] = -rho^(i0 + i)
// (KIND is a template parameter: the two proof shapes are two kernels, so neither carries the other's branches and registers)
template <int KIND>
__global__ void __launch_bounds__(256) k_acc_pok_col_sums(ProofIn in, colk::RhoWords rho_words, size_t rows, size_t i0, size_t run, uint32_t *__restrict__ part,
                                                          uint32_t *__restrict__ wts, uint32_t *__restrict__ tp, uint32_t *__restrict__ tn) {
    in.kind = KIND;
    const unsigned n_pts = (unsigned)shape_of(KIND).pts;
    const size_t k = blockIdx.x;
    Fr rho;
    fr_from_words(rho, rho_words.w, in.mont);
    colk::col_block_sum(k, rows, run, part, [&](size_t lo, size_t cnt, Fr &sum) {
        col_run(KIND, rho, i0 + lo, cnt, k == 0,
                [&](size_t j, const Fr &u, const Fr &v, Fr &s) { col_term(s, KIND, lo + j, k, u, v, [&](size_t r_, unsigned q_, Fr &x_) { in.r(r_, q_, x_); }); },
                [&](size_t j, const Fr &u, const Fr &v, const Fr &tw) {
                    const size_t i = lo + j;
                    row_weights(KIND, i, u, v, tw, ACCPK_FUNCTORS(in),
                                [&](unsigned q, const Fr &x) { if (q < n_pts) st_words(wts, i * n_pts + q, x); else st_words(q == n_pts ? tp : tn, i, x); });
                },
                sum);
    });
}
#endif

}  // namespace accpk
