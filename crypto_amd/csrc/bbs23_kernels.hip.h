// crypto_amd/csrc/bbs23_kernels.hip.h — the scalar and staging half of verifying BBS (2023) proofs of knowledge in bulk on gfx950 (dock_bbs.hip drives it).
//
// Device side of the two PoKOfSignature23G1Proof::verify of the reference (bbs_plus/src/proof_23_cdl.rs:302-549, proof_23_ietf.rs:244-479) for many proofs
// under one key.  The signature parameters [g1, h_1 .. h_L] are ONE base set, P_i = the small MSM of the row (c_i, y_i1 .. y_iL) over it, y_ij = c_i m_ij
// (revealed) or z_ij (hidden).
//   CDL   points Abar, Bbar, d, T1, T2; responses z1 (over Abar), z2, z3 (over d); challenge c
//         z1 Abar + z2 d - c Bbar - T1 = O                              a 4-term segment  [Abar, d, Bbar, T1] . (z1, z2, -c, -1)
//         P_i + z3 d - T2 = O                                           a 2-term segment  [d, T2] . (z3, -1), compared with -P_i
//   IETF  points Abar, Bbar, T; responses z_a (over Abar), z_b (over Bbar)
//         P_i + z_a Abar + z_b Bbar - T = O                             a 3-term segment  [Abar, Bbar, T] . (z_a, z_b, -1), compared with -P_i
// and for both the pairing e(Abar, w) e(-Bbar, g2) = 1.  The scalar field has to
//   write the rows where the many-row MSM reads them (msm_many.hip.h many_rows_resident)                                   k_bbs23_rows
//   write the own scalars where the segmented small MSM reads them                                                        k_bbs23_own
//   one verdict: the column sums C_k and the weights over the proofs' own points (CDL: u_i = rho^2i on the first check, v_i = rho^(2i+1) on the second,
//   t_i = rho^i on the pairing; IETF: u_i = t_i = rho^i)                                                                 k_bbs23_col_sums, k_col_finish
// and two kernels move words only: k_bbs23_stage lays the points out for the segment MSM and the pairing (-Bbar by a flip of y), k_bbs23_verdict folds a
// row's checks into its status byte.  The proof kind is a template parameter of every kernel that depends on it: two kernels, neither carries the other's
// branches and registers.  The per-lane routines are FRD functions over load / store functors, as bbs_pok_kernels.hip.h's are: the same text runs on the
// host under -DFP29_CHECK (tests/native/bbs23_dev_host_shim.cpp).  Operand classes as in col_sums.hip.h: "product" (limbs < 2^29, value < 2 r), "lazy
// sum" (one carry pass after every addition of a product).
//
// Bounds of the batch sums.  Every column, C_0 included, adds ONE product per row to a lane's sum: a run of COL_RUN = 16 rows is at most 16
// terms, value < 32 r, limbs <= 2^29 + 1 after each carry pass.  The fixed tree of a block of 256 adds sums of equal depth: after its eight levels a slot
// holds at most 256 x 16 products, value < 2^13 r — a first operand of fr_mul (limbs < 2^31, value x 2 r far below 2^34 r^2).  The second pass adds products,
// one per block, with a carry pass each.  A weight is a product, the negation of a product (neg_product: 512 r - v < 514 r as a first operand) or, for CDL's d,
// u z2 + v z3: a lazy sum of two products (value < 4 r, one carry pass) reduced by a product with one.
#pragma once
#include "bbs_routines.hip.h"

namespace bbs23k {
using namespace fr29;
using colk::neg_product;
using colk::pow_start;

constexpr int FQW = 12;           // u32 words of a base-field element
constexpr int CDL = 0, IETF = 1;
// the shape of a proof kind: points and fixed responses per proof, own scalars (= bases of its segments) per row, segments per row
struct Shape { int pts, resp, own, segs; };
FRD Shape shape_of(int kind) { return kind == CDL ? Shape{5, 3, 6, 2} : Shape{3, 2, 3, 1}; }
constexpr int MAX_PTS = 5;

// sum += a b, one carry pass.  a, b: products
FRD void add_product(Fr &sum, const Fr &a, const Fr &b) {
    Fr p; fr_mul(p, a, b);                            // 2 r * 2 r
    fr_add(sum, sum, p); fr_norm(sum, sum);
}
// entry j of the values of row i as the Schnorr check over the parameters weighs it: c_i m_ij where j is revealed, the response as it stands where it is
// hidden.  chal(i, Fr &), val(i, j, Fr &) load products; rev(i, j) is the mask byte
template <class Cc, class V, class Rv> FRD void value(Fr &y, size_t i, size_t j, Cc chal, V val, Rv rev) {
    Fr v, mult; fr_one(mult);
    val(i, j, v);
    if (rev(i, j)) chal(i, mult);
    fr_mul(y, v, mult);                               // 2 r * 2 r
}
// entry k of row i: c_i, y_i(k-1)
template <class Cc, class V, class Rv> FRD void row_entry(Fr &o, size_t i, size_t k, Cc chal, V val, Rv rev) {
    if (k == 0) chal(i, o); else value(o, i, k - 1, chal, val, rev);
}
// own scalar t of row i.  resp(i, q, Fr &) loads z1, z2, z3 (CDL) / z_a, z_b (IETF)
//   CDL   (z1, z2, -c, -1) over [Abar, d, Bbar, T1], then (z3, -1) over [d, T2]
//   IETF  (z_a, z_b, -1) over [Abar, Bbar, T]
template <class Cc, class Rs> FRD void own_scalar(Fr &o, int kind, size_t i, unsigned t, Cc chal, Rs resp) {
    Fr v;
    if (t < 2) { resp(i, t, o); return; }
    if (kind == CDL && t == 4) { resp(i, 2, o); return; }
    if (kind == CDL && t == 2) chal(i, v); else fr_one(v);
    neg_product(o, v);
}
// One lane's run of a column of the batch: rows j < cnt of the run see the weights of row e0 + j — IETF: u = v = t = rho^(e0 + j); CDL:
// u = rho^(2 (e0 + j)), v = u rho and, for the lanes of column 0 (with_weights), t = rho^(e0 + j).  term(j, u, v, sum) adds the column's product of that row
// to the lazy sum (add_product); weights(j, u, v, t) is called for the lanes of column 0.  The sum leaves reduced to a product.  rho: a product, so is
// everything derived from it.
template <class T, class W> FRD void col_run(int kind, const Fr &rho, size_t e0, size_t cnt, bool with_weights, T term, W weights, Fr &sum) {
    // the lanes that write weights carry t and square it (u = t^2); the others carry u alone and step it by rho^2: one chain either way
    const bool chain_t = kind == CDL && with_weights;
    Fr step, u, v, t;
    if (kind == IETF || chain_t) step = rho; else fr_mul(step, rho, rho);
    pow_start(u, step, e0);
    fr_zero(sum);
    for (size_t j = 0; j < cnt; j++) {
        t = u;
        if (chain_t) fr_mul(u, t, t);
        if (kind == IETF) v = u; else fr_mul(v, u, rho);
        term(j, u, v, sum);
        if (with_weights) weights(j, u, v, t);
        if (j + 1 < cnt) fr_mul(u, t, step);
    }
    Fr one; fr_one(one);
    fr_mul(sum, sum, one);
}
// what column k adds for row i under the weight w of the check over the parameters (CDL: v, IETF: u): C_0: w c;  C_j: w y_ij
template <class Cc, class V, class Rv> FRD void col_term(Fr &sum, size_t i, size_t k, const Fr &w, Cc chal, V val, Rv rev) {
    Fr a;
    row_entry(a, i, k, chal, val, rev);
    add_product(sum, a, w);
}
// the weights of row i over its own points in the one G1 equation — CDL (Abar, Bbar, d, T1, T2): u z1, -u c, u z2 + v z3, -u, -v; IETF (Abar, Bbar, T):
// u z_a, u z_b, -u — then t and -t for the two sides of the pairing.  st(q, Fr) stores weight q < pts + 2 (a product)
template <class Cc, class Rs, class ST> FRD void row_weights(int kind, size_t i, const Fr &u, const Fr &v, const Fr &t, Cc chal, Rs resp, ST st) {
    Fr a, w, one; fr_one(one);
    resp(i, 0, a); fr_mul(w, a, u); st(0, w);
    if (kind == IETF) {
        resp(i, 1, a); fr_mul(w, a, u); st(1, w);
        neg_product(w, u); st(2, w);
        st(3, t); st(4, w);                           // (t = u)
        return;
    }
    chal(i, a); fr_mul(w, a, u); neg_product(w, w); st(1, w);
    resp(i, 1, a); fr_mul(w, a, u);
    resp(i, 2, a); add_product(w, a, v); fr_mul(w, w, one); st(2, w);      // a lazy sum of two products
    neg_product(w, u); st(3, w);
    neg_product(w, v); st(4, w);
    st(5, t);
    neg_product(w, t); st(6, w);
}

// ---- base-field words: comparisons and one subtraction from p (affine Montgomery words of the ABI; -y of y != 0 is p - y in either form) ----
#define BBS23K_P_WORDS {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau}
FRD bool fq_zero_words(const uint32_t *w, int k) { uint32_t o = 0; for (int i = 0; i < k; i++) o |= w[i]; return o == 0; }
// o = p - y for 0 < y < p; zero stays zero
FRD void fq_neg_words(uint32_t o[FQW], const uint32_t y[FQW]) {
    constexpr uint32_t P_[FQW] = BBS23K_P_WORDS;
    if (fq_zero_words(y, FQW)) { for (int i = 0; i < FQW; i++) o[i] = 0; return; }
    uint64_t br = 0;
    for (int i = 0; i < FQW; i++) { const uint64_t d = (uint64_t)P_[i] - y[i] - br; o[i] = (uint32_t)d; br = (d >> 32) & 1; }
}
// a == -b for two affine points (x | y, 24 words) with flags: both identities, or equal x and y_a + y_b = p
FRD bool g1_is_negation(const uint32_t a[2 * FQW], bool a_inf, const uint32_t b[2 * FQW], bool b_inf) {
    constexpr uint32_t P_[FQW] = BBS23K_P_WORDS;
    if (a_inf || b_inf) return a_inf && b_inf;
    uint32_t diff = 0;
    uint64_t c = 0;
    for (int i = 0; i < FQW; i++) {
        diff |= a[i] ^ b[i];
        c += (uint64_t)a[FQW + i] + b[FQW + i];
        diff |= (uint32_t)c ^ P_[i];
        c >>= 32;
    }
    return diff == 0 && c == 0;
}
// which point of the proof slot `slot` of a row takes.  Slots below `own` are the bases of the row's segments, the last two the sides of its pairing (Abar,
// then Bbar, whose y is flipped)
//   CDL (Abar, Bbar, d, T1, T2)  [Abar, d, Bbar, T1 | d, T2 | Abar, Bbar]          IETF (Abar, Bbar, T)  [Abar, Bbar, T | Abar, Bbar]
FRD unsigned stage_src(int kind, unsigned slot) { return (unsigned)((kind == CDL ? 0x10423120ull : 0x10210ull) >> (4 * slot)) & 15u; }
// the first failure in the order the reference returns them, under the names both protocols share (proof_23_cdl.rs:302-549, proof_23_ietf.rs:244-479):
// 1 ZeroSignature, 2 FirstSchnorrVerificationFailed (CDL only), 3 SecondSchnorrVerificationFailed (IETF: its only Schnorr check), 4 PairingCheckFailed; 0: verified
FRD uint8_t status_of(bool a_inf, bool first_ok, bool second_ok, bool pairing_ok) { return a_inf ? 1 : !first_ok ? 2 : !second_ok ? 3 : !pairing_ok ? 4 : 0; }

#if defined(__HIPCC__)
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
using colk::ld_words;
using colk::st_words;
// what the kernels below load: chal: rows x 8 words, resp: rows x nresp x 8 words, vals: rows x L x 8 words packed, rev: rows x L bytes
struct ProofIn {
    const uint32_t *__restrict__ chal, *__restrict__ resp, *__restrict__ vals; const uint8_t *__restrict__ rev; size_t L; unsigned nresp; bool mont;
    __device__ __forceinline__ void c(size_t i, Fr &x) const { ld_words(x, chal, i, mont); }
    __device__ __forceinline__ void f(size_t i, unsigned t, Fr &x) const { ld_words(x, resp, i * nresp + t, mont); }
    __device__ __forceinline__ void v(size_t i, size_t j, Fr &x) const { ld_words(x, vals, i * L + j, mont); }
    __device__ __forceinline__ bool r(size_t i, size_t j) const { return rev[i * L + j] != 0; }
};
#define BBS23K_CHAL(in) [&](size_t r_, Fr &x_) { in.c(r_, x_); }
#define BBS23K_RESP(in) [&](size_t r_, unsigned t_, Fr &x_) { in.f(r_, t_, x_); }
#define BBS23K_VALS(in) [&](size_t r_, size_t j_, Fr &x_) { in.v(r_, j_, x_); }, [&](size_t r_, size_t j_) { return in.r(r_, j_); }
// rows[(i * n + k) * 8 ..] = the canonical words (below r) of (c_i, y_i1 .. y_iL)_k for i < rows, k < n = L + 1: one lane per entry, the lanes of a row
// neighbours.  The same for both kinds.
__global__ void __launch_bounds__(256) k_bbs23_rows(ProofIn in, size_t rows, size_t n, uint32_t *__restrict__ out_rows) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n, k = t % n;
    if (i >= rows) return;
    Fr o;
    row_entry(o, i, k, BBS23K_CHAL(in), BBS23K_VALS(in));
    st_words(out_rows, t, o);
}
// own[(i * n_own + t) * 8 ..] = the canonical words of the row's own scalars (own_scalar), one lane per scalar
template <int KIND> __global__ void __launch_bounds__(256) k_bbs23_own(ProofIn in, size_t rows, uint32_t *__restrict__ own) {
    constexpr unsigned n_own = KIND == CDL ? 6 : 3;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n_own;
    if (i >= rows) return;
    Fr o;
    own_scalar(o, KIND, i, (unsigned)(t % n_own), BBS23K_CHAL(in), BBS23K_RESP(in));
    st_words(own, t, o);
}
// One lane per (row, slot), slot < own + 2: the bases of the row's segments, own[(i * n_own + slot) * 24 ..] (stage_src), and the two sides of its pairing,
// pa[24 i ..] = Abar, pb[24 i ..] = -Bbar (y flipped; an identity stays zero words), with skip[i] / skip[rows + i] = that point is the identity (zero words).
// points: rows x pts x 24 words
template <int KIND> __global__ void __launch_bounds__(256) k_bbs23_stage(const uint32_t *__restrict__ points, size_t rows, uint32_t *__restrict__ own, uint32_t *__restrict__ pa,
                                                                         uint32_t *__restrict__ pb, uint8_t *__restrict__ skip) {
    constexpr unsigned n_own = KIND == CDL ? 6 : 3, n_slots = n_own + 2, n_pts = KIND == CDL ? 5 : 3;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n_slots;
    const unsigned slot = (unsigned)(t % n_slots);
    if (i >= rows) return;
    const unsigned src = stage_src(KIND, slot);
    uint32_t w[2 * FQW];
    const uint4 *q = reinterpret_cast<const uint4 *>(points + (i * n_pts + src) * 2 * FQW);
    for (int k = 0; k < 6; k++) { const uint4 a = q[k]; w[4 * k] = a.x; w[4 * k + 1] = a.y; w[4 * k + 2] = a.z; w[4 * k + 3] = a.w; }
    uint32_t *dst = slot < n_own ? own + (i * n_own + slot) * 2 * FQW : (slot == n_own ? pa : pb) + i * 2 * FQW;
    if (slot >= n_own) skip[(slot - n_own) * rows + i] = fq_zero_words(w, 2 * FQW) ? 1 : 0;
    if (slot == n_own + 1) { uint32_t y[FQW]; fq_neg_words(y, w + FQW); for (int k = 0; k < FQW; k++) w[FQW + k] = y[k]; }
    uint4 *o = reinterpret_cast<uint4 *>(dst);
    for (int k = 0; k < 6; k++) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
// One lane per row: seg[(segs i + q) * 36 ..] are the row's segment sums (normalised Jacobian words X | Y | 1) with their identity flags seg_inf — CDL: the
// first check's sum (it holds iff the sum is the identity), then Q_i = z3 d - T2; IETF: Q_i = z_a Abar + z_b Bbar - T — b[24 i ..] = P_i with b_inf,
// pairing[i] the pairing's verdict byte, a_inf[i] = Abar is the identity.  The check over the parameters holds iff Q_i = -P_i.
template <int KIND> __global__ void __launch_bounds__(256) k_bbs23_verdict(const uint32_t *__restrict__ seg, const uint8_t *__restrict__ seg_inf, const uint32_t *__restrict__ b,
                                                                           const uint8_t *__restrict__ b_inf, const uint8_t *__restrict__ pairing, const uint8_t *__restrict__ a_inf,
                                                                           size_t rows, uint8_t *__restrict__ status) {
    constexpr size_t segs = KIND == CDL ? 2 : 1;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const size_t sq = segs * i + (segs - 1);
    uint32_t q[2 * FQW], p[2 * FQW];
    for (int k = 0; k < 2 * FQW; k++) { q[k] = seg[sq * 3 * FQW + k]; p[k] = b[i * 2 * FQW + k]; }
    const bool first_ok = KIND == CDL ? seg_inf[segs * i] != 0 : true;
    status[i] = status_of(a_inf[i] != 0, first_ok, g1_is_negation(q, seg_inf[sq] != 0, p, b_inf[i] != 0), pairing[i] != 0);
}
// grid (L + 1, blocks): block (k, b) sums column k over the rows [b * 256 * run, ..) of the chunk as k_bbs_pok_col_sums does (a lane's own start powers, a
// fixed tree in LDS, part[(k * gridDim.y + b) * NL ..] in the internal form).  Column 0 also writes the rows' weights as canonical words: wts[(pts i + q) * 8 ..]
// over the own points (q < pts), tp[8 i ..] = rho^(i0 + i), tn[8 i ..] = -rho^(i0 + i)
template <int KIND>
__global__ void __launch_bounds__(256) k_bbs23_col_sums(ProofIn in, colk::RhoWords rho_words, size_t rows, size_t i0, size_t run, uint32_t *__restrict__ part,
                                                        uint32_t *__restrict__ wts, uint32_t *__restrict__ tp, uint32_t *__restrict__ tn) {
    constexpr unsigned n_pts = KIND == CDL ? 5 : 3;
    const size_t k = blockIdx.x;
    Fr rho;
    fr_from_words(rho, rho_words.w, in.mont);
    colk::col_block_sum(k, rows, run, part, [&](size_t lo, size_t cnt, Fr &sum) {
        col_run(KIND, rho, i0 + lo, cnt, k == 0,
                [&](size_t j, const Fr &u, const Fr &v, Fr &s) {
                    if (KIND == CDL) col_term(s, lo + j, k, v, BBS23K_CHAL(in), BBS23K_VALS(in)); else col_term(s, lo + j, k, u, BBS23K_CHAL(in), BBS23K_VALS(in));
                },
                [&](size_t j, const Fr &u, const Fr &v, const Fr &tw) {
                    const size_t i = lo + j;
                    row_weights(KIND, i, u, v, tw, BBS23K_CHAL(in), BBS23K_RESP(in),
                                [&](unsigned q, const Fr &x) { if (q < n_pts) st_words(wts, i * n_pts + q, x); else st_words(q == n_pts ? tp : tn, i, x); });
                },
                sum);
    });
}
#endif

}  // namespace bbs23k
