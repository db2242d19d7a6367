// crypto_amd/csrc/bbs_pok_kernels.hip.h — the scalar half of verifying BBS+ proofs of knowledge in bulk on gfx950 (dock_bbs.hip drives it).
//
// Device side of PoKOfSignatureG1Proof::verify (bbs_plus/src/proof.rs:529-611) for many proofs under one key.  Proof i has the points A', Abar, d, T1, T2, the
// responses z1, z2 (over A', h_0), z3 (over d), z4 (over h_0), one value per message (the revealed message, or the response of a hidden one) and a challenge c.
// With the signature parameters [g1, h_0, h_1 .. h_L] as ONE base set the reference's second Schnorr check is
//   P_i + z3_i d_i - T2_i = O,   P_i = the small MSM of the row (c_i, z4_i, y_i1 .. y_iL),   y_ij = c_i m_ij (revealed) or z_ij (hidden)
// and the first one a five-term sum over the proof's own points, [A', h_0, Abar, d, T1] . [z1, z2, -c, c, -1] = O.  The scalar field has to
//   write the rows where the many-row MSM reads them (msm_many.hip.h many_rows_resident)                                  k_bbs_pok_rows
//   write the own-point scalars (z1, z2, -c, c, -1 | z3, -1) where the segmented small MSM reads them                     k_bbs_pok_own
//   one verdict: the column sums C_k and the weights of the MSMs over the own points (weights u_i = rho^2i on the first check, v_i = rho^(2i+1) on the
//   second, t_i = rho^i on the pairing)                                                                                 k_bbs_pok_col_sums, k_col_finish
// and two kernels move words only: k_bbs_pok_stage lays the points out for the segment MSM and the pairing (-Abar by a flip of y), k_bbs_pok_verdict folds
// the four checks of a row into its status byte.  The per-lane routines are FRD functions over load / store functors, as bbs_kernels.hip.h's are: the same text
// runs on the host under -DFP29_CHECK (tests/native/bbs_pok_dev_host_shim.cpp).  Operand classes as there: "product" (limbs < 2^29, value < 2 r), "lazy sum"
// (one carry pass after every addition of a product).
//
// Bounds of the batch sums.  A lane's run of COL_RUN = 16 rows adds one product per row to its sum, two in column 1 (u_i z2_i and
// v_i z4_i): at most 32 terms, value < 64 r, limbs <= 2^29 + 1 after each carry pass.  The fixed tree of a block of 256 adds sums of equal depth: after its eight
// levels a slot holds at most 256 x 32 products, value < 2^14 r — a first operand of fr_mul (limbs < 2^31, value x 2 r far below 2^34 r^2).  The second pass
// adds products, one per block, with a carry pass each.
#pragma once
#include "bbs_routines.hip.h"

namespace bbspk {
using namespace fr29;
using colk::neg_product;
using colk::pow_start;

constexpr int POK_OWN = 7;        // own-point scalars per row: five of the first check, two of the second
constexpr int POK_PTS = 5;        // points per proof: A', Abar, d, T1, T2
constexpr int FQW = 12;           // u32 words of a base-field element

// sum += a b, one carry pass.  a, b: products
FRD void add_product(Fr &sum, const Fr &a, const Fr &b) {
    Fr p; fr_mul(p, a, b);                            // 2 r * 2 r
    fr_add(sum, sum, p); fr_norm(sum, sum);
}
// entry j of the values of row i as the second check weighs it: c_i m_ij where j is revealed, the response as it stands where it is hidden.
// chal(i, Fr &), val(i, j, Fr &) load products; rev(i, j) is the mask byte
template <class Cc, class V, class Rv> FRD void pok_value(Fr &y, size_t i, size_t j, Cc chal, V val, Rv rev) {
    Fr v, mult; fr_one(mult);
    val(i, j, v);
    if (rev(i, j)) chal(i, mult);
    fr_mul(y, v, mult);                               // 2 r * 2 r
}
// entry k of row i: c_i, z4_i, y_i(k-2).  fixed(i, t, Fr &) loads z1 .. z4 for t = 0 .. 3
template <class Cc, class F, class V, class Rv> FRD void pok_row_entry(Fr &o, size_t i, size_t k, Cc chal, F fixed, V val, Rv rev) {
    if (k == 0) chal(i, o); else if (k == 1) fixed(i, 3, o); else pok_value(o, i, k - 2, chal, val, rev);
}
// own-point scalar t < 7 of row i: (z1, z2, -c, c, -1) over [A', h_0, Abar, d, T1], then (z3, -1) over [d, T2]
template <class Cc, class F> FRD void pok_own_scalar(Fr &o, size_t i, unsigned t, Cc chal, F fixed) {
    Fr v;
    if (t == 0) fixed(i, 0, o);
    else if (t == 1) fixed(i, 1, o);
    else if (t == 2) { chal(i, v); neg_product(o, v); }
    else if (t == 3) chal(i, o);
    else if (t == 5) fixed(i, 2, o);
    else { fr_one(v); neg_product(o, v); }
}
// One lane's run of a column of the batch: rows j < cnt of the run see u = rho^(2 (e0 + j)) and v = u rho.  term(j, u, v, sum) adds the column's one or two
// products of that row to the lazy sum (add_product).  The lanes of column 0 (with_weights) also carry t = rho^(e0 + j) and hand weights(j, u, v, t) the row's
// weights; the other columns do not pay for that chain.  The sum leaves reduced to a product.  rho: a product, so is everything derived from it.
template <class T, class W> FRD void pok_col_run(const Fr &rho, size_t e0, size_t cnt, bool with_weights, T term, W weights, Fr &sum) {
    Fr rho2, u, v, t, one; fr_one(one);
    fr_mul(rho2, rho, rho);
    pow_start(u, rho2, e0);
    if (with_weights) pow_start(t, rho, e0); else fr_one(t);
    fr_zero(sum);
    for (size_t j = 0; j < cnt; j++) {
        fr_mul(v, u, rho);
        term(j, u, v, sum);
        if (with_weights) weights(j, u, v, t);
        if (j + 1 < cnt) { fr_mul(u, u, rho2); if (with_weights) fr_mul(t, t, rho); }
    }
    fr_mul(sum, sum, one);
}
// what column k adds for row i: C_0: v c;  C_1: u z2 + v z4;  C_(j+1): v y_ij
template <class Cc, class F, class V, class Rv> FRD void pok_col_term(Fr &sum, size_t i, size_t k, const Fr &u, const Fr &v, Cc chal, F fixed, V val, Rv rev) {
    Fr a;
    if (k == 0) { chal(i, a); add_product(sum, a, v); }
    else if (k == 1) { fixed(i, 1, a); add_product(sum, a, u); fixed(i, 3, a); add_product(sum, a, v); }
    else { pok_value(a, i, k - 2, chal, val, rev); add_product(sum, a, v); }
}
// the weights of row i over its own points A', Abar, d, T1, T2 in the one G1 equation: u z1, -u c, u c + v z3, -u, -v; and t, -t for the two sides of the
// pairing.  st(q, Fr) stores weight q < 7 (a product)
template <class Cc, class F, class ST> FRD void pok_weights(size_t i, const Fr &u, const Fr &v, const Fr &t, Cc chal, F fixed, ST st) {
    Fr c, z, uc, w, one; fr_one(one);
    chal(i, c);
    fixed(i, 0, z); fr_mul(w, z, u); st(0, w);
    fr_mul(uc, c, u);
    neg_product(w, uc); st(1, w);
    fixed(i, 2, z); w = uc; add_product(w, z, v); fr_mul(w, w, one); st(2, w);      // a lazy sum of two products
    neg_product(w, u); st(3, w);
    neg_product(w, v); st(4, w);
    st(5, t);
    neg_product(w, t); st(6, w);
}

// ---- base-field words: nothing but comparisons and one subtraction from p (affine Montgomery words of the ABI; -y of y != 0 is p - y in either form) ----
#define BBSPK_P_WORDS {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau}
FRD bool fq_zero_words(const uint32_t *w, int k) { uint32_t o = 0; for (int i = 0; i < k; i++) o |= w[i]; return o == 0; }
// o = p - y for 0 < y < p; zero stays zero
FRD void fq_neg_words(uint32_t o[FQW], const uint32_t y[FQW]) {
    constexpr uint32_t P_[FQW] = BBSPK_P_WORDS;
    if (fq_zero_words(y, FQW)) { for (int i = 0; i < FQW; i++) o[i] = 0; return; }
    uint64_t br = 0;
    for (int i = 0; i < FQW; i++) { const uint64_t d = (uint64_t)P_[i] - y[i] - br; o[i] = (uint32_t)d; br = (d >> 32) & 1; }
}
// a == -b for two affine points (x | y, 24 words) with flags: both identities, or equal x and y_a + y_b = p
FRD bool g1_is_negation(const uint32_t a[2 * FQW], bool a_inf, const uint32_t b[2 * FQW], bool b_inf) {
    constexpr uint32_t P_[FQW] = BBSPK_P_WORDS;
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
// the first failure of PoKOfSignatureG1Proof::verify in the order it returns them (proof.rs:529-611): 1 ZeroSignature, 2 the first Schnorr check,
// 3 the second, 4 the pairing; 0: verified
FRD uint8_t pok_status(bool a_inf, bool first_ok, bool second_ok, bool pairing_ok) { return a_inf ? 1 : !first_ok ? 2 : !second_ok ? 3 : !pairing_ok ? 4 : 0; }

#if defined(__HIPCC__)
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
using colk::ld_words;
using colk::st_words;
// what the kernels below load: chal: rows x 8 words, fixed: rows x 4 x 8 words (z1 .. z4), vals: rows x L x 8 words packed, rev: rows x L bytes
struct PokIn {
    const uint32_t *__restrict__ chal, *__restrict__ fixed, *__restrict__ vals; const uint8_t *__restrict__ rev; size_t L; bool mont;
    __device__ __forceinline__ void c(size_t i, Fr &x) const { ld_words(x, chal, i, mont); }
    __device__ __forceinline__ void f(size_t i, unsigned t, Fr &x) const { ld_words(x, fixed, i * 4 + t, mont); }
    __device__ __forceinline__ void v(size_t i, size_t j, Fr &x) const { ld_words(x, vals, i * L + j, mont); }
    __device__ __forceinline__ bool r(size_t i, size_t j) const { return rev[i * L + j] != 0; }
};
#define POK_FUNCTORS(in) [&](size_t r_, Fr &x_) { in.c(r_, x_); }, [&](size_t r_, unsigned t_, Fr &x_) { in.f(r_, t_, x_); }, \
                         [&](size_t r_, size_t j_, Fr &x_) { in.v(r_, j_, x_); }, [&](size_t r_, size_t j_) { return in.r(r_, j_); }
// rows[(i * n + k) * 8 ..] = the canonical words (below r) of (c_i, z4_i, y_i1 .. y_iL)_k for i < rows, k < n = L + 2: one lane per entry, the lanes of a row
// neighbours
__global__ void __launch_bounds__(256) k_bbs_pok_rows(PokIn in, size_t rows, size_t n, uint32_t *__restrict__ out_rows) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / n, k = t % n;
    if (i >= rows) return;
    Fr o;
    pok_row_entry(o, i, k, POK_FUNCTORS(in));
    st_words(out_rows, t, o);
}
// own[(i * 7 + t) * 8 ..] = the canonical words of (z1, z2, -c, c, -1 | z3, -1)_t: the scalars of the row's 5-term and 2-term segments, one lane per scalar
__global__ void __launch_bounds__(256) k_bbs_pok_own(PokIn in, size_t rows, uint32_t *__restrict__ own) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / POK_OWN;
    if (i >= rows) return;
    Fr o;
    pok_own_scalar(o, i, (unsigned)(t % POK_OWN), [&](size_t r, Fr &x) { in.c(r, x); }, [&](size_t r, unsigned q, Fr &x) { in.f(r, q, x); });
    st_words(own, t, o);
}
// One lane per (row, slot), slot < 9: the bases of the row's two segments, own[(i * 7 + slot) * 24 ..] = [A', h_0, Abar, d, T1 | d, T2]_slot (slot < 7), and
// the two sides of its pairing, pa[24 i ..] = A' (slot 7), pb[24 i ..] = -Abar (slot 8: y flipped), with skip[i] / skip[rows + i] = that point is the
// identity (zero words).  points: rows x 5 x 24 words in the order A', Abar, d, T1, T2
struct PointWords { uint32_t w[2 * FQW]; };
__global__ void __launch_bounds__(256) k_bbs_pok_stage(const uint32_t *__restrict__ points, PointWords h0, size_t rows, uint32_t *__restrict__ own, uint32_t *__restrict__ pa,
                                                       uint32_t *__restrict__ pb, uint8_t *__restrict__ skip) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = t / 9;
    const unsigned slot = (unsigned)(t % 9);
    if (i >= rows) return;
    const unsigned src = (unsigned)(0x1042321F0ull >> (4 * slot)) & 15u;      // the point of the proof that the slot takes (slot 1: h_0)
    uint32_t w[2 * FQW];
    if (slot == 1) { for (int k = 0; k < 2 * FQW; k++) w[k] = h0.w[k]; }
    else {
        const uint4 *q = reinterpret_cast<const uint4 *>(points + (i * POK_PTS + src) * 2 * FQW);
        for (int k = 0; k < 6; k++) { const uint4 a = q[k]; w[4 * k] = a.x; w[4 * k + 1] = a.y; w[4 * k + 2] = a.z; w[4 * k + 3] = a.w; }
    }
    uint32_t *dst = slot < POK_OWN ? own + (i * POK_OWN + slot) * 2 * FQW : (slot == 7 ? pa : pb) + i * 2 * FQW;
    if (slot >= POK_OWN) skip[(slot - POK_OWN) * rows + i] = fq_zero_words(w, 2 * FQW) ? 1 : 0;
    if (slot == 8) { uint32_t y[FQW]; fq_neg_words(y, w + FQW); for (int k = 0; k < FQW; k++) w[FQW + k] = y[k]; }
    uint4 *o = reinterpret_cast<uint4 *>(dst);
    for (int k = 0; k < 6; k++) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
// One lane per row: seg[(2 i) * 36 ..] is the first check's sum and seg[(2 i + 1) * 36 ..] = Q_i = z3 d - T2 (normalised Jacobian words X | Y | 1) with their
// identity flags seg_inf, b[24 i ..] = P_i with b_inf, pairing[i] the pairing's verdict byte, a_inf[i] = A' is the identity.  The second check holds iff
// Q_i = -P_i.
__global__ void __launch_bounds__(256) k_bbs_pok_verdict(const uint32_t *__restrict__ seg, const uint8_t *__restrict__ seg_inf, const uint32_t *__restrict__ b,
                                                         const uint8_t *__restrict__ b_inf, const uint8_t *__restrict__ pairing, const uint8_t *__restrict__ a_inf, size_t rows,
                                                         uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    uint32_t q[2 * FQW], p[2 * FQW];
    for (int k = 0; k < 2 * FQW; k++) { q[k] = seg[(2 * i + 1) * 3 * FQW + k]; p[k] = b[i * 2 * FQW + k]; }
    status[i] = pok_status(a_inf[i] != 0, seg_inf[2 * i] != 0, g1_is_negation(q, seg_inf[2 * i + 1] != 0, p, b_inf[i] != 0), pairing[i] != 0);
}
// grid (L + 2, blocks): block (k, b) sums column k over the rows [b * 256 * run, ..) of the chunk as k_bbs_col_sums does (a lane's own start powers, a fixed
// tree in LDS, part[(k * gridDim.y + b) * NL ..] in the internal form).  Column 0 also writes the rows' weights as canonical words: w5[(5 i + q) * 8 ..] over the
// own points (q < 5), tp[8 i ..] = rho^(i0 + i), tn[8 i ..] = -rho^(i0 + i)
__global__ void __launch_bounds__(256) k_bbs_pok_col_sums(PokIn in, colk::RhoWords rho_words, size_t rows, size_t i0, size_t run, uint32_t *__restrict__ part,
                                                          uint32_t *__restrict__ w5, uint32_t *__restrict__ tp, uint32_t *__restrict__ tn) {
    const size_t k = blockIdx.x;
    Fr rho;
    fr_from_words(rho, rho_words.w, in.mont);
    colk::col_block_sum(k, rows, run, part, [&](size_t lo, size_t cnt, Fr &sum) {
        pok_col_run(rho, i0 + lo, cnt, k == 0,
                    [&](size_t j, const Fr &u, const Fr &v, Fr &s) { pok_col_term(s, lo + j, k, u, v, POK_FUNCTORS(in)); },
                    [&](size_t j, const Fr &u, const Fr &v, const Fr &tw) {
                        const size_t i = lo + j;
                        pok_weights(i, u, v, tw, [&](size_t r, Fr &x) { in.c(r, x); }, [&](size_t r, unsigned q, Fr &x) { in.f(r, q, x); },
                                    [&](unsigned q, const Fr &x) { if (q < POK_PTS) st_words(w5, i * POK_PTS + q, x); else st_words(q == 5 ? tp : tn, i, x); });
                    },
                    sum);
    });
}
#endif

}  // namespace bbspk
