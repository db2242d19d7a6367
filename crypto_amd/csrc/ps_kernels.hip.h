// crypto_amd/csrc/ps_kernels.hip.h — the scalar half of Pointcheval-Sanders (Coconut) signatures in bulk on gfx950 (dock_ps.hip drives it).
//
// Device side of Signature::new and Signature::verify (coconut/src/signature/ps_signature.rs:46-64, 95-142) and of SignaturePoK::verify
// (coconut/src/proof/signature_pok/proof.rs:32-56) for many rows under one key.  The public key is ONE G2 base set [alpha_tilde, beta_tilde_1 .. beta_tilde_L,
// g_tilde]; every group operation runs in kernels the library already has (the many-row MSM, k_mul_add_g2_gls, the line kernels), and what the scalar field has to
// do is to write scalars where those kernels read them:
//   sign        r_i and u_i = r_i (x + sum_j y_j m_ij), the two fixed-base scalars of (sigma_1, sigma_2) = (r g, u g)              k_ps_sign_rows
//   verify      the row (1, m_i1 .. m_iL) over pk[0 .. L]: Q_i = alpha_tilde + sum_j m_ij beta_tilde_j                            k_bbs_rows with ONE fixed column
//                                                                                                                                (bbs_kernels.hip.h: the same row)
//   one verdict the weights w_i = rho^i, the products w_i m_ij and -w_i, column-major: L + 2 scalar vectors over the signatures     k_ps_col_scalars
//   proof       two rows of L + 2 entries per proof over the whole key: S_i = (0, hidden ? z_ij : 0 .., z_r,i) and
//               R_i = (1, revealed ? m_ij : 0 .., 0)                                                                              k_ps_pok_rows
//               the Schnorr comparison, the identity flags and the pairing byte into a status                                     k_ps_verdict
// Blocks are 256 independent lanes; scalars move as two 16-byte words (col_sums.hip.h ld_words / st_words).  The per-lane routines are FRD functions over
// load / store functors: the same text runs on the host under -DFP29_CHECK, where every product asserts its operand contract
// (tests/native/ps_dev_host_shim.cpp).  Operand classes as in col_sums.hip.h: "product" (limbs < 2^29, value < 2 r), "lazy sum" (one carry pass after every
// addition of a product: limbs <= 2^29 + 3 below the top limb, value < 2 r per term).
//
// Bounds.  u_i's inner sum is x plus L products, a lazy sum of L + 1 terms: value < 2 (L + 1) r, the top limb < (L + 1) / 32 + 1.  It enters
// fr_mul as the first operand (limbs < 2^31) against one (value < r): 2 (L + 1) r^2 < 2^34 r^2 for every L < 2^33 - 1; the ABI refuses L >= 2^31 - 2.  A carry pass
// after every term, not one per sixteen: a product's limbs are up to 2^29 - 1, so seven of them on top of a normalised limb reach 2^32 and wrap the 32-bit limb;
// at most six terms could share a pass, and a pass is nine shifts and adds against the hundred multiply-adds of the product in front of it.  The weights of the
// batch are products of products; -w_i goes through neg_product (512 r - v < 514 r as a first operand).
#pragma once
#include "bbs_routines.hip.h"

namespace psk {
using namespace fr29;
using colk::neg_product;
using colk::pow_start;

constexpr int G2W = 48;           // u32 words of an affine G2 point of the ABI

// u = r (x + sum_j y_j m_j).  r: a product; x(Fr &), y(j, Fr &), m(j, Fr &) load products.  u: a product
template <class X, class Y, class M> FRD void sign_scalar(Fr &u, const Fr &r, size_t L, X x, Y y, M m) {
    Fr sum, a, b, p, one; fr_one(one);
    x(sum);
    for (size_t j = 0; j < L; j++) {
        y(j, a); m(j, b);
        fr_mul(p, a, b);                              // 2 r * 2 r
        fr_add(sum, sum, p); fr_norm(sum, sum);
    }
    fr_mul(sum, sum, one);                            // 2 (L + 1) r * r
    fr_mul(u, sum, r);                                // 2 r * 2 r
}
// entry k < L + 2 of the rows of proof i.  which = 0: S_i = (0, hidden ? z_ij : 0 .., z_r,i); which = 1: R_i = (1, revealed ? m_ij : 0 .., 0).
// val(i, j, Fr &) loads values[i][j], resp(i, Fr &) the last response (products); rev(i, j) is the mask byte
template <class V, class Rs, class Rv> FRD void pok_row_entry(Fr &o, int which, size_t i, size_t k, size_t L, V val, Rs resp, Rv rev) {
    fr_zero(o);
    if (k == 0) { if (which) fr_one(o); return; }
    if (k == L + 1) { if (!which) resp(i, o); return; }
    if (rev(i, k - 1) == (which != 0)) val(i, k - 1, o);
}
// One lane's run of column k < L + 2 of the batch: out(j, Fr) takes the scalar of the run's j-th row, j < cnt, under the weight w = rho^(e0 + j) — column 0: w;
// column k in 1 .. L: w m_(k-1); column L + 1: -w.  m(j, Fr &) loads the message of the run's j-th row in this column (a product).  rho: a product
template <class M, class ST> FRD void col_scalars(const Fr &rho, size_t e0, size_t cnt, size_t k, size_t L, M m, ST out) {
    Fr w, v, o;
    pow_start(w, rho, e0);
    for (size_t j = 0; j < cnt; j++) {
        if (k == 0) o = w;
        else if (k == L + 1) neg_product(o, w);
        else { m(j, v); fr_mul(o, v, w); }            // 2 r * 2 r
        out(j, o);
        if (j + 1 < cnt) fr_mul(w, w, rho);
    }
}
// a == b for two affine G2 points (48 canonical Montgomery words each) with flags: both identities, or neither and equal words.  An identity may come as a
// flag or as zero words.  a(q, w) / b(q, w) load the four words 4 q .. 4 q + 3 of the point, q < 12: the points stream through, twelve 16-byte loads each
template <class A, class B> FRD bool g2_equal(A a, bool a_inf, B b, bool b_inf) {
    uint32_t diff = 0, anya = 0, anyb = 0;
    for (int q = 0; q < G2W / 4; q++) {
        uint32_t x[4], y[4]; a(q, x); b(q, y);
        for (int k = 0; k < 4; k++) { diff |= x[k] ^ y[k]; anya |= x[k]; anyb |= y[k]; }
    }
    a_inf = a_inf || !anya; b_inf = b_inf || !anyb;
    if (a_inf || b_inf) return a_inf && b_inf;
    return diff == 0;
}
// the first failure in the order SignaturePoK::verify returns them (proof.rs:46-55: proof_res.and(sig_res)) under crypto_amd.bbs_plus.STATUS's numbers: 3 the
// Schnorr check (this protocol's only one), 1 ZeroSignature, 4 PairingCheckFailed; 0: verified.  2 is never returned
FRD uint8_t status_of(bool schnorr_ok, bool sigma_1_inf, bool sigma_2_inf, bool pairing_ok) {
    return !schnorr_ok ? 3 : (sigma_1_inf || sigma_2_inf) ? 1 : !pairing_ok ? 4 : 0;
}

#if defined(__HIPCC__)
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
using colk::ld_words;
using colk::st_words;
// One lane per row: out[16 i ..] = r_i, out[16 i + 8 ..] = u_i as canonical words (below r), the order (sigma_1_i, sigma_2_i) leaves the fixed-base kernel in.
// sk: (1 + L) x 8 words (x, y_1 .. y_L), r: rows x 8 words, msgs: rows x L x 8 words packed, all in the caller's form (mont)
__global__ void __launch_bounds__(256) k_ps_sign_rows(const uint32_t *__restrict__ sk, const uint32_t *__restrict__ r, const uint32_t *__restrict__ msgs, int mont, size_t rows, size_t L,
                                                      uint32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    Fr ri, u;
    ld_words(ri, r, i, mont != 0);
    sign_scalar(u, ri, L, [&](Fr &x) { ld_words(x, sk, 0, mont != 0); }, [&](size_t j, Fr &x) { ld_words(x, sk, 1 + j, mont != 0); },
                [&](size_t j, Fr &x) { ld_words(x, msgs, i * L + j, mont != 0); });
    st_words(out, 2 * i, ri); st_words(out, 2 * i + 1, u);
}
// what the proof kernels load: resp: rows x 8 words, vals: rows x L x 8 words packed, rev: rows x L bytes
struct PokIn {
    const uint32_t *__restrict__ resp, *__restrict__ vals; const uint8_t *__restrict__ rev; size_t L; bool mont;
};
// One lane per entry: out_rows[((which * rows + i) * n + k) * 8 ..] = entry k < n = L + 2 of row `which` of proof i (pok_row_entry) as canonical words: the
// S rows of the chunk first, then its R rows — 2 rows MSM rows in all
__global__ void __launch_bounds__(256) k_ps_pok_rows(PokIn in, size_t rows, uint32_t *__restrict__ out_rows) {
    const size_t n = in.L + 2, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, row = t / n, k = t % n;
    if (row >= 2 * rows) return;
    const int which = row >= rows ? 1 : 0;
    Fr o;
    pok_row_entry(o, which, row - (which ? rows : 0), k, in.L, [&](size_t i, size_t j, Fr &x) { ld_words(x, in.vals, i * in.L + j, in.mont); },
                  [&](size_t i, Fr &x) { ld_words(x, in.resp, i, in.mont); }, [&](size_t i, size_t j) { return in.rev[i * in.L + j] != 0; });
    st_words(out_rows, t, o);
}
// grid (L + 2, blocks): lane t of block (k, b) writes the `run` rows from (b * 256 + t) * run on of column k, with a start power of its own:
// cols[(k * cstride + i) * 8 ..] = the column's scalar of row i of the chunk (col_scalars), canonical words.  msgs: rows x L x 8 words packed; i0: the chunk's
// first row in the batch
__global__ void __launch_bounds__(256) k_ps_col_scalars(const uint32_t *__restrict__ msgs, colk::RhoWords rho_words, int mont, size_t rows, size_t L, size_t i0, size_t run,
                                                        size_t cstride, uint32_t *__restrict__ cols) {
    const size_t k = blockIdx.x, lo = ((size_t)blockIdx.y * 256 + threadIdx.x) * run;
    if (lo >= rows) return;
    const size_t cnt = rows - lo < run ? rows - lo : run;
    Fr rho;
    fr_from_words(rho, rho_words.w, mont != 0);
    col_scalars(rho, i0 + lo, cnt, k, L, [&](size_t j, Fr &v) { ld_words(v, msgs, (lo + j) * L + (k - 1), mont != 0); },
                [&](size_t j, const Fr &o) { st_words(cols, k * cstride + lo + j, o); });
}
// One lane per row: got[48 i ..] = S_i + (-c_i) k_i with its identity flag got_inf, t[48 i ..] the proof's commitment (zero words: the identity); sig: the
// rows' sigma_1' (rows x 24 words) followed by their -sigma_2' (zero words: the identity); pairing[i] the pairing's verdict byte
__global__ void __launch_bounds__(256) k_ps_verdict(const uint32_t *__restrict__ got, const uint8_t *__restrict__ got_inf, const uint32_t *__restrict__ t, const uint32_t *__restrict__ sig,
                                                    const uint8_t *__restrict__ pairing, size_t rows, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const uint4 *qa = reinterpret_cast<const uint4 *>(got + i * G2W), *qb = reinterpret_cast<const uint4 *>(t + i * G2W);
    auto words = [](const uint4 *p) { return [p](int q, uint32_t w[4]) { const uint4 v = p[q]; w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }; };
    const bool schnorr_ok = g2_equal(words(qa), got_inf[i] != 0, words(qb), false);
    const uint4 *s1 = reinterpret_cast<const uint4 *>(sig + i * 24), *s2 = reinterpret_cast<const uint4 *>(sig + (rows + i) * 24);
    uint32_t any1 = 0, any2 = 0;
    for (int q = 0; q < 6; q++) { const uint4 a = s1[q], b = s2[q]; any1 |= a.x | a.y | a.z | a.w; any2 |= b.x | b.y | b.z | b.w; }
    status[i] = status_of(schnorr_ok, !any1, !any2, pairing[i] != 0);
}
#endif

}  // namespace psk
