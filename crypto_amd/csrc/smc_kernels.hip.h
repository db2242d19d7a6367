// crypto_amd/csrc/smc_kernels.hip.h — the scalar and staging half of verifying range proofs over weak-BB signatures in bulk on gfx950 (dock_smc.hip drives it).
//
// Device side of smc_range_proof's CLSRangeProof::verify (cls_range_proof/range_proof_cdh.rs:164-189, :226-256) and CCSArbitraryRangeProof::verify
// (ccs_range_proof/arbitrary_range_cdh.rs:210-250, :311-359) for many proofs of ONE statement: `sides` S = 1 (CLS) or 2 (CCS: min, max), l digits a side, the
// statement's constants w_j (j < l) and (a_s, b_s, e_s) per side.  A proof is a commitment C, a challenge c, per side a point D_s and a response zr_s, and per
// digit d < S l (side-major: d = s l + j) the points A', Abar, T with the responses z1, z2 of short_group_sig/src/weak_bb_sig_pok_cdh.rs.  Its M = S (l + 1)
// equations, each a 4-term segment, in the order the kernels number them (m < M):
//   m = s < S          a_s c C + (b_s c + sum_j w_j z2_sj) g + e_s zr_s h - D_s = O            [C, g, h, D_s] . (a_s c, b_s c + sum_j w_j z2_sj, e_s zr_s, -1)
//   m = S + d          z1_d g1 - z2_d A'_d - c Abar_d - T_d = O                                [g1, A'_d, Abar_d, T_d] . (z1_d, -z2_d, -c, -1)
// and per digit the pairing e(A'_d, pk) e(-Abar_d, g2) = 1.  The scalar field has to
//   write the own scalars where the segmented small MSM reads them, one lane per equation                                k_smc_own
//   one verdict: equation e = i M + m of the batch weighs rho^e, pairing slice i S l + d weighs rho^(i S l + d): the coefficients of the shared points g1, g, h
//   and the weights over the proofs' own points                                                                          k_smc_col_sums, k_col_finish
// and two kernels move words only: k_smc_stage lays the points out for the segment MSM and the pairing (-Abar by a flip of y), k_smc_verdict folds a proof's
// flags into (status, detail).  The per-lane routines are FRD functions over load / store functors, as acc_pok_kernels.hip.h's are: the same text runs on the
// host under -DFP29_CHECK (tests/native/smc_dev_host_shim.cpp).  Operand classes as in col_sums.hip.h: "product" (limbs < 2^29, value < 2 r), "lazy sum"
// (one carry pass after every addition of a product).
//
// Bounds.  The inner product of a side adds b_s c and l <= 64 products w_j z2_sj, a carry pass after each: 65 terms, limbs <= 2^29 + 1, value
// < 130 r — a first operand of fr_mul (limbs < 2^31, value x 2 r far below 2^34 r^2), which reduces it to a product.  A lane's run of COL_RUN = 16
// equations adds at most ONE product per equation to its sum: value < 32 r.  The fixed tree of a block of 256 adds sums of equal depth: after its eight levels
// a slot holds at most 256 x 16 products, value < 2^13 r.  The second pass adds products, one per block, with a carry pass each.  A weight is a product of two
// products; the C of a CCS proof takes the sum of two, carried once (value < 4 r) and reduced by a product with one.
#pragma once
#include "col_sums.hip.h"

namespace smck {
using namespace fr29;
using colk::neg_product;
using colk::pow_start;

constexpr int FQW = 12;           // u32 words of a base-field element
constexpr int MAX_L = 64, MAX_SIDES = 2;
constexpr int EQ_TERMS = 4;       // terms of every equation
constexpr int STMT_CONSTS = 3 * MAX_SIDES;      // the statement on the device: (a, b, e) of side 0, of side 1, then w_0 .. w_(l-1); 8 words each
// the shape of a statement: M equations and S l digits (= pairing slices) a proof
FRD unsigned eq_count(int sides, int l) { return (unsigned)(sides * (l + 1)); }
FRD unsigned digit_count(int sides, int l) { return (unsigned)(sides * l); }
// the position of digit d (side-major) in the order the reference verifies them: CLS j; CCS min[0], max[0], min[1], ..
FRD unsigned ref_position(int sides, int l, unsigned d) { return sides == 1 ? d : 2u * (d % (unsigned)l) + d / (unsigned)l; }

// sum += a b, one carry pass.  a, b: products
FRD void add_product(Fr &sum, const Fr &a, const Fr &b) {
    Fr p; fr_mul(p, a, b);                            // 2 r * 2 r
    fr_add(sum, sum, p); fr_norm(sum, sum);
}
// The four own scalars of equation m of proof i, as products.  chal(i, Fr &), zr(i, s, Fr &), z(i, d, q, Fr &) (q = 0: z1, 1: z2), stmt(k, Fr &) (k < 6 the
// sides' constants, 6 + j the weight w_j) load products
template <class Cc, class Zr, class Z, class St> FRD void own_scalars(Fr o[EQ_TERMS], int sides, int l, size_t i, unsigned m, Cc chal, Zr zr, Z z, St stmt) {
    Fr c, v, one;
    fr_one(one);
    chal(i, c);
    neg_product(o[3], one);
    if (m >= (unsigned)sides) {
        const unsigned d = m - (unsigned)sides;
        z(i, d, 0, o[0]);
        z(i, d, 1, v); neg_product(o[1], v);
        neg_product(o[2], c);
        return;
    }
    Fr k, sum;
    stmt(3 * m, k); fr_mul(o[0], k, c);               // a_s c
    fr_zero(sum);
    stmt(3 * m + 1, k); add_product(sum, k, c);       // b_s c
    for (int j = 0; j < l; j++) { stmt(STMT_CONSTS + j, k); z(i, m * (unsigned)l + (unsigned)j, 1, v); add_product(sum, k, v); }
    fr_mul(o[1], sum, one);                           // 130 r * r
    stmt(3 * m + 2, k); zr(i, m, v); fr_mul(o[2], k, v);      // e_s zr_s
}

// ---- the batch ------------------------------------------------------------------------------------------------------------------------------------------------
// Which shared point an equation's own scalar t multiplies, or -1: a digit's t = 0 is g1's (column 0); a side's t = 1 is g's (1), t = 2 h's (2)
FRD int col_of(bool side, unsigned t) { return side ? (t == 1 ? 1 : t == 2 ? 2 : -1) : (t == 0 ? 0 : -1); }
// One lane's run of column k: the equations [e_lo, e_lo + cnt) of a chunk whose first equation has the batch's exponent e0 (a multiple of M) and whose first
// pairing slice has the exponent p0.  own(e, t, Fr &) loads own scalar t of equation e of the chunk (a product).  The sum of the column's terms u_e own(e, t_k)
// leaves as a product.  The lanes of column 0 (with_weights) also store the weights: wt(kind, index, Fr) with kind 0: over C (index i), 1: over D (i S + s),
// 2: over a digit's points (3 slice + {0, 1, 2}: A', Abar, T), 3 / 4: +- rho^(p0 + slice) for the pairing's sides (slice).  rho: a product.
template <class Own, class WT> FRD void col_run(int sides, int l, const Fr &rho, size_t e0, size_t p0, size_t e_lo, size_t cnt, int k, bool with_weights, Own own, WT wt, Fr &sum) {
    const size_t M = eq_count(sides, l), D = digit_count(sides, l);
    Fr u, t, a, w, one;
    fr_one(one);
    pow_start(u, rho, e0 + e_lo);
    if (with_weights) {                               // the first pairing slice at or after e_lo
        const size_t i = e_lo / M, m = e_lo % M;
        pow_start(t, rho, p0 + i * D + (m < (size_t)sides ? 0 : m - (size_t)sides));
    }
    fr_zero(sum);
    for (size_t j = 0; j < cnt; j++) {
        const size_t e = e_lo + j, i = e / M;
        const unsigned m = (unsigned)(e % M);
        const bool side = m < (unsigned)sides;
        for (unsigned q = 0; q < (unsigned)EQ_TERMS; q++) {
            const int col = col_of(side, q);
            if (col == k) { own(e, q, a); add_product(sum, a, u); }
            if (!with_weights || col >= 0) continue;
            own(e, q, a);
            if (!side) { fr_mul(w, a, u); wt(2, 3 * (i * D + (m - (unsigned)sides)) + (q - 1), w); }
            else if (q == 3) { fr_mul(w, a, u); wt(1, i * (size_t)sides + m, w); }
            else if (m == 0) {                        // C: a_0 c u, and for two sides + a_1 c u rho
                fr_mul(w, a, u);
                if (sides == 2) {
                    Fr u1, w1; fr_mul(u1, u, rho);
                    own(e + 1, 0, a); fr_mul(w1, a, u1);
                    fr_add(w, w, w1); fr_norm(w, w); fr_mul(w, w, one);       // 4 r * r
                }
                wt(0, i, w);
            }
        }
        if (with_weights && !side) {
            const size_t slice = i * D + (m - (unsigned)sides);
            wt(3, slice, t);
            neg_product(w, t); wt(4, slice, w);
            fr_mul(t, t, rho);
        }
        if (j + 1 < cnt) fr_mul(u, u, rho);
    }
    fr_mul(sum, sum, one);
}

// ---- base-field words: one subtraction from p (affine Montgomery words of the ABI; -y of y != 0 is p - y in either form) ----
#define SMCK_P_WORDS {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau}
FRD bool fq_zero_words(const uint32_t *w, int k) { uint32_t o = 0; for (int i = 0; i < k; i++) o |= w[i]; return o == 0; }
// o = p - y for 0 < y < p; zero stays zero
FRD void fq_neg_words(uint32_t o[FQW], const uint32_t y[FQW]) {
    constexpr uint32_t P_[FQW] = SMCK_P_WORDS;
    if (fq_zero_words(y, FQW)) { for (int i = 0; i < FQW; i++) o[i] = 0; return; }
    uint64_t br = 0;
    for (int i = 0; i < FQW; i++) { const uint64_t d = (uint64_t)P_[i] - y[i] - br; o[i] = (uint32_t)d; br = (d >> 32) & 1; }
}
// Where slot `slot` < 6 of equation m takes its point from.  Slots 0 .. 3 are the bases of the segment, 4 and 5 the sides of a digit's pairing (A', then Abar,
// whose y is flipped).  kind 0: shared point `index` (0 g1, 1 g, 2 h); 1: the proof's commitment; 2: its side point `index`; 3: point `index` (0 A', 1 Abar, 2 T)
// of digit m - S; -1: the slot does not exist (a side has no pairing)
struct StageSrc { int kind; unsigned index; };
FRD StageSrc stage_src(int sides, unsigned m, unsigned slot) {
    if (m < (unsigned)sides) {
        if (slot == 0) return StageSrc{1, 0};
        if (slot == 1 || slot == 2) return StageSrc{0, slot};
        if (slot == 3) return StageSrc{2, m};
        return StageSrc{-1, 0};
    }
    if (slot == 0) return StageSrc{0, 0};
    return StageSrc{3, slot < 4 ? slot - 1 : slot - 4};
}
// (status, detail) of one proof in the reference's order of errors.  seg_ok(m): equation m holds; pair_ok(d): digit d's pairing does; a_zero(d): its A' is the
// identity.  1, s + 1: the commitment equation of side s fails (InvalidRangeProof) — it wins over a bad digit; 2, 4 q + k: the digit at position q of the
// reference's order fails its check k (1 A' is the identity, 2 the Schnorr check, 3 the pairing), the smallest 4 q + k; 0, 0: verified.  merged: the digits
// have no pairing of their own (pair_ok is not asked) and the proof's ONE merged check decides last: 3, 0 where it fails (merged_ok)
template <class SO, class PO, class AZ>
FRD void proof_verdict(int sides, int l, bool merged, bool merged_ok, SO seg_ok, PO pair_ok, AZ a_zero, uint8_t &status, int32_t &detail) {
    for (int s = 0; s < sides; s++) if (!seg_ok((unsigned)s)) { status = 1; detail = s + 1; return; }
    int32_t best = 0;
    for (unsigned d = 0; d < digit_count(sides, l); d++) {
        const int k = a_zero(d) ? 1 : !seg_ok((unsigned)sides + d) ? 2 : (!merged && !pair_ok(d)) ? 3 : 0;
        if (!k) continue;
        const int32_t v = 4 * (int32_t)ref_position(sides, l, d) + k;
        if (!best || v < best) best = v;
    }
    if (!best && merged && !merged_ok) { status = 3; detail = 0; return; }
    status = best ? 2 : 0; detail = best;
}
// the weight of digit d in the merged check of a proof: random^d, in the order of the reference's add_sources (side-major).  random: a product
FRD void merge_weight(Fr &t, const Fr &random, unsigned d) { pow_start(t, random, d); }

#if defined(__HIPCC__)
// ---- kernels --------------------------------------------------------------------------------------------------------------------------------------
using colk::ld_words;
using colk::st_words;
// what the kernels below load: chal: rows x 8 words, zr: rows x S x 8, z: rows x S l x 2 x 8, stmt: (6 + l) x 8 (in the caller's form, as the proofs are)
struct ProofIn {
    const uint32_t *__restrict__ chal, *__restrict__ zr, *__restrict__ z, *__restrict__ stmt; int sides, l; bool mont;
    __device__ __forceinline__ void c(size_t i, Fr &x) const { ld_words(x, chal, i, mont); }
    __device__ __forceinline__ void r(size_t i, unsigned s, Fr &x) const { ld_words(x, zr, i * (size_t)sides + s, mont); }
    __device__ __forceinline__ void d(size_t i, unsigned dg, unsigned q, Fr &x) const { ld_words(x, z, (i * digit_count(sides, l) + dg) * 2 + q, mont); }
    __device__ __forceinline__ void k(unsigned j, Fr &x) const { ld_words(x, stmt, j, mont); }
};
// own[(e * 4 + t) * 8 ..] = the canonical words of the own scalars of equation e = i M + m, one lane per equation
__global__ void __launch_bounds__(256) k_smc_own(ProofIn in, size_t rows, uint32_t *__restrict__ own) {
    const unsigned M = eq_count(in.sides, in.l);
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = e / M;
    if (i >= rows) return;
    Fr o[EQ_TERMS];
    own_scalars(o, in.sides, in.l, i, (unsigned)(e % M), [&](size_t r_, Fr &x_) { in.c(r_, x_); }, [&](size_t r_, unsigned s_, Fr &x_) { in.r(r_, s_, x_); },
                [&](size_t r_, unsigned d_, unsigned q_, Fr &x_) { in.d(r_, d_, q_, x_); }, [&](unsigned j_, Fr &x_) { in.k(j_, x_); });
#pragma unroll
    for (int t = 0; t < EQ_TERMS; t++) st_words(own, e * EQ_TERMS + t, o[t]);
}
// One lane per (equation e, slot < 6): the bases of the equation's segment, bases[(e * 4 + slot) * 24 ..] (stage_src), and for a digit the two sides of its
// pairing, pa[24 slice ..] = A', pb[24 slice ..] = -Abar (y flipped), slice = i S l + d, with skip[slice] / skip[slices + slice] = that point is the identity
// (zero words).  commitments: rows x 24 words; side_points: rows x S x 24; digit_points: rows x S l x 3 x 24; shared: g1, g, h
struct SharedPoints { uint32_t w[3][2 * FQW]; };
__global__ void __launch_bounds__(256) k_smc_stage(const uint32_t *__restrict__ commitments, const uint32_t *__restrict__ side_points, const uint32_t *__restrict__ digit_points,
                                                   SharedPoints shared, int sides, int l, size_t rows, uint32_t *__restrict__ bases, uint32_t *__restrict__ pa,
                                                   uint32_t *__restrict__ pb, uint8_t *__restrict__ skip) {
    const unsigned M = eq_count(sides, l), D = digit_count(sides, l);
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, e = t / 6, i = e / M;
    const unsigned slot = (unsigned)(t % 6), m = (unsigned)(e % M);
    if (i >= rows) return;
    const StageSrc src = stage_src(sides, m, slot);
    if (src.kind < 0) return;
    const size_t slice = i * D + (m - (unsigned)sides), slices = rows * D;      // (read for digits only)
    uint32_t w[2 * FQW];
    if (src.kind == 0) { for (int k = 0; k < 2 * FQW; k++) w[k] = shared.w[src.index][k]; }
    else {
        const uint32_t *from = src.kind == 1 ? commitments + i * 2 * FQW : src.kind == 2 ? side_points + (i * (size_t)sides + src.index) * 2 * FQW
                                                                                          : digit_points + (slice * 3 + src.index) * 2 * FQW;
        const uint4 *q = reinterpret_cast<const uint4 *>(from);
        for (int k = 0; k < 6; k++) { const uint4 a = q[k]; w[4 * k] = a.x; w[4 * k + 1] = a.y; w[4 * k + 2] = a.z; w[4 * k + 3] = a.w; }
    }
    uint32_t *dst = slot < 4 ? bases + (e * EQ_TERMS + slot) * 2 * FQW : (slot == 4 ? pa : pb) + slice * 2 * FQW;
    if (slot >= 4) skip[(slot - 4) * slices + slice] = fq_zero_words(w, 2 * FQW) ? 1 : 0;
    if (slot == 5) { uint32_t y[FQW]; fq_neg_words(y, w + FQW); for (int k = 0; k < FQW; k++) w[FQW + k] = y[k]; }
    uint4 *o = reinterpret_cast<uint4 *>(dst);
    for (int k = 0; k < 6; k++) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
// One lane per proof: seg_inf[M i ..] are the identity flags of its segment sums (an equation holds iff its sum is the identity), pairing[S l i ..] the
// pairings' verdict bytes — merged: pairing[i] the ONE merged check's — skip as k_smc_stage wrote it (its first `slices` bytes: A' is the identity)
__global__ void __launch_bounds__(256) k_smc_verdict(const uint8_t *__restrict__ seg_inf, const uint8_t *__restrict__ pairing, const uint8_t *__restrict__ skip, int sides, int l,
                                                     bool merged, size_t rows, uint8_t *__restrict__ status, int32_t *__restrict__ detail) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const size_t M = eq_count(sides, l), D = digit_count(sides, l);
    uint8_t st; int32_t dt;
    proof_verdict(sides, l, merged, merged && pairing[i] != 0, [&](unsigned m) { return seg_inf[i * M + m] != 0; }, [&](unsigned d) { return pairing[i * D + d] != 0; },
                  [&](unsigned d) { return skip[i * D + d] != 0; }, st, dt);
    status[i] = st; detail[i] = dt;
}
// The merged form.  One lane per slice: tw[8 slice ..] = tw[8 (slices + slice) ..] = random_i^d as canonical words — the scalars of the proof's two
// S l-term segments over its staged A' and -Abar.  random: rows x 8 words in the caller's form
__global__ void __launch_bounds__(256) k_smc_merge_weights(const uint32_t *__restrict__ random, int sides, int l, bool mont, size_t rows, uint32_t *__restrict__ tw) {
    const size_t D = digit_count(sides, l), slices = rows * D, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= slices) return;
    Fr rnd, w;
    ld_words(rnd, random, t / D, mont);
    merge_weight(w, rnd, (unsigned)(t % D));
    st_words(tw, t, w); st_words(tw, slices + t, w);
}
// One lane per (proof, side): the merged points of the proofs as the segment MSM left them — sums[36 j ..] normalised (x, y, z), inf[j] their identity
// flags, j = i the sum over A', j = rows + i the sum over -Abar — as the pairing's operands: pa / pb[24 i ..] (the identity: zero words), skip[i] / skip[rows + i]
__global__ void __launch_bounds__(256) k_smc_merged_sides(const uint32_t *__restrict__ sums, const uint8_t *__restrict__ inf, size_t rows, uint32_t *__restrict__ pa,
                                                          uint32_t *__restrict__ pb, uint8_t *__restrict__ skip) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2 * rows) return;
    const bool z = inf[j] != 0;
    const uint4 *q = reinterpret_cast<const uint4 *>(sums + j * 3 * FQW);
    uint4 *o = reinterpret_cast<uint4 *>((j < rows ? pa + j * 2 * FQW : pb + (j - rows) * 2 * FQW));
    for (int k = 0; k < 6; k++) o[k] = z ? make_uint4(0, 0, 0, 0) : q[k];
    skip[j] = z ? 1 : 0;
}
// grid (3, blocks): block (k, b) sums column k over the equations [b * 256 * run, ..) of the chunk's rows * M (a lane's own start powers, a fixed tree in LDS,
// part[(k * gridDim.y + b) * NL ..] in the internal form).  Column 0 also writes the weights as canonical words: w_side[8 i ..] over C, w_side[8 (rows + i S + s) ..]
// over D, w_digit[8 (3 slice + q) ..] over A', Abar, T, tp / tn[8 slice ..] = +- rho^(p0 + slice).  own: k_smc_own's output
__global__ void __launch_bounds__(256) k_smc_col_sums(const uint32_t *__restrict__ own, colk::RhoWords rho_words, int sides, int l, bool mont, size_t rows, size_t e0, size_t p0, size_t run,
                                                      uint32_t *__restrict__ part, uint32_t *__restrict__ w_side, uint32_t *__restrict__ w_digit, uint32_t *__restrict__ tp,
                                                      uint32_t *__restrict__ tn) {
    const int k = (int)blockIdx.x;
    Fr rho;
    fr_from_words(rho, rho_words.w, mont);
    colk::col_block_sum((size_t)k, rows * eq_count(sides, l), run, part, [&](size_t lo, size_t cnt, Fr &sum) {
        col_run(sides, l, rho, e0, p0, lo, cnt, k, k == 0, [&](size_t e, unsigned q, Fr &x) { ld_words(x, own, e * EQ_TERMS + q, false); },
                [&](int kind, size_t idx, const Fr &x) {
                    if (kind == 0) st_words(w_side, idx, x); else if (kind == 1) st_words(w_side, rows + idx, x); else if (kind == 2) st_words(w_digit, idx, x);
                    else st_words(kind == 3 ? tp : tn, idx, x);
                },
                sum);
    });
}
#endif

}  // namespace smck
