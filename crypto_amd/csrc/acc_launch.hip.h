// crypto_amd/csrc/acc_launch.hip.h — host-callable launchers of the accumulator witness-update kernels (k_acc.hip, acc_kernels.hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace acck {
// How a call is cut.  All three constants are UNMEASURED (tests/perf/acc_update_timing.py reports what they would be tuned from):
//   ACC_FILL_LANES   lanes that fill the device: 256 CUs x 4 SIMDs x one wave of 64.  With at least this many elements every element's passes run whole (K = 1).
//   ACC_MIN_CHUNK    entries of the longer list per chunk, at least: a chunk costs four products per entry, its combination four more and a round trip of
//                    160 bytes, so at 32 entries the split adds about 3 % of work.
//   ACC_SHARE_LANES  beyond this many elements a lane of the finishing step takes several (one Fermat inversion, ~430 products, per lane): at most 32.
constexpr size_t ACC_FILL_LANES = 65536, ACC_MIN_CHUNK = 32, ACC_SHARE_LANES = 131072, ACC_MAX_SPLIT = 4096;
struct AccShape { uint32_t K; size_t G; };      // chunks per element, lanes of the finishing step
// forced_split: 0 = automatic, else the chunk count (1 .. ACC_MAX_SPLIT)
AccShape acc_shape(size_t m, size_t n_add, size_t n_rem, int forced_split);
// workspace of a call, in bytes (each a multiple of 256): the tables as words and in internal form, the chunk results, the scratch slots
size_t acc_table_entries(size_t n_add, size_t n_rem);
size_t acc_part_bytes(size_t m, AccShape sh);
size_t acc_scratch_bytes(size_t m);
// table_words: acc_table_entries() x 8 words, ark-ff Montgomery form: [a | F | r | G | Phi] -> tab (x 10 words).  mont = 0: the words are canonical
// (the public lists of the holders' update, as the caller gave them)
void launch_acc_prep(hipStream_t s, const uint32_t *table_words, size_t entries, uint32_t *tab, int mont = 1);
// elems: m x 8 words (mont: ark-ff Montgomery form, else any 256-bit value).  fg: f (m x 8 canonical words), then g (the same).
void launch_acc_factors(hipStream_t s, const uint32_t *tab, size_t n_add, size_t n_rem, const uint32_t *elems, int mont, size_t m, AccShape sh,
                        uint32_t *part, uint32_t *scratch, uint32_t *fg);
// Omega: v_AD at the N points pts (the transform's form, limb-major) -> ev (the same form).  sh = acc_shape(N, ..); part as above with m = N.
void launch_acc_omega_eval(hipStream_t s, const uint32_t *tab, size_t n_add, size_t n_rem, const uint32_t *pts, size_t N, AccShape sh, uint32_t *part, uint32_t *ev);
// coefficient k < len = ev[rev k] / N (ninv_words: 1 / N, canonical) as canonical words, and nz[k] = (it is not zero).  ev: the inverse transform's
// bit-reversed output for logn >= 2, the values themselves for logn = 0 and 1 (the transform of size two runs here)
void launch_acc_omega_coeffs(hipStream_t s, const uint32_t *ev, int logn, const uint32_t ninv_words[8], size_t len, uint32_t *coeff, uint8_t *nz);
// the public update.  lists: [a | r] in internal form (launch_acc_prep).  fs: f (m x 8 canonical words), then s = 1 / d_D; ok[i] = (d_D(y_i) != 0).
// part: acc_part_bytes(m, sh) serve (two results per chunk, not four)
void launch_acc_pub_factors(hipStream_t s, const uint32_t *lists, size_t n_add, size_t n_rem, const uint32_t *elems, int mont, size_t m, AccShape sh,
                            uint32_t *part, uint32_t *scratch, uint32_t *fs, uint8_t *ok);
// UNMEASURED: powers per lane of k_acc_pub_rows.  A lane pays at most 2 log2(n) products for its start power, then two per entry (the product and the
// conversion to words): at 32 the start costs at most 26 products against 64
constexpr size_t ACC_ROW_RUN = 32;
// rows x n canonical words-of-8, packed: row i = s_i y_i^j (elems / s_words: the first holder of the chunk)
void launch_acc_pub_rows(hipStream_t s, const uint32_t *elems, int mont, const uint32_t *s_words, size_t rows, size_t n, uint32_t *out_rows);

// ---- issuing witnesses: d_i = prod_j (member_j - y_i) over the whole accumulator, then the scalars of the window-table multiplication ----
//   ACC_D_PASS       members per pass when they come from the host: 32 MB of words and 40 MB of internal form in the slot's workspace.  UNMEASURED.
//   ACC_D_UNROLL_MIN non-members from which a lane may own four of them (k_acc_d<4>): four waves' worth, so that the lanes of the four-fold form still fill
//                    a wave; below, one per lane (k_acc_d<1>).  UNMEASURED.
//   ACC_D_UNROLL_MIN_CHUNK   ... and only when the chunks of the four-fold form hold at least this many members.  Four times fewer lanes mean four times as
//                    many chunks to reach ACC_FILL_LANES; with short chunks their combination and the lower occupancy (3 waves per SIMD against 5) cost more
//                    than the shared loads save.  Measured (profiles/acc_issue_timing.json): chunks of 64 lose 40 % to the one-fold form,
//                    256 tie, 1024 and more win 15 - 21 %; 512 itself was not measured.
//   ACC_FILL_LANES / ACC_MIN_CHUNK are reused as they stand: acc_shape(lanes, members of the pass, 0, forced) cuts the pass into chunks.  UNMEASURED for this kernel.
constexpr size_t ACC_D_PASS = (size_t)1 << 20, ACC_D_UNROLL_MIN = 4 * 64, ACC_D_UNROLL_MIN_CHUNK = 512;
inline size_t acc_d_lanes(size_t m, int U) { return (m + (size_t)U - 1) / (size_t)U; }
// non-members per lane for m non-members against passes of n members: forced (1 or 4), or 0 = automatic by the constants above (forced_split as acc_shape takes it)
inline int acc_d_unroll(size_t m, size_t n, int forced, int forced_split) {
    if (forced == 1 || forced == 4) return forced;
    if (m < ACC_D_UNROLL_MIN) return 1;
    return n / acc_shape(acc_d_lanes(m, 4), n, 0, forced_split).K >= ACC_D_UNROLL_MIN_CHUNK ? 4 : 1;
}
size_t acc_d_part_bytes(size_t m, uint32_t K);        // chunk products (K > 1), a multiple of 256
size_t acc_d_run_bytes(size_t m);                     // the running products between passes
// One pass: tab = the n members of the pass in internal form (launch_acc_prep), elems = the m non-members (m x 8 words; mont: ark-ff Montgomery form), K chunks
// (acc_shape(acc_d_lanes(m, U), n, 0, forced).K).  first: the running product starts from d_in (m x 8 words in the caller's form, or NULL: one), else from run;
// last: d_words (m x 8 words in the caller's form) and nz[i] = (d_i != 0) are written, else run.
void launch_acc_d(hipStream_t s, const uint32_t *tab, size_t n, const uint32_t *elems, int mont, size_t m, int U, uint32_t K, const uint32_t *d_in, bool first, bool last,
                  uint32_t *part, uint32_t *run, uint32_t *d_words, uint8_t *nz);
// sc: m x 8 canonical words: (f_V - d_i) t_i (d_words != NULL; d_words and fv_words in the caller's form) or t_i; t_words: ark-ff Montgomery words.
// zero[i] = (d_i is zero)
void launch_acc_issue_scalars(hipStream_t s, const uint32_t *d_words, const uint32_t *t_words, const uint32_t fv_words[8], int mont, size_t m, uint32_t *sc, uint8_t *zero);
}  // namespace acck
