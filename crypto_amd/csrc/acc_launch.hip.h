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
}  // namespace acck
