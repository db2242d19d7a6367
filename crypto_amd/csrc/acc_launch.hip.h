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
// table_words: acc_table_entries() x 8 words, ark-ff Montgomery form: [a | F | r | G | Phi] -> tab (x 10 words)
void launch_acc_prep(hipStream_t s, const uint32_t *table_words, size_t entries, uint32_t *tab);
// elems: m x 8 words (mont: ark-ff Montgomery form, else any 256-bit value).  fg: f (m x 8 canonical words), then g (the same).
void launch_acc_factors(hipStream_t s, const uint32_t *tab, size_t n_add, size_t n_rem, const uint32_t *elems, int mont, size_t m, AccShape sh,
                        uint32_t *part, uint32_t *scratch, uint32_t *fg);
}  // namespace acck
