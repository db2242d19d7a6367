/* include/dock_gpu_dev.h — DEVELOPMENT surface of the MI355X backend: tuning knobs of the kernels, stage timers, self-test and fault-injection
 * hooks.  Served by crypto_amd/libdock_gpu_dev.so only — the twin of the product library built from the same objects plus
 * crypto_amd/csrc/dock_dev.hip (and dock_core.hip compiled -DDGPU_DEV).  The product library libdock_gpu.so (include/dock_gpu.h: what a Rust host
 * binds) exports none of these; tests/, tools/ and the stage / roofline leg of bench.py load the twin.
 *
 * Every knob returns the SAME result limb for limb at any setting (the parity tests sweep each of them against the automatic choice); the defaults
 * are the measured optima on MI355X.  Process-wide. */
#ifndef DOCK_GPU_DEV_H
#define DOCK_GPU_DEV_H
#include "dock_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* window width c (bits) used by the bucket method; 0 = automatic from n.  Any value gives the same point. */
int32_t dgpu_set_window_bits(int32_t c);
/* terms per lane of the bucket accumulation (16..4096; 0 = automatic).  Any value gives the same point (tests sweep it). */
int32_t dgpu_set_chunk(int32_t terms);
/* rows per launch of dgpu_msm_g*_handle_many (1..65535; 0 = automatic from the row length: 2^17 terms' worth, at most 4096 rows).  Any value gives the
 * same rows (tests compare chunked against unchunked). */
int32_t dgpu_set_many_chunk_rows(int32_t rows);
/* dgpu_msm_g*_segments: fold = 0 the per-segment fold by the chunk's segment count, 1 always the host threads' host_fold, 2 always k_seg_fold on the device;
 * chunk_terms = terms per chunk (1 .. 2^20; 0 = automatic, 2^16; a segment longer than the limit travels alone).  Any setting gives the same words (tests
 * cross chunk boundaries with small inputs and compare both folds). */
int32_t dgpu_set_msm_segments(int32_t fold, int32_t chunk_terms);
/* Geometry of dgpu_fp12_pow_batch, dgpu_fp12_multi_pow_device and dgpu_gt_in_subgroup_device, and of nothing else (the final-exponentiation
 * launchers keep their own rule): groups of six lanes per wave (1..10), bases per group of the product of powers (1..8; the batch form always takes one), elements per chunk
 * (1..65536; the power table takes 5.4 KB per element).  0 = automatic: by the launch's group count, n / 2048 clamped to 1..8 (provisional until
 * tests/perf/gt_pow_timing.py's sweep has run), 16384.  Any setting gives the same bytes. */
int32_t dgpu_set_gt_pow(int32_t groups_per_wave, int32_t bases_per_group, int32_t chunk_elems);
/* dgpu_witness_map_r1cs_many: rows per chunk (1..4096; 0 = automatic: at most 4096 rows, 2^17 domain elements, 2^21 assignment scalars) and statements per
 * block of the block kernel (1..512, clamped to 2^10 / D, the most a block's LDS holds; 0 = automatic: 256 / D for D <= 128, else 1; both provisional until
 * tests/perf/witness_map_many_timing.py has run).  Any setting gives the same bytes (tests cross chunk and block boundaries at small m). */
int32_t dgpu_set_wm_many(int32_t chunk_rows, int32_t rows_per_block);
/* dgpu_accumulator_update_*: chunks per element of the two passes (1..4096; 0 = automatic: 1 when the elements alone fill the device, else enough chunks of
 * at least 32 list entries to reach 65536 lanes — both constants unmeasured until tests/perf/acc_update_timing.py has run).  Any value gives the same words
 * (tests force 1, 2 and 5 at small shapes).  dgpu_dev_get_acc_split returns the chunk count the process's last call ran with (0: none yet).
 * The public-information pair cuts its passes by the same knob: dgpu_accumulator_omega_g1 per evaluation point, dgpu_accumulator_update_witnesses_public_g1
 * per holder. */
int32_t dgpu_dev_set_acc_split(int32_t chunks);
int32_t dgpu_dev_get_acc_split(void);
/* dgpu_accumulator_d_for_batch[_resident]: members per pass (1 .. 2^31 - 1; 0 = automatic: 2^20, unmeasured) — tests make 33 members take five passes — and
 * non-members per lane of k_acc_d (1 or 4; 0 = automatic: 4 from 256 non-members on when the chunks then hold at least 512 members; tests/perf/acc_issue_timing.py
 * compares the two).  The chunks
 * per pass follow dgpu_dev_set_acc_split.  Any setting gives the same words.  dgpu_dev_get_acc_d_unroll returns the non-members per lane the process's last
 * call ran with (0: none yet). */
int32_t dgpu_dev_set_acc_d_pass(int32_t entries);
int32_t dgpu_dev_set_acc_d_unroll(int32_t non_members_per_lane);
int32_t dgpu_dev_get_acc_d_unroll(void);
/* Route of the witness map's transforms (crypto_amd/csrc/k_ntt.hip run_passes).  path = 0: automatic — one k_ntt_stage launch per stage below 2^10, the piped
 * k_ntt_r4 passes with the (ab - c) / Z step and the coset epilogue fused into the first / last pass for 2^10 .. 2^26, k_ntt_fused (2^11-element tiles, groups
 * of up to 7 stages) with the separate k_pointwise / k_coset_scale above (arrays beyond 4 GB).  path = 1: one launch per stage with the separate k_coset_scale /
 * k_pointwise at every size.  path = 2: k_ntt_fused with the separate epilogue — what domains above 2^26 run — for every domain of at least 2^11 elements (one
 * tile); smaller domains keep the automatic route.  split / n_split: stage counts of the piped passes in decimation-in-frequency order (the strided passes, then
 * the flat one; the forward transform runs them reversed), 1 .. 10 stages each, at most 12 entries; a split applies only to domains whose log2 equals its sum
 * and only on the piped route; n_split = 0 clears it.  Flat passes of fewer than 6 stages and strided passes whose columns are less than a tile's width apart
 * never occur automatically; k_ntt_r4 handles them (tests force 5,5,5,1 and its like to imitate the three strided passes of 2^23 .. 2^26 at small sizes).
 * DGPU_E_BADARG, with the previous setting left in place, for anything else.  Any setting gives the same bytes (tests/test_gpu_ntt_paths.py compares every
 * route with the CPU oracle).
 * dgpu_dev_get_ntt_last: *path = the route of the last transform the process launched (0 piped, 1 per stage, 2 staged), groups[0 .. min(cap, n)) = its stage
 * groups in launch order (per stage: n = log2 D ones); returns n (0: no transform yet). */
int32_t dgpu_dev_set_ntt(int32_t path, const int32_t *split, int32_t n_split);
int32_t dgpu_dev_get_ntt_last(int32_t *path, int32_t *groups, int32_t cap);
/* What the accumulate stage of the last bucket MSM decided on the device (crypto_amd/csrc/dyn_chunk.hip.h, msm_kernels.hip.h K5 / K6), read back after the call
 * has returned: out[0] = terms per chunk CH, out[1] = chunks with work T, out[2] = the heavy threshold 16 CH (a bucket of at least that many terms is folded by a
 * block, k_fixup_heavy), out[3] = the sorted (bucket, term) pairs E, out[4] = heavy buckets of more than 512 pieces (folded range by range: k_fixup_heavy_ranges /
 * _join), out[5] = heavy buckets in all (those of out[4] included).  Read only: it copies the words the call left in its slot's workspace, which only grows.
 * WHICH slot: the calling thread's context hands its slots out in turn, and this reads the one handed out last — the last call's as long as calls are made one at
 * a time on one context (what tests/test_gpu_heavy_buckets.py does); with calls in flight side by side, or after a call that takes a slot without accumulating
 * (an upload, dgpu_scalars_sort, an MSM on the bucket-free small path), it reads another call's leftovers or fails.  A call of 2^19 terms or more with host
 * scalars runs two term ranges and leaves the second one's words.  DGPU_E_BADARG: out is NULL, no call has taken a slot yet, or that slot's workspace holds no
 * consistent words (no accumulation has run on it). */
int32_t dgpu_dev_get_acc_last(uint32_t out[6]);
/* Bits of the table fingerprints of the SAVER keys created from now on (dgpu_saver_dk_create of include/dock_gpu_saver.h: libdock_gpu_saver_dev.so serves both; existing keys keep theirs): 1 .. 63 keeps the low bits, 0 restores
 * all 64, -1 keeps none, so that a whole column is ONE run of equal fingerprints.  Any setting gives the same chunks: the fingerprint only finds candidates
 * (tests make runs exist by pigeonhole with 3 bits at b = 4). */
int32_t dgpu_dev_set_saver_fp_bits(int32_t bits);
/* log2 of the buckets one lane of the bucket reduction sums serially on the table pipeline (0..6; -1 = automatic: 3 for a 2^19-bucket table when the
 * call runs alone, 4 when three or more calls are in flight on the device context).  Any value gives the same point. */
int32_t dgpu_set_reduce_shift(int32_t log2_buckets_per_lane);
/* form of the bucket reduction.  0 (default): the shared bucket set of the table pipeline by bit marginals (crypto_amd/csrc/reduce_kernels.hip.h:
 * one butterfly network per wave, class folds with four members per value; the plain pipeline's per-window reduction then runs as 4); 2: the same with
 * one lane per value in the class folds; 4 / 1: the scan form of rounds 1-4 (k_reduce_l0, then k_reduce_top_quad / k_reduce_top). */
int32_t dgpu_set_reduce_lanes(int32_t lanes);
/* Forms of the Miller-loop kernels, a bit mask (default 31).  Bit 0: dgpu_multi_miller_loop of up to 8192 pairs runs its line kernel in pieces
 * and overlaps the products / host share of a finished piece with the next (and dgpu_g2_prepare runs the same lanes-per-point chain
 * followed by a parallel conversion pass).  Bit 1: the product tree gives every node 18 lane pairs (one Fp2 product deep per level) instead
 * of three.  Bit 2: up to 4096 pairs the line kernel gives every (P, Q) sixteen lanes (a doubling step two Fp2 operations deep instead of
 * five).  Bit 3 (with bit 2): those sixteen lanes are four lanes in each of four waves, a wave per role (k_miller_lines_ws).  Bit 4: the sparse
 * products of a launch of up to 512 blocks run as three waves per 32 slices (k_line_products3).  Every combination gives the same Fp12 value
 * limb for limb (tests compare all 32).  Upper bits, zero = the default: bits 8-13 / 16-21 the bits of |x| at which the chain is cut into three
 * launches (40 and 17), bits 24-27 the slice length of the last piece's sparse products, bits 28-29 log2 of a factor on bit 4's block limit
 * (tools/dev/ml_cuts_sweep.py, ml_tail_sweep.py, ml_lp3_limit.py).  DGPU_E_BADARG for anything else. */
int32_t dgpu_set_miller_pipeline(int32_t mode);

/* ---- instrumentation (bench.py's stage breakdown and roofline leg; rocprofv3 cross-check) ----
 * When enabled, every stage of the next calls is bracketed by HIP events on the library's own stream. */
int32_t dgpu_prof_enable(int32_t on);
int32_t dgpu_prof_reset(void);
/* fills up to `cap` entries; returns the number of stages recorded.  names[i] points to a static string.  The last row, "hipMalloc", is
 * always present: calls = device allocations since dgpu_prof_reset (0 in steady state), total_ms = the time they took. */
int32_t dgpu_prof_read(const char **names, double *total_ms, uint64_t *calls, int32_t cap);

/* ---- self-test hooks (run the device field / group code on tiny inputs) ---- */
/* host: the GLV split of a G1 scalar used by dgpu_g1_scale_batch: k mod r = k1 + k2 * lambda, lambda = x_BLS^2 - 1, k1, k2 < 2^128 */
int32_t dgpu_selftest_glv_decompose(const uint64_t k[4], uint64_t k1[2], uint64_t k2[2]);
/* host: the GLS split of a G2 scalar used by dgpu_g2_mul_add_batch and dgpu_g2_fold_apply: k mod r = d0 + d1 |x| + d2 |x|^2 + d3 |x|^3,
 * |x| = 0xd201000000010000 (the BLS parameter), d0, d1, d2 < |x| */
int32_t dgpu_selftest_gls4_decompose(const uint64_t k[4], uint64_t d[4]);
int32_t dgpu_selftest_fp_mul(const uint64_t *a /* n*6 */, const uint64_t *b /* n*6 */, size_t n, uint64_t *out /* n*6 */);
int32_t dgpu_selftest_g1_sum(const uint64_t *pts_xy /* n*12 */, const uint8_t *neg, size_t n, uint64_t out_xyz[18]);
/* One arithmetic function of the device headers per call, one kernel per op (crypto_amd/csrc/selftest_kernels.hip.h lists the ops and their row
 * shapes): n rows of in_words u64 in and out_words u64 out, in the ABI forms of dock_gpu.h (field elements * 2^384 mod p, Fr as 256-bit words,
 * points out as X, Y, ZZ, ZZZ).  stress = k: an operand is added to itself k - 1 times, un-normalised, before the operation (for the Fr word ops
 * it is the Montgomery flag, for the chains a repetition count).  For the six-lane GT group ops (selftest_gt_kernels.hip.h) stress = reps | G << 8:
 * reps = how many times the output is fed back (at most 64), G = groups of six lanes per 64-lane wave, one of 1, 3 and 10.
 * DGPU_E_BADARG: unknown op, a row shape that is not the op's, or a stress the op does not take (any other G among them). */
int32_t dgpu_selftest_arith(int32_t op, int32_t stress, const uint64_t *in, size_t in_words, size_t n, uint64_t *out, size_t out_words);

/* ---- the sort stage of the bucket MSMs on its own (crypto_amd/csrc/dev_sort_hooks.hip.h; tests/test_gpu_sort_stage.py, tests/util.py sort_model / check_sort) ----
 * Each device hook takes a slot, allocates its own buffers, fills every output buffer AND DGPU_SELFTEST_GUARD words behind it with DGPU_SELFTEST_SENTINEL on
 * the slot's stream, runs the product's launchers (crypto_amd/csrc/sort_launch.hip.h) unchanged, copies everything back, guards included, and frees its buffers:
 * every output array below is `its length + DGPU_SELFTEST_GUARD` words long.  The two words the product's drivers clear before a sort (heavy[0] and the bad
 * word) are cleared here too. */
#define DGPU_SELFTEST_GUARD 64
#define DGPU_SELFTEST_SENTINEL 0xA5A5A5A5u
/* The two-level partition sort (launch_psort) of n scalars (8 u32 each) at width c (16..22) with W = 255 / c + 1 windows.  key_wstride = 0: the one bucket set of
 * a table (NB = 2^(c-1)); 2^(c-1): one set per window (NB = W 2^(c-1)).  val = (val_base + w val_wstride + i) | sign << 31.  idflag (flag_base + n bytes, or
 * NULL: keep every row): idflag[flag_base + i] != 0 drops row i.  part_log, P and ntiles are computed as the product's drivers do.  dyn_args = NULL: the static
 * heavy_thr (0xffffffff: nothing flagged) and no dyn; else the six words {fixed_ch, min_chunk, max_chunks, lanes_per_chunk, T_max, nb_shared} and dyn[0..4].
 * place: 0 = the product's rule, 1 = direct placement, 2 = write combining; *placed = the one that ran (1 or 2).
 * Out: off[NB + 1], entries[n W], heavy[1 + heavy_cap], dyn[5] (with dyn_args), bad[1], each followed by its guard.  DGPU_E_BADARG for a shape the product's
 * drivers never launch (W > 16, a scatter whose LDS does not fit) or n > 2^22. */
int32_t dgpu_selftest_psort(const uint32_t *scalars, size_t n, int32_t c, int32_t W, uint32_t key_wstride, uint32_t val_base, uint32_t val_wstride,
                            const uint8_t *idflag, uint32_t flag_base, uint32_t heavy_thr, uint32_t heavy_cap, const uint32_t *dyn_args, int32_t place,
                            uint32_t *off, uint32_t *entries, uint32_t *heavy, uint32_t *dyn, uint32_t *bad, int32_t *placed);
/* The sweep route of the plain pipeline for n scalars (at most 2^20) at width c (7..22), with the geometry of plain_geometry (g2 != 0: G2's accumulate geometry),
 * in the order msm_device_ranges launches it: digit codes (bases: n prepared base records of 32 (G1) / 64 (G2) words whose flag word drops a row, or NULL),
 * count sweep, scan, chunk rule (fixed_ch: 0 = the rule, else kept as dgpu_set_chunk's), k_flag_heavy, scatter sweep.  heavy_cap = 0: the geometry's
 * (n W / 256 + 1).  Out: off[NB + 1], cursor[NB], entries[n W], heavy[1 + heavy_cap], dyn[5], bad[1], each followed by its guard; NB = W 2^(c-1). */
int32_t dgpu_selftest_sort_sweep(const uint32_t *scalars, size_t n, int32_t c, int32_t g2, const uint32_t *bases, uint32_t fixed_ch, uint32_t heavy_cap,
                                 uint32_t *off, uint32_t *cursor, uint32_t *entries, uint32_t *heavy, uint32_t *dyn, uint32_t *bad);
/* launch_scan over NB counters (1 .. 2^26): off[NB + 1] and, with_cursor != 0, cursor[NB], each followed by its guard; with_cursor = 0 passes no cursor buffer. */
int32_t dgpu_selftest_scan(const uint32_t *cnt, size_t NB, int32_t with_cursor, uint32_t *off, uint32_t *cursor);
/* launch_dyn_chunk on the pair count E: dyn[0..4] = chunk length, chunks, heavy threshold, E, 0, followed by the guard. */
int32_t dgpu_selftest_dyn_chunk(uint32_t E, uint32_t fixed_ch, uint32_t min_chunk, uint32_t max_chunks, uint32_t lanes_per_chunk, uint32_t T_max, uint32_t nb_shared, uint32_t *dyn);
/* host, no device: choose_chunk(E, min_chunk, max_chunks, lanes_per_chunk, nb_shared), the host's copy of the rule (a chunk forced by dgpu_set_chunk is returned
 * as it is); DGPU_E_BADARG (negative) for min_chunk < 1 or lanes_per_chunk outside 1 .. 131072. */
int32_t dgpu_selftest_choose_chunk(uint64_t E, int32_t min_chunk, uint64_t max_chunks, int32_t lanes_per_chunk, uint64_t nb_shared);

/* ---- fault injection (tests/test_gpu_fault_paths.py): the k-th hipMalloc from now and the count - 1 after it fail ---- */
int32_t dgpu_dev_fail_alloc_after(int64_t k, int64_t count);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
