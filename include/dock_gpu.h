/* include/dock_gpu.h — C ABI of libdock_gpu.so, the MI355X (gfx950) backend for the one data-parallel
 * hot path of docknetwork/crypto: BLS12-381 variable-base MSM (G1/G2) and the batched Miller loop.
 *
 * The reference has no FFI for this path today: every call is a statically dispatched call into
 * arkworks (ark-ec 0.4).  Each entry point below names the reference call it replaces; the Rust-side
 * binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - return int32_t: 0 = DGPU_OK, negative = DGPU_E_*; never unwinds, aborts or prints.
 *   - field elements are ark-ff `Fp<MontBackend,N>` raw limbs: little-endian u64, value * R mod p,
 *     R = 2^384 for Fq (6 limbs), R = 2^256 for Fr (4 limbs)   (SURVEY.md A.5).
 *   - G1 affine = x,y (12 u64); G2 affine = x.c0,x.c1,y.c0,y.c1 (24 u64); identity is flagged out of
 *     band by `is_inf[i] != 0` (ark-ec `Affine{ x, y, infinity }` is not repr(C), the shim repacks);
 *     a point whose coordinate words are all zero is also treated as the identity.
 *   - group results are returned as a Jacobian triple X,Y,Z (ark-ec `Projective`): always the
 *     normalised representative (Z = R, i.e. one) or Z = 0 for the identity, so equal group elements
 *     give bit-identical output.
 *   - caller owns every buffer; nothing is retained after return except behind explicit handles.
 *   - thread-safe and re-entrant (the reference calls MSM from inside rayon workers,
 *     verifiable_encryption/src/tz_21/rdkgith.rs:140-147): up to six calls per device run concurrently (one
 *     slot = streams + workspace each); callers beyond six wait for a slot and are served first come, first served
 *     (the MSM rate does not depend on the number of calling threads: tests/native/inflight_threads.cpp).
 */
#ifndef DOCK_GPU_H
#define DOCK_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)      /* the library is built with -fvisibility=hidden: these entry points are its whole surface */

#define DGPU_OK            0
#define DGPU_E_NODEVICE   -1   /* no usable HIP device / dgpu_init not called or failed */
#define DGPU_E_OOM        -2   /* device or host allocation failed */
#define DGPU_E_BADARG     -3   /* NULL pointer, bad handle, offset + n out of range, n too large */
#define DGPU_E_HIP        -4   /* a HIP runtime call failed (see dgpu_last_hip_error) */
#define DGPU_E_ZERO       -5   /* final_exponentiation of 0 (arkworks returns None) */
#define DGPU_E_TOO_SMALL  -6   /* n below dgpu_set_min_gpu_n threshold: caller should stay on its CPU path */
#define DGPU_E_LENGTH     -7   /* multi_miller_loop with unequal lengths (arkworks zip_eq panics) */

/* ---- lifecycle ---- */
/* Optional, before anything else: process-level settings of the ROCm runtime that suit this library.  The library never changes its host's environment on
 * its own; a host that wants the setting calls this from its start-up code — before the process's first HIP call (the runtime reads its configuration once)
 * and while no other thread can be inside getenv / setenv.  DGPU_E_BADARG: unknown flag, or this library has already made a HIP call (too late).
 *   DGPU_HINT_EIGHT_HW_QUEUES   export GPU_MAX_HW_QUEUES=8 unless the variable is set: the runtime maps a process's streams onto that many hardware
 *                               queues (default 4); with up to six calls in flight, each on three streams, two streams on one queue run one after the
 *                               other (Miller loop -7 %, aggregation -5 %, MSM rate unchanged: profiles/r05_hwq_bench_ab.txt).  A host that has already
 *                               initialised HIP (PyTorch) exports the variable itself instead. */
#define DGPU_HINT_EIGHT_HW_QUEUES 1u
int32_t dgpu_runtime_hints(uint32_t flags);
/* fork(): HIP state does not survive it.  fork + exec is safe (the library's worker pool re-arms itself in the child); a child that goes on to USE the library
 * must bring it up again itself (dgpu_shutdown, then dgpu_init*) — handles, streams and resident tables of the parent mean nothing there. */
int32_t dgpu_init(int32_t device);           /* bind to a HIP device ordinal (one process per GPU); idempotent */
/* Several GPUs in ONE process (a Rust host is one process): one context per device, each with its own streams and
 * workspaces.  dgpu_init_devices(mask): bit d = use HIP device d; contexts are numbered 0.. in increasing device order.
 * dgpu_init_device_list: context k on physical[k] (a device may be listed twice: two contexts on one GPU, used by the tests on a
 * one-GPU box).  Entry points that take host pointers run on the calling thread's context (dgpu_set_device, thread-local, default =
 * context 0); entry points that take a handle run on the context that owns the handle. */
int32_t dgpu_init_devices(uint32_t device_mask);
int32_t dgpu_init_device_list(const int32_t *physical, int32_t count);
int32_t dgpu_context_count(void);
int32_t dgpu_set_device(int32_t context);
int32_t dgpu_shutdown(void);
int32_t dgpu_device_count(void);
const char *dgpu_strerror(int32_t code);
int32_t dgpu_last_hip_error(void);
/* below this many terms the MSM entry points return DGPU_E_TOO_SMALL without touching the device
 * (>= 95 % of the reference's call sites have n < 100).  Default: DGPU_DEFAULT_MIN_GPU_N, the measured
 * crossover against the CPU path; 0 = always run on the device. */
#define DGPU_DEFAULT_MIN_GPU_N 256
/* MSMs over a bases HANDLE (dgpu_msm_*_handle, dgpu_msm_*_resident) are refused only below min(threshold, DGPU_MIN_GPU_N_HANDLE) terms: the handle
 * carries the small path's table, a call is one launch (0.14 ms at 16 terms; one CPU thread: 0.64 ms), and a caller who uploaded bases wants them used. */
#define DGPU_MIN_GPU_N_HANDLE 8
int32_t dgpu_set_min_gpu_n(size_t n);
size_t dgpu_get_min_gpu_n(void);
/* Several devices behind the UNMODIFIED call: with more than one device context in the process (dgpu_init_devices) the one-shot entry points
 * (dgpu_msm_g1 / _g2 [_mont | _strided]) shard calls of at least n terms over all of them — context k takes the contiguous balanced chunk k of the terms
 * on a host thread inside the call (from its own resident copy of that chunk once the resident-bases cache holds it: each device caches ITS chunk of a
 * key), the partial points are folded on the host: BASELINE config 5's shape (2^24 terms over 8 GPUs) from `msm_bigint(&[G1Affine], ..)`.  Same group
 * element as on one device.  n = 0: off (the default — host-pointer calls then run on the calling thread's context, dgpu_set_device). */
int32_t dgpu_set_auto_shard_min_n(size_t n);
/* (tuning knobs of the kernels — window width, chunk length, reduction geometry, Miller-loop forms —, stage timers and self-test hooks are NOT part
 * of this ABI: include/dock_gpu_dev.h, served by the development twin libdock_gpu_dev.so.  The product runs every knob at its measured optimum.) */
/* MSMs of up to n terms (default and maximum 8192) over plain bases — one-shot calls, plain handles — run as 64 signed 4-bit windows, each a
 * tree over the terms' table entries (a table launch and a tree launch: crypto_amd/csrc/small_kernels.hip.h) instead of the ~15-launch bucket
 * pipeline: 0.27 - 0.6 ms instead of 0.7 - 0.9 ms per call.  A plain HANDLE of up to 8192 bases gets a table of its own when it is uploaded (one
 * made another way: at its second small MSM, or by dgpu_bases_precompute_*) — the eight multiples of P, 2^64 P, 2^128 P, 2^192 P per base, 6.5 KB (G1) / 13 KB (G2)
 * per base, released with the handle — and its calls are ONE launch of 16 trees over 4 n leaves and a 60-doubling fold on the host:
 * 0.14 - 0.4 ms (G1 n = 600 / 4096: 0.19 / 0.29 ms; G2: 0.37 / 0.57).  If that allocation fails the calls keep building their per-call table.
 * 0: always the bucket pipeline (the parity tests compare the two). */
int32_t dgpu_set_small_msm_max(size_t n);
/* Workspaces.  Every call in flight owns one of the context's slots (stream + grow-only device workspace).  The slots are sized AHEAD of
 * the calls so that no MSM path allocates in steady state (a hipMalloc costs 0.1 - 1 ms and the hipFree of the buffer it replaces waits for
 * the whole device, i.e. for every other call in flight): dgpu_bases_upload_* / dgpu_bases_precompute_* / dgpu_window_table_mul_to_bases_*
 * size every slot for MSMs over that handle; dgpu_reserve_g1/g2(n) does it for one-shot calls (dgpu_msm_*) of up to n terms on the calling
 * thread's context — what a Rust host calls once at start-up; without it the first one-shot call of a new size grows its own slot and
 * every idle one.  dgpu_device_alloc_count: hipMalloc calls issued by the library so far:
 * a steady-state delta of 0 is asserted by tests/test_gpu_reserve.py. */
int32_t dgpu_reserve_g1(size_t n);
int32_t dgpu_reserve_g2(size_t n);
uint64_t dgpu_device_alloc_count(void);

/* ---- one-shot MSM: host buffers in, one point out ----
 * replaces <G1Projective as VariableBaseMSM>::msm_bigint(bases, bigints)
 *   legogroth16/src/prover.rs:286,299,363,592 ; utils/src/pairs.rs:153-155 ; utils/src/owned_pairs.rs:103-105
 * Callers pass n = min(bases.len(), scalars.len()) — the truncation arkworks applies (prover.rs:286).
 * Preconditions (DGPU_E_BADARG otherwise, nothing is allocated): n < 2^31 and n * W < 2^32 where W = 255 / c + 1 is the number of
 * windows (c = 16 from n = 2^17 on: n < 2^28; split larger MSMs and fold the parts with dgpu_fold_*).  Scalars are 255-bit values
 * (Fr::MODULUS_BIT_SIZE): scalars >= r but < 2^255 are multiplied as the integers they are (the same group element as for the reduced
 * scalar, and what arkworks computes).  A scalar with bit 255 set has no meaning that is independent of arkworks' window width — its
 * `make_digits` reads bit 255 in the top window unless the width divides 255 (n <= 32, 2^18 < n <= 2^20, 2^21 < n <= 2^23
 * ignore it, every other n multiplies by the full 256-bit integer) — so every MSM entry point REFUSES such input with DGPU_E_BADARG and the
 * caller stays on its CPU path; `Fr::into_bigint()` never produces it.  (tests/test_gpu_msm.py::test_scalars_with_bit_255)
 * Bases may be any points of the curve, in the prime-order subgroup or not (every MSM entry point, handles, tables and the resident-bases
 * cache included: tests/test_gpu_off_subgroup.py). */
int32_t dgpu_msm_g1(const uint64_t *bases_xy /* n*12 */, const uint8_t *is_inf /* n or NULL */,
                    const uint64_t *scalars /* n*4, canonical */, size_t n, uint64_t out_xyz[18]);
/* replaces <G1Projective as VariableBaseMSM>::msm_unchecked(bases, &[Fr]) (Fr in Montgomery form, R = 2^256)
 *   utils/src/pairs.rs:145-147 ; utils/src/randomized_mult_checker.rs:100 ; schnorr_pok/src/pok_generalized_pedersen.rs:97 */
int32_t dgpu_msm_g1_mont(const uint64_t *bases_xy, const uint8_t *is_inf,
                         const uint64_t *scalars_mont, size_t n, uint64_t out_xyz[18]);
/* The same straight from the caller's `&[G1Affine]` / `&[G2Affine]`: ark-ec 0.4 `Affine<P> { x, y, infinity }` is a Rust struct of
 * 104 (G1) / 200 (G2) bytes whose field offsets the shim reads with core::mem::offset_of! — no host-side repacking into x|y arrays (the
 * 96-MB copy loop of a 2^20-term call; utils/src/pairs.rs:143-156 and the 166 direct call sites hand over exactly this slice).  Point i
 * lives at bases + i * stride_bytes: x at x_off, y at y_off (48 / 96 bytes of Montgomery limbs each, 8-byte aligned), the `infinity`
 * bool at inf_off (DGPU_NO_INF_OFF: no flag byte; all-zero coordinates still mean the identity).  montgomery != 0: scalars are &[Fr].
 * The whole array crosses PCIe as it is (stride_bytes per point) and is converted on the device. */
#define DGPU_NO_INF_OFF (~(size_t)0)
int32_t dgpu_msm_g1_strided(const void *bases, size_t stride_bytes, size_t x_off, size_t y_off, size_t inf_off,
                            const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t out_xyz[18]);
int32_t dgpu_msm_g2_strided(const void *bases, size_t stride_bytes, size_t x_off, size_t y_off, size_t inf_off,
                            const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t out_xyz[36]);
int32_t dgpu_bases_upload_g1_strided(const void *bases, size_t stride_bytes, size_t x_off, size_t y_off, size_t inf_off, size_t n, uint64_t *handle);
int32_t dgpu_bases_upload_g2_strided(const void *bases, size_t stride_bytes, size_t x_off, size_t y_off, size_t inf_off, size_t n, uint64_t *handle);
/* same pair over G2 — legogroth16/src/prover.rs:344 (b_g2_query), delegatable_credentials/src/set_commitment.rs:566 */
int32_t dgpu_msm_g2(const uint64_t *bases_xy /* n*24 */, const uint8_t *is_inf,
                    const uint64_t *scalars, size_t n, uint64_t out_xyz[36]);
int32_t dgpu_msm_g2_mont(const uint64_t *bases_xy, const uint8_t *is_inf,
                         const uint64_t *scalars_mont, size_t n, uint64_t out_xyz[36]);

/* ---- the resident-bases cache behind the one-shot entry points above ----
 * The reference's call sites pass the same proving-key slices proof after proof (legogroth16/src/prover.rs:286,299,363,592 `msm_bigint(&pk.h_query, ..)`,
 * `&query[1..]`; utils/src/pairs.rs:143-156) and know nothing of handles.  So that the UNMODIFIED call reaches the resident path, dgpu_msm_g1 / _g2
 * [_mont | _strided] with n >= the cache's threshold (default 2^16) remember what they were given: the first sighting of (pointer, n, layout) runs one-shot
 * and keeps a 64-bit fingerprint of 32 evenly spaced records; the second sighting with the same fingerprint uploads the points once, keeps a fingerprint of
 * every record (8 B each, host memory) and turns them into a precomputed-multiples table (dgpu_bases_precompute_*: ~40 ms at 2^20 G1 points, once per key);
 * from then on the call is dgpu_msm_*_handle on that table — only the scalars cross PCIe (2^20 G1 terms: 5.3 -> ~2.8 ms).  A call whose points lie
 * INSIDE a resident entry of the same layout (`&query[1..]`, a shorter n) resolves to (entry, offset).  Same group element, limb for limb, either way.
 * Stale keys: before a resident entry's result is used the host re-fingerprints the records of the call's range and compares with what was uploaded; a difference
 * evicts the entry and the call runs one-shot on what the buffer holds now.  DEFAULT = DGPU_CACHE_VERIFY_FULL: every record, on the library's host threads, BESIDE the
 * MSM on the resident copy, whose result is discarded if the check fails (1.5 ms of host work per 2^20 G1 points; 3.21 -> 3.22 ms per call;
 * dgpu_legogroth16_prove_host checks its views beside the proof the same way: 10.0 -> 10.4 - 10.8 ms) — the unmodified call never answers from a key that has changed.
 * A host whose key cannot change between calls may select the sampled mode (s records per use, its first and last among them): a refilled buffer is still
 * noticed at once, an IN-PLACE edit of a few records only with probability s / n per call.  dgpu_bases_cache_invalidate drops entries by address range.
 * (Rust: a `&[G1Affine]` borrowed from a `ProvingKey` cannot change while borrowed; between calls it can.)
 *   dgpu_set_bases_cache_bytes(b)   device bytes the cache may hold (least recently used entries go first; an entry in use is never freed under its
 *                                   user); 0 = off and emptied.  Default (DGPU_CACHE_BYTES_AUTO): a quarter of the device memory that is free at the
 *                                   cache's first use.
 *                                   Whatever the budget, the cache gives way when the device is full: a failed allocation of the library releases
 *                                   least recently used entries and is tried again.
 *   dgpu_set_bases_cache_min_n(n)   calls below n terms are never cached (default 65536)
 *   dgpu_set_bases_cache_verify(s)  DGPU_CACHE_VERIFY_FULL (default), or s = 2 .. 4096 records sampled per use
 *   dgpu_bases_cache_invalidate     forget every entry that overlaps [p, p + bytes)
 *   dgpu_bases_cache_stats          out[0..7] = hits, misses (cacheable calls that ran one-shot), fills, stale evictions, budget evictions, bytes in use,
 *                                   byte budget (0 until resolved), resident entries */
#define DGPU_CACHE_VERIFY_FULL (-1)
#define DGPU_CACHE_BYTES_AUTO (~(size_t)0)
int32_t dgpu_set_bases_cache_bytes(size_t bytes);
int32_t dgpu_set_bases_cache_min_n(size_t n);
int32_t dgpu_set_bases_cache_verify(int32_t samples);
int32_t dgpu_bases_cache_invalidate(const void *p, size_t bytes);
int32_t dgpu_bases_cache_clear(void);
int32_t dgpu_bases_cache_stats(uint64_t out[8]);

/* ---- device-resident operands (proving-key queries live in HBM across proofs) ----
 * `offset` expresses `&query[1..]` (legogroth16/src/prover.rs:592). */
int32_t dgpu_bases_upload_g1(const uint64_t *bases_xy, const uint8_t *is_inf, size_t n, uint64_t *handle);
int32_t dgpu_bases_upload_g2(const uint64_t *bases_xy, const uint8_t *is_inf, size_t n, uint64_t *handle);
int32_t dgpu_bases_free(uint64_t handle);
int32_t dgpu_scalars_upload(const uint64_t *scalars /* n*4 */, size_t n, int32_t montgomery, uint64_t *handle);
int32_t dgpu_scalars_free(uint64_t handle);
/* one resident scalar vector from several host arrays, in order (the prover's `assignment` = inputs[1..] ++ witnesses,
 * legogroth16/src/prover.rs:319-321, without concatenating on the host) */
int32_t dgpu_scalars_upload_parts(const uint64_t *const *parts, const size_t *counts, size_t n_parts, int32_t montgomery, uint64_t *handle);
int32_t dgpu_msm_g1_handle(uint64_t bases, size_t offset, const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t out_xyz[18]);
int32_t dgpu_msm_g2_handle(uint64_t bases, size_t offset, const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t out_xyz[36]);
/* MANY small MSMs over ONE resident base set in one call: row j multiplies bases [offset, offset + n) of the handle by the n scalars at
 * scalars + 4 * row_stride * j (row_stride >= n scalars between rows; what lies between two rows is never read) and writes out_xyz[j] (18 / 36 words) —
 * bit for bit what dgpu_msm_g*_handle(bases, offset, scalars + 4 * row_stride * j, n, montgomery, ..) writes, identity rows included — and out_inf[j] = 1
 * for an identity row (out_inf may be NULL).  The reference issues its small MSMs this way: verifiable_encryption/src/tz_21/dkgith.rs:174-192,368
 * (NUM_REPETITIONS x NUM_PARTIES msm_unchecked(comm_key, ..)), rdkgith.rs:140-147, bbs_plus/src/setup.rs:128-146,176-193, kvac/src/bbdt_2016/setup.rs:109,
 * kvac/src/bbs_sharp/setup.rs:122, schnorr_pok/src/pok_generalized_pedersen.rs:97,153.
 * Refusals: a scalar with bit 255 set ANYWHERE in the m x n block refuses the whole call (DGPU_E_BADARG; no row of out_xyz is then defined); m = 0 is
 * DGPU_OK without touching a device or the pointers; n = 0 answers every row as the single call answers n = 0; NULL scalars / out_xyz with m, n > 0,
 * row_stride < n, offset + n beyond the handle, a bad or busy handle: DGPU_E_BADARG; DGPU_E_TOO_SMALL only when m * n (the batch, not the row) is below
 * min(dgpu_get_min_gpu_n(), DGPU_MIN_GPU_N_HANDLE): 300 one-term rows are device work.
 * Paths: a PLAIN handle of at most 8192 bases with n <= dgpu_set_small_msm_max takes the many-row kernels (crypto_amd/csrc/many_kernels.hip.h) over the
 * handle's small-path table (built on the spot if the handle has none yet): per chunk of rows ONE launch of the 16 trees of every row — rows of up to 32
 * terms share blocks — and ONE launch that folds and normalises every row on the device; the host only copies.  Any other handle the single call accepts
 * (a precomputed-multiples table, more than 8192 bases, dgpu_set_small_msm_max(0), no memory for the table) runs its rows through the single-row driver inside
 * the call: correct, not faster than the caller's own loop.  Sharded handles are refused like dgpu_msm_*_handle refuses them.
 * Memory: the call owns one slot; rows go in chunks of min(4096, 2^17 / n) rows, so the slot's grow-only workspace stays below ~70 MB whatever m, and a
 * second call of a shape already seen allocates nothing.  Thread-safe like every entry point: several calls may be in flight. */
int32_t dgpu_msm_g1_handle_many(uint64_t bases, size_t offset, const uint64_t *scalars, size_t row_stride, size_t n, size_t m, int32_t montgomery,
                                uint64_t *out_xyz /* m * 18 */, uint8_t *out_inf /* m or NULL */);
int32_t dgpu_msm_g2_handle_many(uint64_t bases, size_t offset, const uint64_t *scalars, size_t row_stride, size_t n, size_t m, int32_t montgomery,
                                uint64_t *out_xyz /* m * 36 */, uint8_t *out_inf /* m or NULL */);
/* MANY small MSMs, each over its OWN bases, in one call: N terms (bases_xy, is_inf, scalars as for dgpu_msm_g*) cut into nseg segments; segment g is the
 * terms [seg_end[g - 1], seg_end[g]) with seg_end[-1] = 0, seg_end ascending and seg_end[nseg - 1] == N (the convention of dgpu_multi_miller_loop_segments).
 * out_xyz[g] (18 / 36 words) is bit for bit what dgpu_msm_g* writes for that segment alone with the size threshold off: the normalised Jacobian point
 * (X, Y, 1), or (1, 1, 0) with out_inf[g] = 1 for the identity (out_inf may be NULL); an empty segment is the identity.  montgomery != 0 takes &[Fr] limbs as
 * dgpu_msm_g*_mont does.  Bases may be any points of the curve.  The reference issues such batches back to back: saver/src/encryption.rs:710-740 (chunks + 2
 * msm_bigint calls, one per ciphertext column), legogroth16/src/link/utils.rs:85-120 (one sum per matrix column), the paired halving MSMs of
 * legogroth16/src/aggregation/utils.rs:51-81, the per-proof MSMs of bbs_plus/src/proof.rs:580.
 * Refusals: a scalar with bit 255 set ANYWHERE refuses the whole call (DGPU_E_BADARG; no row of out_xyz is then defined); nseg = 0 is DGPU_OK without touching
 * a device or the pointers; with nseg > 0, a NULL bases_xy / scalars / out_xyz / seg_end, a descending seg_end, seg_end[nseg - 1] != N or N >= 2^31:
 * DGPU_E_BADARG, decided before the device is looked at; DGPU_E_NODEVICE comes before any size threshold; DGPU_E_TOO_SMALL only when N (the batch, not the
 * segment) is below dgpu_get_min_gpu_n(): 300 segments of one term are device work.
 * Paths: segments of up to 8192 terms (and dgpu_set_small_msm_max) travel in chunks of whole segments — one upload, ONE launch of the table of eight multiples
 * over all the chunk's bases, ONE launch of the 64 window trees of every segment (short segments share blocks; crypto_amd/csrc/seg_kernels.hip.h), and the
 * per-segment fold: on the device in one more launch when the chunk has many segments, on the host's threads when it has few (the count at which the device takes over is a
 * provisional default until it is measured; no times are quoted for this call yet).  A LONGER segment goes through
 * the single-call driver inside the call: correct, not faster than the caller's own dgpu_msm_g* call.
 * Memory: the call owns one slot; a chunk holds at most 2^16 terms (the table is 1.6 KB per G1 base, 3.3 KB per G2 base: at most 109 / 218 MB) and 4096
 * segments (64 window sums each: 55 / 109 MB), so the slot's grow-only workspace stays bounded whatever N, a failed or refused call leaves nothing else
 * behind, and a second call of a shape already seen allocates nothing.  Thread-safe like every entry point: several calls may be in flight. */
int32_t dgpu_msm_g1_segments(const uint64_t *bases_xy /* N * 12 */, const uint8_t *is_inf /* N or NULL */, const uint64_t *scalars /* N * 4 */, size_t N,
                             const uint64_t *seg_end, size_t nseg, int32_t montgomery, uint64_t *out_xyz /* nseg * 18 */, uint8_t *out_inf /* nseg or NULL */);
int32_t dgpu_msm_g2_segments(const uint64_t *bases_xy /* N * 24 */, const uint8_t *is_inf /* N or NULL */, const uint64_t *scalars /* N * 4 */, size_t N,
                             const uint64_t *seg_end, size_t nseg, int32_t montgomery, uint64_t *out_xyz /* nseg * 36 */, uint8_t *out_inf /* nseg or NULL */);
/* Precomputed-multiples mode for a resident query (in place; the handle keeps its id): the device builds table[w][i] = 2^(c w) P_i for the
 * W = 255 / c + 1 windows (W x the memory: 1.7 GB for a 2^20-point G1 query at c = 20 — sized for 288 GB of HBM), after which every MSM on
 * the handle adds digit w of scalar i into ONE bucket set shared by all windows: wider windows (13 instead of 16 additions per term at
 * n = 2^20), 16x fewer buckets to reduce, no Horner fold on the host.  Same group element as before, limb for limb.  window_bits: 0 =
 * chosen from n, else 16..22.  Works on plain (dgpu_bases_upload_*, dgpu_window_table_mul_to_bases_*) and sharded handles; offsets
 * (`&query[1..]`) and sub-ranges keep working.  While the table is being built the handle is unavailable (DGPU_E_BADARG).
 * A handle too small for a bucket table to pay (below 2^15 points with window_bits = 0) stays plain; with up to 8192 points it gets the small
 * path's table (dgpu_set_small_msm_max above) if its upload has not built it already.
 * The automatic width (20 from 320 000 points) is the optimum for full-width scalars.  A query that is multiplied by a WITNESS (a proving key's
 * a / b / l queries: half of a Groth16 witness is 0 or 1, much of the rest small) adds fewer points per MSM but reduces the same number of
 * buckets, and a proof reduces five bucket sets: DGPU_TABLE_C_WITNESS = 17 has the window count of 18 (15) with half the buckets — measured
 * at 2^20 constraints: 12.4 -> 11.75 ms per proof, 10.2 -> 9.6 with four in flight (19: 12.5, 18: 12.0, 16: 12.9). */
#define DGPU_TABLE_C_WITNESS 17
int32_t dgpu_bases_precompute_g1(uint64_t bases, int32_t window_bits);
int32_t dgpu_bases_precompute_g2(uint64_t bases, int32_t window_bits);
/* ---- one partition sort for several tables ----
 * A, B-in-G1 and B-in-G2 of a LegoGroth16 proof multiply the same assignment by three queries of equal length (legogroth16/src/prover.rs:325-344
 * through calculate_coeff :585-594).  With the queries held as precomputed tables of ONE shape (same window width, same row count) the sort of
 * the (window, bucket) keys is the same for all three: dgpu_scalars_sort does it once — for scalars [scalar_offset, scalar_offset + n) against rows
 * [base_offset, base_offset + n) of any table of that shape (G1 or G2) — and dgpu_msm_g1/g2_sorted run the rest of the MSM on a table of
 * that shape (DGPU_E_BADARG otherwise).  Identity rows of a table are passed over by the accumulation.  The result is the group element
 * dgpu_msm_*_resident returns for the same operands.  row_shift = k > 0: the table is k rows SHORTER than that shape and holds the points
 * of its rows k, k + 1, ... (the l_query against the list sorted for the a_query: the assignment minus its first k entries, prover.rs:292-299);
 * the terms of rows < k are passed over.  Free the sorted handle with dgpu_scalars_free once the MSMs have returned. */
int32_t dgpu_bases_table_shape(uint64_t table, size_t *rows, int32_t *window_bits, int32_t *windows);   /* DGPU_E_BADARG: not a precomputed table */
int32_t dgpu_scalars_sort(uint64_t table, size_t base_offset, uint64_t scalars, size_t scalar_offset, size_t n, uint64_t *sorted_handle);
int32_t dgpu_msm_g1_sorted(uint64_t table, uint64_t sorted, size_t row_shift, uint64_t out_xyz[18]);
int32_t dgpu_msm_g2_sorted(uint64_t table, uint64_t sorted, size_t row_shift, uint64_t out_xyz[36]);
/* both operands resident: the timed region of bench.py (inputs already in HBM) */
int32_t dgpu_msm_g1_resident(uint64_t bases, size_t base_offset, uint64_t scalars, size_t scalar_offset, size_t n, uint64_t out_xyz[18]);
int32_t dgpu_msm_g2_resident(uint64_t bases, size_t base_offset, uint64_t scalars, size_t scalar_offset, size_t n, uint64_t out_xyz[36]);

/* ---- several GPUs behind the ABI (SURVEY.md 8b `dgpu_msm_g1_sharded`, 8e): point-chunk sharding inside one process ----
 * Context k (see dgpu_init_devices) takes the contiguous balanced chunk k of the n terms, runs the whole single-GPU pipeline on it
 * from its own host thread inside the call, and the per-device partial points (144 / 288 B) are folded on the host — bit-identical
 * to the single-device result (the ABI returns the normalised representative).  ngpus = 0: every initialised context.
 *   dgpu_msm_*_sharded            one-shot: host bases + scalars in (each device pulls its own chunk over its own PCIe link)
 *   dgpu_bases_upload_*_sharded   a proving-key query resident across the devices; free with dgpu_bases_free
 *   dgpu_msm_*_sharded_handle     fresh host scalars against such a handle (n <= number of bases: the first n terms)
 *   dgpu_scalars_upload_sharded   scalars split the way the bases handle `like` is split; free with dgpu_scalars_free
 *   dgpu_msm_*_sharded_resident   both operands resident (BASELINE config 5's timed region: inputs pre-sharded) */
int32_t dgpu_msm_g1_sharded(const uint64_t *bases_xy, const uint8_t *is_inf, const uint64_t *scalars, size_t n, int32_t ngpus, uint64_t out_xyz[18]);
int32_t dgpu_msm_g2_sharded(const uint64_t *bases_xy, const uint8_t *is_inf, const uint64_t *scalars, size_t n, int32_t ngpus, uint64_t out_xyz[36]);
int32_t dgpu_bases_upload_g1_sharded(const uint64_t *bases_xy, const uint8_t *is_inf, size_t n, int32_t ngpus, uint64_t *handle);
int32_t dgpu_bases_upload_g2_sharded(const uint64_t *bases_xy, const uint8_t *is_inf, size_t n, int32_t ngpus, uint64_t *handle);
int32_t dgpu_msm_g1_sharded_handle(uint64_t bases, const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t out_xyz[18]);
int32_t dgpu_msm_g2_sharded_handle(uint64_t bases, const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t out_xyz[36]);
int32_t dgpu_scalars_upload_sharded(const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t like, uint64_t *handle);
/* scalars [lo, hi) of a resident vector as a new vector on device context `dst_context`: device to device (a peer copy over xGMI between two
 * GPUs; peer access is enabled between the process's devices at init).  dgpu_legogroth16_prove on a sharded key moves h this way. */
int32_t dgpu_scalars_copy_range(uint64_t scalars, size_t lo, size_t hi, int32_t dst_context, uint64_t *handle);
int32_t dgpu_msm_g1_sharded_resident(uint64_t bases, uint64_t scalars, uint64_t out_xyz[18]);
int32_t dgpu_msm_g2_sharded_resident(uint64_t bases, uint64_t scalars, uint64_t out_xyz[36]);

/* ---- multi-process multi-GPU: fold per-rank partial results (host code; EC addition is not an RCCL reduction op, so the
 * collective is an all-gather of k normalised Jacobian triples followed by this fold) ---- */
int32_t dgpu_fold_g1(const uint64_t *partials_xyz /* k*18 */, size_t k, uint64_t out_xyz[18]);
int32_t dgpu_fold_g2(const uint64_t *partials_xyz /* k*36 */, size_t k, uint64_t out_xyz[36]);
/* sum_i scalars[i] * points[i] over k <= DGPU_MAX_LINCOMB affine points, computed on the HOST (no device call, usable without a device).
 * This is the O(1) group arithmetic around the MSMs that the reference does with `mul_bigint` on the CPU, not a replacement for them:
 * delta_g1 * r, s g_a + r g1_b - rs delta - v eta/delta, g_d (legogroth16/src/prover.rs:309-313, 350-355, 361-368, 585-594).
 * points: k x 12 (G1) / 24 (G2) u64 Montgomery, is_inf: k bytes or NULL, scalars: k x 4 u64 canonical; out: normalised Jacobian. */
#define DGPU_MAX_LINCOMB 16
int32_t dgpu_lincomb_g1(const uint64_t *points_xy, const uint8_t *is_inf, const uint64_t *scalars, size_t k, uint64_t out_xyz[18]);
int32_t dgpu_lincomb_g2(const uint64_t *points_xy, const uint8_t *is_inf, const uint64_t *scalars, size_t k, uint64_t out_xyz[36]);

/* ---- pairings ----
 * replaces Bls12_381::multi_miller_loop(a, b) — utils/src/randomized_pairing_check.rs:207,
 * legogroth16/src/verifier.rs:69-76.  skip[i] != 0 marks a pair with an identity member (arkworks
 * filters those out).  Output: raw MillerLoopOutput, Fp12 as c0.c0.c0 ... c1.c2.c1 (72 u64).
 * Every Miller-loop entry point accepts any P on E(Fp) and any Q of order greater than the loop's doubling chain on E'(Fp2), in the
 * prime-order subgroups or not; only all-zero words or a skip flag mark an identity member (P = (0, 2) is a point). */
int32_t dgpu_multi_miller_loop(const uint64_t *p_xy /* n*12 */, const uint64_t *q_xy /* n*24 */,
                               const uint8_t *skip /* n or NULL */, size_t n, uint64_t out_f12[72]);
/* E::G2Prepared — the form in which the reference's verifier and pairing checker HOLD their G2 operands
 * (legogroth16/src/data_structures.rs:118-120 `gamma_g2_neg_pc` / `delta_g2_neg_pc`, verifier.rs:22-23,69-76;
 * utils/src/randomized_pairing_check.rs:35 `pending: (Vec<G1Prepared>, Vec<G2Prepared>)`, :119-138,:204-214).
 * One prepared point = arkworks' `ell_coeffs`: 68 triples (Fp2, Fp2, Fp2), each Fq 6 x u64 Montgomery limbs in the order
 * c0.c0 c0.c1 c1.c0 c1.c1 c2.c0 c2.c1 -> DGPU_G2_PREPARED_WORDS u64 = 19 584 B; `infinity` travels as a flag byte and the
 * block of an identity point is all zero.
 * dgpu_g2_prepare replaces `G2Prepared::from(G2Affine)` for a batch (the 63 doubling + 5 addition steps run on the GPU);
 * dgpu_multi_miller_loop_prepared replaces `E::multi_miller_loop(a, b)` where b is already prepared: the same raw
 * MillerLoopOutput, limb for limb, as dgpu_multi_miller_loop on the unprepared points (the reference asserts exactly this
 * for pairings, utils/src/msm.rs:261-276).  skip[i] != 0, an all-zero P or an all-zero coefficient block skip pair i. */
#define DGPU_G2_PREPARED_WORDS (68 * 36)
#define DGPU_MAX_PREPARED ((size_t)1 << 18)     /* pairs per call (5 GB of coefficients) */
int32_t dgpu_g2_prepare(const uint64_t *q_xy /* n*24 */, const uint8_t *is_inf /* n or NULL */, size_t n,
                        uint64_t *out_coeffs /* n*DGPU_G2_PREPARED_WORDS */, uint8_t *out_inf /* n */);
int32_t dgpu_multi_miller_loop_prepared(const uint64_t *p_xy /* n*12 */, const uint64_t *coeffs /* n*DGPU_G2_PREPARED_WORDS */,
                                        const uint8_t *skip /* n or NULL */, size_t n, uint64_t out_f12[72]);
/* The same product over n_aff pairs with affine Q and n_prep pairs with prepared Q in ONE call (no separate dgpu_g2_prepare, no coefficient
 * round trip for the affine members): what legogroth16/src/verifier.rs:69-76 passes to multi_miller_loop — `[proof.b.into(),
 * pvk.delta_g2_neg_pc.clone(), pvk.gamma_g2_neg_pc.clone()]` — and what a RandomizedPairingChecker's `pending` holds when some operands
 * came in prepared (utils/src/randomized_pairing_check.rs:119-138).  The product does not depend on the order of the pairs. */
int32_t dgpu_multi_miller_loop_mixed(const uint64_t *p_aff /* n_aff x 12 */, const uint64_t *q_aff /* n_aff x 24 */, const uint8_t *skip_aff, size_t n_aff,
                                     const uint64_t *p_prep /* n_prep x 12 */, const uint64_t *coeffs /* n_prep x DGPU_G2_PREPARED_WORDS */, const uint8_t *skip_prep, size_t n_prep,
                                     uint64_t out_f12[72]);
/* prod_i e([m_i] P_i, Q_i) x prod_j e(P'_j, prepared_j): the scalings of RandomizedPairingChecker and its Miller loop as ONE call
 * (utils/src/randomized_pairing_check.rs:125-134 `a.mul_bigint(m)` per source, then :204-214 the lazy multi_miller_loop) — limb for limb what
 * dgpu_g1_scale_batch followed by dgpu_multi_miller_loop_mixed returns.  The line coefficients of a pair depend on Q alone, so the chain of the Q_i
 * and the scaling chains of the P_i run side by side and the scaled points never visit the host (1024 pairs: 1.64 -> 1.34 ms).
 * scalars: n_aff x 4 canonical words (scalar_stride = 4) or ONE scalar for every pair (scalar_stride = 0), reduced mod r; a pair whose
 * scaled point is the identity (m = 0 mod r, P all zero), whose Q is all zero or whose skip flag is set contributes one.  P_i in the
 * prime-order subgroup (the invariant of arkworks' G1Affine: the scaling uses the endomorphism); any other P is scaled as dgpu_g1_scale_batch
 * scales it, and a pair whose scaled point turns out to be the identity on the device contributes one in both forms of the call. */
int32_t dgpu_multi_miller_loop_scaled(const uint64_t *p_aff /* n_aff x 12 */, const uint64_t *scalars, size_t scalar_stride, const uint64_t *q_aff /* n_aff x 24 */,
                                      const uint8_t *skip_aff, size_t n_aff,
                                      const uint64_t *p_prep /* n_prep x 12 */, const uint64_t *coeffs /* n_prep x DGPU_G2_PREPARED_WORDS */, const uint8_t *skip_prep, size_t n_prep,
                                      uint64_t out_f12[72]);
/* nseg independent Miller loops in one call: segment g is the pairs [seg_end[g - 1], seg_end[g]) (ascending, seg_end[nseg - 1] == n; an empty
 * segment yields one); out_f12 = nseg x 72 words, each what dgpu_multi_miller_loop returns for that segment alone.  Serves the
 * mutually independent `E::multi_pairing` calls the aggregation issues one after another (legogroth16/src/aggregation/commitment.rs:30-31,54-67,
 * aggregation/utils.rs:95-96: ten per GIPA round, 1 ... n/2 pairs each): a line-kernel launch lasts as long as its 68 dependent steps
 * whatever the pair count, so the segments share one. */
int32_t dgpu_multi_miller_loop_segments(const uint64_t *p_xy, const uint64_t *q_xy, const uint8_t *skip, size_t n,
                                        const uint64_t *seg_end, size_t nseg, uint64_t *out_f12 /* nseg x 72 */);
/* the same followed by the final exponentiation of every segment (E::multi_pairing), on the host threads that assemble the Miller outputs;
 * DGPU_E_ZERO if a Miller output is zero (arkworks' multi_pairing would panic on the `None`: cannot happen for points of G1 x G2) */
int32_t dgpu_multi_pairing_segments(const uint64_t *p_xy, const uint64_t *q_xy, const uint8_t *skip, size_t n,
                                    const uint64_t *seg_end, size_t nseg, uint64_t *out_gt /* nseg x 72 */);
/* the same with the pairs chunked over the process's device contexts (ngpus = 0: all of them), raw outputs multiplied on the host */
int32_t dgpu_multi_miller_loop_sharded(const uint64_t *p_xy, const uint64_t *q_xy, const uint8_t *skip, size_t n, int32_t ngpus, uint64_t out_f12[72]);
/* replaces Bls12_381::final_exponentiation — utils/src/randomized_pairing_check.rs:213 (host code, once per batch) */
int32_t dgpu_final_exponentiation(const uint64_t in_f12[72], uint64_t out_f12[72]);
/* the same for n independent elements, on the device (crypto_amd/csrc/gt_kernels.hip.h: one element per group of six lanes), whatever n: one verdict
 * per statement needs one final exponentiation per proof (dgpu_legogroth16_verify_each).  out_gt: n x 72 words, for canonical input words equal to what
 * dgpu_final_exponentiation returns; is_zero[i] = 1 where element i is zero (arkworks' None, dgpu_final_exponentiation's DGPU_E_ZERO), its words are
 * then zero.  Large n runs in chunks of bounded device memory.  n = 0: DGPU_OK without a device; NULL pointers with n > 0: DGPU_E_BADARG. */
int32_t dgpu_final_exponentiation_batch(const uint64_t *in_f12 /* n*72 */, size_t n, uint64_t *out_gt /* n*72 */, uint8_t *is_zero /* n */);

/* ---- pieces of utils::randomized_pairing_check::RandomizedPairingChecker (utils/src/randomized_pairing_check.rs:24-215) ----
 * out_i = s_i * P_i as affine points (the per-equation `a.mul_bigint(m)` scalings, :125-127,152-158), batched on the GPU.
 * scalar_stride = 4: one canonical scalar per point; scalar_stride = 0: the same scalar for every point.
 * negate[i] != 0 returns -(s_i P_i) (the `-c.mul_bigint(m)` of add_multiple_sources, :156-158).
 * P_i in G1: the scaling computes k1 P + k2 phi(P) for the GLV split s mod r = k1 + k2 lambda, which is [s] P there only; for any other
 * point of the curve it returns that same k1 P + k2 phi(P) (e.g. ((k1 + k2) mod 3) P for P of order 3), the identity flagged as usual. */
int32_t dgpu_g1_scale_batch(const uint64_t *p_xy /* n*12 */, const uint8_t *is_inf, const uint64_t *scalars, size_t scalar_stride,
                            const uint8_t *negate, size_t n, uint64_t *out_xy /* n*12 */, uint8_t *out_inf /* n */);
/* GT arithmetic on the host: PairingOutput `+` is the Fp12 product, `mul_bigint` the power (:136 `self.right += out.mul_bigint(m)`) */
int32_t dgpu_fp12_mul(const uint64_t a[72], const uint64_t b[72], uint64_t out[72]);
int32_t dgpu_fp12_pow(const uint64_t a[72], const uint64_t e[4], uint64_t out[72]);
/* ok[i] = a_i is an element of GT (order dividing r): `Valid::check` of ark-ec's PairingOutput (a proof deserialized with Validate::Yes), answered
 * with a Frobenius identity and one exponentiation by the 64-bit curve parameter (0.09 ms per element on a host thread) instead of f^r (1.3 ms) */
int32_t dgpu_gt_in_subgroup(const uint64_t *a /* n*72 */, size_t n, uint8_t *ok /* n */);
/* prod_i a_i^{e_i}: the fold of `PairingOutput::mul_bigint` + `add_assign` in the aggregation verifier
 * (legogroth16/src/aggregation/groth16/verifier.rs:272-370); host threads, generic Fp12 arithmetic */
int32_t dgpu_fp12_multi_pow(const uint64_t *a /* n*72 */, const uint64_t *e /* n*4 */, size_t n, uint64_t out[72]);
/* The same three on the DEVICE, for many elements (crypto_amd/csrc/gt_kernels.hip.h: one element per group of six lanes, signed 4-bit windows over
 * a table of eight powers with Granger-Scott squarings when every base of a wave lies in the cyclotomic subgroup, binary square-and-multiply
 * otherwise).  Any Fp12 base, any 256-bit exponent (not reduced mod r: `PairingOutput::mul_bigint`); the words are those of dgpu_fp12_pow,
 * dgpu_fp12_multi_pow and dgpu_gt_in_subgroup.  No size threshold: the device runs whatever n, in chunks of bounded device memory; the host entry
 * points above stay the choice for a few elements (the crossover has not been measured yet: tests/perf/gt_pow_timing.py writes it to
 * profiles/gt_pow_timing.json).  n = 0: DGPU_OK without a device (the product is then the
 * element one); NULL pointers with n > 0, an e_stride other than 4 (an exponent per base) or 0 (one for all): DGPU_E_BADARG. */
int32_t dgpu_fp12_pow_batch(const uint64_t *a /* n*72 */, const uint64_t *e, size_t e_stride /* 4 or 0 */, size_t n, uint64_t *out /* n*72 */);
int32_t dgpu_fp12_multi_pow_device(const uint64_t *a /* n*72 */, const uint64_t *e /* n*4 */, size_t n, uint64_t out[72]);
int32_t dgpu_gt_in_subgroup_device(const uint64_t *a /* n*72 */, size_t n, uint8_t *ok /* n */);

/* ---- fixed-base batch multiplication ----
 * replaces ark-ec FixedBase::{get_window_table, msm} as the reference calls them: WindowTable::new / multiply_many and
 * multiply_field_elems_with_same_group_elem (utils/src/msm.rs:8-62) and the six query computations of the LegoGroth16 CRS
 * generator followed by normalize_batch (legogroth16/src/generator.rs:335-399,424-431).
 * out_i = scalars_i * base as affine points (x, y Montgomery limbs; zeros and out_inf[i] = 1 for the identity).
 * montgomery != 0: scalars are Fr Montgomery limbs (what &[Fr] holds), else canonical.  Canonical scalars may be any 256-bit integer,
 * r and above included: all 32 bytes are digits of the table, so the product is the integer times the base (the same point as the scalar
 * reduced mod r; a multiple of r gives the identity).  The table handle keeps 32 x 255 multiples of the base in device memory (1 MiB for G1,
 * 2 MiB for G2). */
int32_t dgpu_window_table_g1(const uint64_t base_xy[12], uint64_t *handle);
int32_t dgpu_window_table_g2(const uint64_t base_xy[24], uint64_t *handle);
int32_t dgpu_window_table_free(uint64_t handle);
int32_t dgpu_window_table_mul_g1(uint64_t table, const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t *out_xy /* n*12 */, uint8_t *out_inf /* n */);
int32_t dgpu_window_table_mul_g2(uint64_t table, const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t *out_xy /* n*24 */, uint8_t *out_inf /* n */);
/* same products left in device memory as an MSM bases handle (dgpu_msm_g1/g2_handle, dgpu_bases_free): a CRS query goes
 * from the generator to the prover without crossing PCIe */
int32_t dgpu_window_table_mul_to_bases_g1(uint64_t table, const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t *bases_handle);
int32_t dgpu_window_table_mul_to_bases_g2(uint64_t table, const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t *bases_handle);
/* table + multiply + free in one call */
int32_t dgpu_fixed_base_g1(const uint64_t base_xy[12], const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t *out_xy, uint8_t *out_inf);
int32_t dgpu_fixed_base_g2(const uint64_t base_xy[24], const uint64_t *scalars, size_t n, int32_t montgomery, uint64_t *out_xy, uint8_t *out_inf);

/* ---- SnarkPack aggregation folding step ----
 * out_i = addend_i + scalars_i * P_i as affine points: `compress` (legogroth16/src/aggregation/utils.rs:34-49), Key::compress and
 * Key::scale (legogroth16/src/aggregation/key.rs:117-175), `b.mul_bigint(r_i)` (aggregation/groth16/prover.rs:107-112).
 * scalar_stride = 4: one canonical scalar per point; 0: one scalar for all.  addend_xy = NULL: plain scaling.
 * Identity inputs: all-zero words or a set flag byte; identity outputs: zero words and out_inf[i] = 1.
 * The points are elements of the prime-order subgroups (what arkworks' G1Affine / G2Affine hold after deserialization or arithmetic):
 * the scalars are split by the GLV / GLS endomorphisms, which act as multiplications only there.  Any 256-bit scalar (reduced mod r). */
int32_t dgpu_g1_mul_add_batch(const uint64_t *p_xy /* n*12 */, const uint8_t *p_inf, const uint64_t *scalars, size_t scalar_stride,
                              const uint64_t *addend_xy /* n*12 or NULL */, const uint8_t *addend_inf, size_t n, uint64_t *out_xy, uint8_t *out_inf);
int32_t dgpu_g2_mul_add_batch(const uint64_t *p_xy /* n*24 */, const uint8_t *p_inf, const uint64_t *scalars, size_t scalar_stride,
                              const uint64_t *addend_xy /* n*24 or NULL */, const uint8_t *addend_inf, size_t n, uint64_t *out_xy, uint8_t *out_inf);
/* The same step for ONE scalar that is not known yet (a GIPA round's challenge arrives after the round's pairings): prepare runs the doubling chains of
 * the points — the part of a double-and-add that does not depend on the scalar, 1 ms whatever n — and keeps 2^k P_i (G1; G2: 2^k |x|^j P_i, the GLS
 * bases) behind a handle (28.7 KB per G1 point, 115 KB per G2 point); apply then adds the entries at the set bits of the split scalar and the addend in a
 * tree nine additions deep: 0.15 - 0.25 ms instead of 1.5.  out_i = addend_i + scalar * P_i, affine, bit for bit what dgpu_g*_mul_add_batch returns
 * (identity: zero words and out_inf[i] = 1).  One handle serves any number of applies; dgpu_fold_free releases it.  crypto_amd/csrc/fold_kernels.hip.h */
int32_t dgpu_g1_fold_prepare(const uint64_t *p_xy /* n*12 */, size_t n, uint64_t *handle);
int32_t dgpu_g2_fold_prepare(const uint64_t *p_xy /* n*24 */, size_t n, uint64_t *handle);
/* both groups' point sets of a round in ONE launch (two prepare calls can land on one hardware queue and run one after the other); a set may be empty
 * (n = 0: its pointers are not read and its handle comes back 0), not both (DGPU_E_BADARG, both handles 0) */
int32_t dgpu_fold_prepare_pair(const uint64_t *g1_xy, size_t n1, uint64_t *g1_handle, const uint64_t *g2_xy, size_t n2, uint64_t *g2_handle);
int32_t dgpu_g1_fold_apply(uint64_t handle, const uint64_t scalar[4], const uint64_t *addend_xy /* n*12 or NULL */, uint64_t *out_xy, uint8_t *out_inf);
int32_t dgpu_g2_fold_apply(uint64_t handle, const uint64_t scalar[4], const uint64_t *addend_xy /* n*24 or NULL */, uint64_t *out_xy, uint8_t *out_inf);
int32_t dgpu_fold_free(uint64_t handle);

/* ---- R1CS -> QAP witness map ----
 * replaces LibsnarkReduction::witness_map_from_matrices (legogroth16/src/r1cs_to_qap.rs:150-210): h = ((A z)(B z) - C z) / Z_D as the
 * D = next_pow2(num_constraints + num_inputs) coefficients the prover pairs with h_query (legogroth16/src/prover.rs:281-286).
 * Matrices in CSR (rowptr[num_constraints + 1], cols[nnz], vals[nnz * 4]); assignment = (1, instance..., witness...), num_vars values.
 * montgomery & 1: coefficients and assignment are ark-ff Fr limbs (R = 2^256), else canonical.  The result is canonical
 * (what `into_bigint` yields, prover.rs:281-283): copied to out_h (D * 4 limbs) and/or left in HBM as a scalars handle that
 * dgpu_msm_g1_resident consumes directly.  montgomery & DGPU_WM_H_MONTGOMERY: the copy in out_h is written as Fr limbs instead (the
 * `Vec<F>` witness_map_from_matrices returns, r1cs_to_qap.rs:150-210 — a drop-in for that function hands back exactly this; the conversion
 * runs on the device); a resident vector stays canonical.  *out_len = D. */
#define DGPU_WM_H_MONTGOMERY 2
int32_t dgpu_witness_map(const uint64_t *a_rowptr, const uint32_t *a_cols, const uint64_t *a_vals, size_t a_nnz,
                         const uint64_t *b_rowptr, const uint32_t *b_cols, const uint64_t *b_vals, size_t b_nnz,
                         const uint64_t *c_rowptr, const uint32_t *c_cols, const uint64_t *c_vals, size_t c_nnz,
                         const uint64_t *assignment, size_t num_vars, size_t num_inputs, size_t num_constraints, int32_t montgomery,
                         uint64_t *out_h, uint64_t *out_handle, size_t *out_len);

/* the same with the circuit's matrices resident in HBM (they are fixed per circuit; only the assignment changes per proof) */
int32_t dgpu_r1cs_upload(const uint64_t *a_rowptr, const uint32_t *a_cols, const uint64_t *a_vals, size_t a_nnz,
                         const uint64_t *b_rowptr, const uint32_t *b_cols, const uint64_t *b_vals, size_t b_nnz,
                         const uint64_t *c_rowptr, const uint32_t *c_cols, const uint64_t *c_vals, size_t c_nnz,
                         size_t num_vars, size_t num_inputs, size_t num_constraints, int32_t montgomery, uint64_t *handle);
int32_t dgpu_r1cs_free(uint64_t handle);
/* shape of a resident circuit (any pointer may be NULL); dgpu_legogroth16_prove refuses an (n_inst, num_vars) that disagrees with it */
int32_t dgpu_r1cs_shape(uint64_t r1cs, size_t *num_vars, size_t *num_inputs, size_t *num_constraints);
int32_t dgpu_witness_map_r1cs(uint64_t r1cs, const uint64_t *assignment, size_t num_vars, int32_t montgomery,
                              uint64_t *out_h, uint64_t *out_handle, size_t *out_len);
/* the same with the assignment z already resident (a dgpu_scalars_upload handle of num_vars scalars on the circuit's device): ONE upload of z
 * per proof then serves the witness map and — at scalar offset 1 — the prover's `assignment` = z[1..] of the a / b_g1 / b_g2 / l MSMs */
int32_t dgpu_witness_map_r1cs_resident(uint64_t r1cs, uint64_t assignment, uint64_t *out_h, uint64_t *out_handle, size_t *out_len);
/* MANY witness maps of ONE resident circuit in one call: row j is the num_vars scalars at assignments + 4 * row_stride * j (row_stride >= num_vars scalars
 * between rows, the convention of dgpu_msm_g1_handle_many; what lies between two rows is never read) and out_h + 4 * D * j receives, word for word, what
 * dgpu_witness_map_r1cs(r1cs, row j, num_vars, montgomery, out_h_j, NULL, ..) writes, with montgomery & 1 and with montgomery & DGPU_WM_H_MONTGOMERY alike.
 * *out_len = D, the length PER ROW.  out_handle receives ONE resident scalar vector of m * D canonical scalars, row j at scalar offset j * D (what
 * dgpu_msm_g1_handle / dgpu_scalars_copy_range address by offset); it is registered last, so a failing call leaves no handle and no allocation behind.  The
 * reference proves its small circuits statement by statement (proof_system/src/sub_protocols/bound_check_legogroth16.rs, r1cs_legogorth16.rs: bound checks,
 * MiMC, the circom vectors); a service proving the same circuit over thousands of assignments has its witness maps here.
 * Refusals, decided before the device is looked at: m = 0 is DGPU_OK without touching a device or the pointers; NULL assignments, both outputs NULL,
 * row_stride < num_vars, num_vars disagreeing with the circuit's shape, m * D beyond the address space, a bad handle: DGPU_E_BADARG.  There is no
 * DGPU_E_TOO_SMALL: the caller has uploaded a circuit and wants it used.
 * Paths: a circuit whose domain is at most 2^10 takes the block kernel (crypto_amd/csrc/wm_block_kernels.hip.h: a statement's a, b, c stay in one
 * block's LDS from the sparse rows to the h scalars; domains of up to 128 elements share blocks): per chunk of rows ONE upload of the chunk's assignments, ONE
 * launch (two more, a copy and a conversion, when Fr-limb host output and a resident vector are asked for together) and ONE download, whatever the number of rows.
 * Larger domains run row by row through the single call's driver inside the call: correct, not faster than the caller's own loop.
 * Memory: the call owns one slot; rows go in chunks of at most 4096 rows, 2^17 domain elements (rows * D) and 2^21 assignment scalars (rows * num_vars), so
 * the slot's grow-only workspace stays bounded whatever m, and a second call of a shape already seen allocates nothing (the resident vector, when asked
 * for, is the caller's).  Thread-safe like every entry point: several calls may be in flight. */
int32_t dgpu_witness_map_r1cs_many(uint64_t r1cs, const uint64_t *assignments, size_t row_stride, size_t num_vars, size_t m, int32_t montgomery,
                                   uint64_t *out_h /* m * D * 4, or NULL */, uint64_t *out_handle /* or NULL */, size_t *out_len);

/* ---- LegoGroth16 key generation from a resident circuit ----
 * dgpu_qap_instance_map replaces LibsnarkReduction::instance_map_with_evaluation (legogroth16/src/r1cs_to_qap.rs:105-147) on a dgpu_r1cs_upload circuit:
 * D = the witness map's domain (the next power of two >= num_constraints + num_inputs), u_i = Z(t) w^i / (D (t - w^i)) for i < D (one batch inversion
 * on the device), then a_j = u_{num_constraints + j} (j < num_inputs) plus the column sums of u_i * A[i][j]; b, c the same over B, C (no instance
 * terms).  t: 4 words (montgomery != 0: an ark-ff Fr, else canonical).  out_a / out_b / out_c: num_vars x 4 words each, out_zt: Z(t) = t^D - 1, all
 * canonical or (montgomery != 0) Fr limbs; any output may be NULL.  *out_domain_size = D.  DGPU_E_BADARG: a bad handle, or Z(t) = 0 (t in the
 * domain; the reference draws t with sample_element_outside_domain, generator.rs:284). */
int32_t dgpu_qap_instance_map(uint64_t r1cs, const uint64_t t[4], int32_t montgomery, uint64_t *out_a, uint64_t *out_b, uint64_t *out_c,
                              uint64_t out_zt[4], size_t *out_domain_size);
/* dgpu_legogroth16_setup replaces generate_parameters_and_extra_info_with_qap (legogroth16/src/generator.rs:245-442) with the toxic waste passed
 * in (the reference draws it from `rng`, :220-232, :283) and the QAP reduction's key scalars (r1cs_to_qap.rs:212-223): the instance map above,
 * mix_j = beta a_j + alpha b_j + c_j, gamma_abc = mix[..n] / gamma (n = num_inputs + commit_witness_count), l = mix[n..] / delta, h_i = Z(t) / delta
 * t^i (i < D - 1), then every FixedBase::msm (:335-406) as a window-table product from the scalars on the device: the five queries become resident
 * bases handles exactly as dgpu_window_table_mul_to_bases_* makes them (an identity where a scalar is zero).
 *   waste          alpha, beta, gamma, delta, eta, t: 6 x 4 words (montgomery != 0: ark-ff Fr limbs, else canonical)
 *   g1_xy / g2_xy  the generators (affine ABI words)
 *   out_handles    a_query, b_g1_query, b_g2_query, h_query (D - 1 points), l_query: bases handles the caller frees with dgpu_bases_free
 *   out_g1         7 x 12 words: alpha_g1, beta_g1, delta_g1, eta_gamma_inv_g1, eta_delta_inv_g1, a_query[0], b_g1_query[0]
 *   out_g2         4 x 24 words: beta_g2, delta_g2, gamma_g2, b_g2_query[0]
 *   gamma_abc_g1   gamma_abc_cap x 12 words of the caller's; the first num_inputs + commit_witness_count rows are written
 *   query_xy / query_inf   NULL, or five pointers each (same order as out_handles; any may be NULL): host copies of the queries as affine ABI
 *                  words and one identity flag per point (a, b_g1, b_g2: num_vars points, h: D - 1, l: num_vars - n) — what a caller that holds
 *                  keys as Vec<G1Affine> or serializes them needs
 *   out_domain_size  D (may be NULL)
 * A dgpu_lego_pk whose handles are out_handles and whose point members point into out_g1 / out_g2 / gamma_abc_g1 proves with dgpu_legogroth16_prove
 * on the same r1cs.  DGPU_E_BADARG: a bad handle or NULL pointer, commit_witness_count > num_vars - num_inputs (InsufficientWitnessesForCommitment,
 * :289-294), gamma or delta = 0 (UnexpectedIdentity), Z(t) = 0, gamma_abc_cap < num_inputs + commit_witness_count.  A refused or failing call
 * leaves no handle and no device allocation behind.  Runs on the circuit's device; stage timers setup.instance_map and setup.fixed_base. */
int32_t dgpu_legogroth16_setup(uint64_t r1cs, size_t commit_witness_count, const uint64_t waste[24], const uint64_t g1_xy[12], const uint64_t g2_xy[24],
                               int32_t montgomery, uint64_t out_handles[5], uint64_t *out_g1, uint64_t *out_g2, uint64_t *gamma_abc_g1, size_t gamma_abc_cap,
                               uint64_t **query_xy, uint8_t **query_inf, size_t *out_domain_size);

/* ---- accumulator manager: the witnesses of many holders after a batch of additions and removals ----
 * Witness::compute_update_using_secret_key_after_batch_updates (vb_accumulator/src/witness.rs:238-285) and its additions-only and removals-only
 * forms (:165-233: the same formula with an empty list), with the evaluations of vb_accumulator/src/batch_utils.rs:81-470 (Poly_d, Poly_v_A, Poly_v_D,
 * Poly_v_AD ::eval_direct / eval_direct_on_batch).  For every element y_i of a holder:
 *     f_i = d_A(y_i) / d_D(y_i)     (the reference's returned d_factor)           d_U(y) = prod_{u in U} (u - y), 1 for an empty U
 *     g_i = v_AD(y_i) / d_D(y_i)
 *     C_i' = f_i C_i + g_i V          (V: the accumulator the reference's variant expects, witness.rs:162-164,196-198,235-237)
 * O(m (n_add + n_rem)) field products and 2 m scalar multiplications on the device; alpha is used on the host only, for O(n_add + n_rem) table entries
 * whose device copy is zeroed before the call returns.  Nothing is cached between calls.
 *   additions / removals   n_add / n_rem x 4 words, in the order the manager applied them (either list may be empty: NULL is fine then)
 *   alpha                  the secret key
 *   elements               m x 4 words
 *   montgomery != 0        every Fr input and output is ark-ff Montgomery limbs (Fr as it lies in memory); else canonical, any 256-bit input taken mod r
 *   witnesses_xy, out_xy   affine Montgomery limbs, x then y; accumulator_xy likewise.  An identity witness or accumulator is all-zero words (the convention of
 *                          dgpu_g1_mul_add_batch's inputs); an identity result is zero words and out_inf[i] = 1
 * A holder whose element is among the removals has d_D = 0: it gets d_factor = 0 and the identity (zero words, out_inf = 1), the point the reference's
 * arithmetic yields there (its batch inversion leaves the zero).  A holder whose element was just added gets d_factor = 0 and g_i V.
 * m = 0: DGPU_OK, nothing is read.  DGPU_E_BADARG: a NULL pointer with a non-zero count, m >= 2^31, n_add + n_rem >= 2^31, an addition or a removal equal
 * to -alpha (a table entry would be zero or need its inverse; the reference computes garbage there) — all decided before the device is looked at.  No size
 * threshold.  Thread-safe like every other entry point.  Stage timers acc.prep, acc.factors, acc.table_mul, acc.scale. */
int32_t dgpu_accumulator_update_factors(const uint64_t *additions, size_t n_add, const uint64_t *removals, size_t n_rem,
                                        const uint64_t alpha[4], const uint64_t *elements /* m*4 */, size_t m, int32_t montgomery,
                                        uint64_t *f /* m*4 */, uint64_t *g /* m*4 */);
int32_t dgpu_accumulator_update_witnesses_g1(const uint64_t *additions, size_t n_add, const uint64_t *removals, size_t n_rem,
                                             const uint64_t alpha[4], const uint64_t *elements /* m*4 */, const uint64_t *witnesses_xy /* m*12 */, size_t m,
                                             const uint64_t accumulator_xy[12], int32_t montgomery,
                                             uint64_t *d_factors /* m*4 */, uint64_t *out_xy /* m*12 */, uint8_t *out_inf /* m */);

/* ---- accumulator: the update from public information (section 4.1 of the paper), both halves ----
 * dgpu_accumulator_omega_g1 is the manager's half, Omega::new (vb_accumulator/src/batch_utils.rs:498-509): the coefficients c_j of v_AD
 * (Poly_v_AD::generate, :115-140,271-300,433-440), each scaling the accumulator V from before the update: omega_j = c_j V.  v_AD has max(n_add, n_rem)
 * coefficients, so its values at the N-th roots of unity (N the next power of two; the passes of the witness update, O(N (n_add + n_rem)) products) and ONE
 * inverse transform of size N give them without polynomial arithmetic.  alpha is used on the host only; the device copies of the tables, the
 * evaluations and the coefficients are zeroed before the call returns, and nothing is cached.
 *   omega_xy, omega_inf    max(n_add, n_rem) entries: affine Montgomery limbs and identity flags.  A zero coefficient, and every entry of an identity
 *                          accumulator, is an identity entry: zero words, flag 1
 *   omega_len              ark-poly drops trailing zero coefficients: the index of the last non-zero coefficient plus one (0 for two empty lists or the zero
 *                          polynomial, e.g. one addition and one removal of the same element); entries from omega_len on are identities
 * Omega::new_for_kb_positive_accumulator (:514-527) is this call with empty additions, the members prf(r) as removals, and the negated accumulator.
 * DGPU_E_BADARG (before the device is looked at): a NULL pointer with a non-zero count, a count >= 2^31, max(n_add, n_rem) > DGPU_ACC_OMEGA_MAX = 2^18 (the
 * work is quadratic: longer batches want a product tree), an addition or a removal equal to -alpha.  Both lists empty: DGPU_OK, omega_len = 0, no device
 * needed.  Stage timers acc.prep, acc.omega_eval, acc.omega_intt, acc.omega_mul.
 *
 * dgpu_accumulator_update_witnesses_public_g1 is the holders' half, m times Witness::compute_update_using_public_info_after_batch_updates
 * (vb_accumulator/src/witness.rs:292-314) with Omega::evaluate (batch_utils.rs:664-691), without the secret key:
 *     f_i = d_A(y_i) / d_D(y_i),  s_i = 1 / d_D(y_i),  C_i' = f_i C_i + sum_j (s_i y_i^j) omega_j
 * The m x n_omega scaled powers are made on the device, straight into the scalar rows of the many-row MSM; they never exist on the host.
 *   omega_xy, omega_inf    n_omega entries as dgpu_accumulator_omega_g1 writes them (omega_inf may be NULL: an entry of zero words is an identity either way).
 *                          n_omega is not tied to the list lengths; n_omega = 0 gives C_i' = f_i C_i
 *   d_factors, out_xy, out_inf   as dgpu_accumulator_update_witnesses_g1
 *   ok                     ok[i] = 0 for a holder whose element is among the removals (d_D = 0, the reference's Err(CannotBeZero)): that holder gets
 *                          d_factor = 0 and the identity (zero words, out_inf = 1), the call still returns DGPU_OK and every other holder gets ok[i] = 1
 * Up to 8192 entries of omega (and dgpu_set_small_msm_max) the rows run through the many-row MSM kernels, in chunks of rows; beyond, row by row through
 * the single-MSM driver.  m = 0: DGPU_OK.  DGPU_E_BADARG as above (n_omega >= 2^31 too).  No size threshold.  Thread-safe; one slot per call.
 * Stage timers acc.prep, acc.pub_factors, acc.pub_rows, msm.many_tree, msm.many_fold, acc.scale. */
#define DGPU_ACC_OMEGA_MAX ((size_t)1 << 18)
int32_t dgpu_accumulator_omega_g1(const uint64_t *additions, size_t n_add, const uint64_t *removals, size_t n_rem,
                                  const uint64_t alpha[4], const uint64_t accumulator_xy[12], int32_t montgomery,
                                  uint64_t *omega_xy /* max(n_add, n_rem) * 12 */, uint8_t *omega_inf /* max(n_add, n_rem) */, size_t *omega_len);
int32_t dgpu_accumulator_update_witnesses_public_g1(const uint64_t *additions, size_t n_add, const uint64_t *removals, size_t n_rem,
                                                    const uint64_t *omega_xy /* n_omega * 12 */, const uint8_t *omega_inf /* n_omega or NULL */, size_t n_omega,
                                                    const uint64_t *elements /* m*4 */, const uint64_t *witnesses_xy /* m*12 */, size_t m, int32_t montgomery,
                                                    uint64_t *d_factors /* m*4 */, uint64_t *out_xy /* m*12 */, uint8_t *out_inf /* m */, uint8_t *ok /* m */);

/* ---- accumulator manager: issuing membership and non-membership witnesses ----
 * dgpu_accumulator_d_for_batch is UniversalAccumulator::compute_d_for_batch_given_members (vb_accumulator/src/universal.rs:479-495; the same double loop
 * opens get_non_membership_witnesses_for_batch, :564-575): for every non-member y_i the product over ALL members of the accumulator ("This is expensive
 * as a product involving all accumulated elements is needed", :461-463),
 *     d_out_i = d_in_i prod_{j < n} (member_j - y_i)          d_in = NULL: one
 * m n field products on the device, n being the size of the accumulator and not of a batch.  d_in is the reference's "partition the members, multiply the
 * outputs" (:476-478) done inside the call: feed the d_out of one partition as the d_in of the next.
 *   members / non_members  n / m x 4 words; montgomery as above (it speaks for members, non_members, d_in and d_out)
 *   nonzero                nonzero[i] = (d_out_i != 0): 0 marks a y_i that IS a member (or a zero d_in)
 * n = 0 copies d_in (or writes ones).  Members from the host travel in passes of at most 2^20 entries; the running products stay on the device between them.
 * Nothing here is secret, so nothing is wiped.
 * dgpu_accumulator_d_for_batch_resident reads the members from a resident scalar vector instead (a dgpu_scalars_upload handle, which holds canonical words
 * after the upload whatever form they came in): entries [offset, offset + n) straight out of it, nothing but the non-members is uploaded, and one handle
 * serves every batch and every partition.  montgomery then speaks for non_members, d_in and d_out only.  DGPU_E_BADARG for a handle that is not a scalar
 * vector, one of another device context than the calling thread's, or a range past its end.
 *
 * dgpu_accumulator_non_membership_witnesses_g1 is compute_non_membership_witnesses_for_batch_given_d (universal.rs:499-535):
 *     C_i = ((f_V - d_i) / (y_i + alpha)) params_gen
 * and dgpu_accumulator_membership_witnesses_g1 is compute_membership_witnesses_for_batch (vb_accumulator/src/positive.rs:369-381):
 *     C_i = (1 / (y_i + alpha)) V
 * The inverses are made on the host (one batch inversion per share of the host threads; alpha is used on the host only), the scalars on the device, straight
 * into the scalar buffer of a window-table multiplication whose table is built in the call's workspace; the points come back normalised.
 *   d, non_members / members   m x 4 words; f_V, alpha: 4 words; montgomery as above
 *   params_gen_xy, accumulator_xy, out_xy, out_inf   as the witnesses of dgpu_accumulator_update_witnesses_g1: an identity base (zero words) gives identities
 *   ok                     a zero d_i is the reference's Err(CannotBeZero): that entry gets ok[i] = 0, zero words and out_inf[i] = 1, every other entry ok[i] = 1,
 *                          and the call returns DGPU_OK (the convention of dgpu_accumulator_update_witnesses_public_g1)
 * A y_i equal to -alpha has no inverse: DGPU_E_BADARG, decided on the host before the device is looked at (as for an addition equal to -alpha above).  The
 * device copies of the inverses, the scalars and the table are zeroed on every return path, the host copies too; nothing is cached.
 *
 * All four: m = 0 is DGPU_OK and reads nothing.  DGPU_E_BADARG for a NULL pointer with a non-zero count, m >= 2^31 or n >= 2^31 — every argument check comes
 * before the device is looked at.  No size threshold.  Thread-safe; one slot per call; a second call of a shape allocates nothing.  Stage timers acc.d_prep,
 * acc.d_eval, acc.issue_scalars, acc.table_mul. */
int32_t dgpu_accumulator_d_for_batch(const uint64_t *members /* n*4 */, size_t n, const uint64_t *non_members /* m*4 */, size_t m, int32_t montgomery,
                                     const uint64_t *d_in /* m*4 or NULL */, uint64_t *d_out /* m*4 */, uint8_t *nonzero /* m */);
int32_t dgpu_accumulator_d_for_batch_resident(uint64_t members /* dgpu_scalars_upload handle */, size_t offset, size_t n,
                                              const uint64_t *non_members /* m*4 */, size_t m, int32_t montgomery,
                                              const uint64_t *d_in /* m*4 or NULL */, uint64_t *d_out /* m*4 */, uint8_t *nonzero /* m */);
int32_t dgpu_accumulator_non_membership_witnesses_g1(const uint64_t *d /* m*4 */, const uint64_t *non_members /* m*4 */, size_t m, const uint64_t f_V[4],
                                                     const uint64_t alpha[4], const uint64_t params_gen_xy[12], int32_t montgomery,
                                                     uint64_t *out_xy /* m*12 */, uint8_t *out_inf /* m */, uint8_t *ok /* m */);
int32_t dgpu_accumulator_membership_witnesses_g1(const uint64_t *members /* m*4 */, size_t m, const uint64_t alpha[4], const uint64_t accumulator_xy[12],
                                                 int32_t montgomery, uint64_t *out_xy /* m*12 */, uint8_t *out_inf /* m */);

/* ---- accumulator proofs in bulk: a status per proof, or one verdict (crypto_amd/csrc/dock_acc_pok.hip, acc_pok_kernels.hip.h) ----
 * The CDH proofs of the VB accumulator (vb_accumulator/src/proofs_cdh.rs: MembershipProof::verify :138-149, NonMembershipProof::verify with
 * verify_except_pairing :365-387, :481-523, over short_group_sig/src/weak_bb_sig_pok_cdh.rs:145-287, schnorr_pok/src/discrete_log.rs:247-253 and
 * schnorr_pok/src/partial.rs:149-166) for n proofs against ONE accumulator value V and one key: the revocation half of what the verifier of presentations runs
 * per credential shown (the BBS+ half: dgpu_bbs_plus_pok_verify_each_g1 below).  A verifier groups its presentations by accumulator epoch; per-row accumulator
 * values are not served.  The KB universal accumulator's CDH proofs wrap the same MembershipProof (kb_universal_accumulator/proofs_cdh.rs), so the membership
 * calls serve both of its proof kinds.
 *   accumulator_xy, p_xy, q_xy   V, params.P and Q: 12 words each, affine Montgomery coordinates; all-zero words are the identity
 *   pk_pc, ptilde_pc  the prepared coefficients (DGPU_G2_PREPARED_WORDS words each, dgpu_g2_prepare / ark-ec G2Prepared) of pk = alpha P~ and of P~
 *   points       membership: n x 3 x 12 words, A', Abar, T (sc.t) of proof i at points + 36 i
 *                non-membership: n x 5 x 12 words, C', Cbar, J, T1 (t_1), T2 (sc_2.t) of proof i at points + 60 i
 *   responses    membership: n x 2 scalars, z1 (sc.response1, over V) and z2 (sc.response2, over -A')
 *                non-membership: n x 3 scalars, s_r and s_y (responses 0 and 1 of sc_resp_1) and s_d (sc_2.response, also response 2 of the first relation)
 *                A partial proof (verify_partial, resp_for_element) needs no path of its own: the caller writes the element's response into z2 or s_y
 *   challenge    n scalars.  montgomery != 0: ark-ff `&[Fr]` limbs; else canonical words, any 256-bit value counting modulo r
 * The reference's checks, in the order it returns their errors:
 *   membership        1  A' != O                                                      else InvalidProof
 *                     2  z1 V - z2 A' - c Abar - T = O                                else InvalidProof
 *                     3  e(A', pk) e(-Abar, P~) = 1                                   else InvalidProof        (the reference's e(Abar, P~) e(-A', pk) = 1 inverted)
 *   non-membership    1  C' != O                                                      else CannotBeZero
 *                     2  J != O                                                       else CannotBeZero
 *                     3  s_d Q - c J - T2 = O                                         else IncorrectRandomizedWitness
 *                     4  s_r V - s_y C' - s_d P - c Cbar - T1 = O                     else SchnorrError(InvalidResponse)
 *                     5  e(C', pk) e(-Cbar, P~) = 1                                   else IncorrectRandomizedWitness
 *
 * The two ..._verify_each_g1 calls write status[i] = 0 (verified) or the number of the FIRST check that fails.  Per chunk of rows one device pipeline: the own
 * scalars (z1, -z2, -c, -1), respectively (s_d, -c, -1 | s_r, -s_y, -s_d, -c, -1) (k_acc_pok_own), the bases [V, A', Abar, T], respectively
 * [Q, J, T2 | V, C', P, Cbar, T1] and the two sides of the pairing (k_acc_pok_stage: the shared points are copied into every row, -Abar is a flip of y), one
 * 4-term segment per row, respectively a 3-term and a 5-term one, of the segmented small MSM, the two-pair pairing check with the shared lines of pk and P~, and
 * k_acc_pok_verdict; only the n status bytes come back.
 *
 * The two ..._verify_batch_g1 calls: ONE verdict.  With rho = random (rho = 0 mod r: DGPU_E_BADARG, decided on the host); an identity A', C' or J anywhere gives
 * *ok = 0, decided on the host on the zero words.  Membership, u_i = t_i = rho^i: *ok = 1 iff
 *     (sum u_i z1_i) V + sum_i [ -u_i z2_i A'_i - u_i c_i Abar_i - u_i T_i ] = O      and      e(sum t_i A'_i, pk) e(-sum t_i Abar_i, P~) = 1
 * Non-membership, u_i = rho^(2i) on check 4, v_i = rho^(2i+1) on check 3, t_i = rho^i on the pairing: *ok = 1 iff
 *     (sum u_i s_r_i) V - (sum u_i s_d_i) P + (sum v_i s_d_i) Q + sum_i [ -u_i s_y_i C'_i - u_i c_i Cbar_i - v_i c_i J_i - u_i T1_i - v_i T2_i ] = O
 *     e(sum t_i C'_i, pk) e(-sum t_i Cbar_i, P~) = 1
 * — the one (three) shared-point coefficients and every weight on the device (k_acc_pok_col_sums, k_col_finish: two passes, no atomics), one variable-base
 * MSM over the chunk's 3 n (5 n) own points and one each over the two pairing sides, ONE small MSM over the shared points, one two-pair Miller loop and final
 * exponentiation.  n = 0 gives *ok = 1.  For a random rho a batch with a failing proof passes with probability at most 2n / r per equation; rho = 1 adds the rows
 * up unweighted, so errors that cancel between rows pass, as they would in the reference with that scalar.
 *
 * All four take the points as members of the prime-order subgroup, as the reference does after deserialising with validation: validate untrusted ones first
 * (dgpu_g1_validate_batch).  n = 0 is DGPU_OK without touching a device or any pointer; with n > 0 a NULL pointer or n >= 2^31 is DGPU_E_BADARG before the device
 * is looked at; then DGPU_E_NODEVICE.  Never DGPU_E_TOO_SMALL.  Thread-safe; one slot per call; a second call of a shape allocates nothing.  Chunks: each 4096
 * rows (91 KB of lines and products per row), batch 65536; the development surface's dgpu_set_many_chunk_rows cuts both.  Nothing secret passes through.  Stage
 * timers acc.pok_own, acc.pok_stage, acc.pok_verdict, acc.pok_columns beside bbs.lines .. bbs.final_exp (the shared pairing check) and those of the MSMs. */
int32_t dgpu_accumulator_membership_proofs_verify_each_g1(const uint64_t accumulator_xy[12], const uint64_t *pk_pc, const uint64_t *ptilde_pc,
                                                          const uint64_t *points /* n*36 */, const uint64_t *responses /* n*8 */,
                                                          const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery, uint8_t *status /* n */);
int32_t dgpu_accumulator_membership_proofs_verify_batch_g1(const uint64_t accumulator_xy[12], const uint64_t *pk_pc, const uint64_t *ptilde_pc,
                                                           const uint64_t *points /* n*36 */, const uint64_t *responses /* n*8 */,
                                                           const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok);
int32_t dgpu_accumulator_non_membership_proofs_verify_each_g1(const uint64_t accumulator_xy[12], const uint64_t p_xy[12], const uint64_t q_xy[12],
                                                              const uint64_t *pk_pc, const uint64_t *ptilde_pc, const uint64_t *points /* n*60 */,
                                                              const uint64_t *responses /* n*12 */, const uint64_t *challenge /* n*4 */, size_t n,
                                                              int32_t montgomery, uint8_t *status /* n */);
int32_t dgpu_accumulator_non_membership_proofs_verify_batch_g1(const uint64_t accumulator_xy[12], const uint64_t p_xy[12], const uint64_t q_xy[12],
                                                               const uint64_t *pk_pc, const uint64_t *ptilde_pc, const uint64_t *points /* n*60 */,
                                                               const uint64_t *responses /* n*12 */, const uint64_t *challenge /* n*4 */, size_t n,
                                                               int32_t montgomery, const uint64_t random[4], int32_t *ok);

/* ---- BBS+ signatures in bulk: sign many, verify many, a verdict per signature or one for all (crypto_amd/csrc/dock_bbs.hip, bbs_kernels.hip.h) ----
 * SignatureG1 / SignatureParamsG1 / PublicKeyG2 of bbs_plus/src/signature.rs:138-296 for n signatures of ONE key, each call one device pipeline per chunk
 * of rows instead of the caller's chain dgpu_msm_g1_handle_many -> dgpu_g1_mul_add_batch -> dgpu_multi_pairing_segments with a PCIe round trip between each.
 *   params        a plain G1 bases handle (dgpu_bases_upload_g1) holding exactly [g1, h_0, h_1 .. h_L] (SignatureParamsG1 { g1, g2, h_0, h }): the call runs on
 *                 the context that owns it and pins it.  A length other than L + 2 is the reference's MessageCountIncompatibleWithSigParams, L = 0 its
 *                 NoMessageToSign: DGPU_E_BADARG, as is an unknown, busy, sharded or precomputed handle or one of another kind
 *   messages      n rows of L scalars, row i at messages + 4 * row_stride * i (row_stride >= L, counted in scalars; what lies between rows is never read)
 *   e, s, sk, random   4 words each (e, s: n x 4).  montgomery != 0: ark-ff `&[Fr]` limbs; else canonical words, any 256-bit value counting modulo r
 *   sig_a, out_a  n x 12 words, affine Montgomery coordinates; all-zero words are the identity
 *   pk_pc, g2_pc  the prepared coefficients (DGPU_G2_PREPARED_WORDS words each, dgpu_g2_prepare / ark-ec G2Prepared) of the public key w = x g2 and of g2
 *
 * dgpu_bbs_plus_sign_many_g1 is SignatureG1::new (signature.rs:138-211) with the caller's e_i and s_i in place of its two `rand` draws (:178, :187), so that
 * the call is deterministic:
 *     A_i = (x + e_i)^-1 (g1 + s_i h_0 + sum_j m_ij h_j)                    b_i: setup.rs:128-146, the inverse: signature.rs:201-206
 * The inverses are made on the host (one batch inversion per share of the host threads; x is used on the host only), everything else on the device: row i of
 * the many-row MSM's scalars becomes (x + e_i)^-1 (1, s_i, m_i1 .. m_iL) (k_bbs_rows), so the MSM over params yields A_i itself, normalised.
 * bad[i] = 1 and zero words in out_a where no signature exists: x + e_i = 0 (the reference draws e again there) or b_i the identity; such a row does not
 * disturb its neighbours and the call returns DGPU_OK.  The host copy of the inverses and the device copies of the inverses and of the rows that carry them are
 * zeroed on every return path before the slot is released; nothing is cached.
 *
 * dgpu_bbs_plus_verify_each_g1 is SignatureG1::verify (signature.rs:272-296) once per row, in the form the reference uses (:284-295):
 *     ok[i] = 1  iff  A_i is not the identity (ZeroSignature, :280-282)  and  e(A_i, w) e(e_i A_i - b_i, g2) = 1
 * b_i comes from the many-row MSM over params, e_i A_i - b_i from k_g1_scale_quad with b_i as its addend (the host splits -e_i, an input, and the kernel negates
 * its result: nothing of the device is waited for), the lines of w and g2 are shared by every row (k_lines_from_prepared), the products run over slices of two,
 * the Miller loop's tail and the final exponentiation on the device compare with one: only the n verdict bytes come back.  A zero Miller output is a rejection;
 * a pair whose G1 member is the identity contributes one, as everywhere in the library.  The points are taken as members of the curve's prime-order subgroup
 * (k_g1_scale_quad's endomorphism and the pairing assume it, as dgpu_legogroth16_verify_each does): validate untrusted ones first (dgpu_g1_validate_batch).
 *
 * dgpu_bbs_plus_verify_batch_g1: ONE verdict for all rows by the random linear combination the reference reaches through RandomizedPairingChecker
 * (utils/src/randomized_pairing_check.rs:96-158); row i has the weight rho^i, rho = random (rho = 0 mod r: DGPU_E_BADARG, decided on the host).  The pairs that
 * share w and g2 are merged before the pairing:
 *     P1 = sum rho^i A_i,   P2 = sum rho^i e_i A_i - sum_k c_k H_k,   c = sum_i rho^i (1, s_i, m_i1 .. m_iL),   H = the L + 2 points of params
 * — the column sums c_k, the weights and rho^i e_i on the device (k_bbs_col_sums, k_col_finish: two passes, no atomics), two variable-base MSMs of n terms
 * over the A_i, ONE MSM of L + 2 terms over params, one two-pair Miller loop and one final exponentiation.  *ok = 1 iff the result is one and no A_i is the
 * identity; n = 0 gives *ok = 1.  rho = 1 adds the rows up unweighted: errors that cancel between rows pass, as they would in the reference with that scalar.
 *
 * All three: n = 0 is DGPU_OK without touching a device or any pointer.  With n > 0 a NULL pointer, row_stride < L, L = 0, n or row_stride >= 2^31 is
 * DGPU_E_BADARG, decided before the device is looked at; DGPU_E_NODEVICE comes before anything the device would decide (the handle).  Never DGPU_E_TOO_SMALL.
 * Thread-safe like every entry point; one slot per call; a second call of a shape allocates nothing.  Rows travel in chunks so that the slot's grow-only
 * workspace stays bounded whatever n: sign min(4096, 2^17 / (L + 2)) rows (below ~80 MB), verify_each the same (at most 4096 rows: 91 KB of lines and
 * products per row, below ~0.5 GB), verify_batch min(65536, 2^20 / L) rows (below ~0.2 GB).  Rows longer than the many-row kernels accept (L + 2 above
 * dgpu_set_small_msm_max, or with it set to 0) take the single-row MSM driver row by row inside the call: correct, not fast.  Stage timers bbs.host_inverses,
 * bbs.glv_split, bbs.rows, bbs.columns, bbs.scale, bbs.lines, bbs.products, bbs.tail, bbs.final_exp beside those of the MSM. */
int32_t dgpu_bbs_plus_sign_many_g1(uint64_t params, size_t L, const uint64_t sk[4], const uint64_t *messages /* n rows */, size_t row_stride,
                                   const uint64_t *e /* n*4 */, const uint64_t *s /* n*4 */, size_t n, int32_t montgomery,
                                   uint64_t *out_a /* n*12 */, uint8_t *bad /* n */);
int32_t dgpu_bbs_plus_verify_each_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a /* n*12 */,
                                     const uint64_t *e /* n*4 */, const uint64_t *s /* n*4 */, const uint64_t *messages /* n rows */, size_t row_stride,
                                     size_t n, int32_t montgomery, uint8_t *ok /* n */);
int32_t dgpu_bbs_plus_verify_batch_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a /* n*12 */,
                                      const uint64_t *e /* n*4 */, const uint64_t *s /* n*4 */, const uint64_t *messages /* n rows */, size_t row_stride,
                                      size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok);

/* ---- BBS+ proofs of knowledge in bulk: a verdict per proof, or one for all (crypto_amd/csrc/dock_bbs.hip, bbs_pok_kernels.hip.h) ----
 * PoKOfSignatureG1Proof::verify (bbs_plus/src/proof.rs:529-611, schnorr_pok/src/discrete_log.rs:248-253) for n proofs under ONE key: what the verifier of
 * presentations runs per credential shown.  It sees no e, s or hidden message, so the three calls above do not serve it.  params, pk_pc, g2_pc, montgomery,
 * row_stride and the identity as all-zero words are as above; further
 *   h_0          the second point of params again, 12 words (the caller has it; the driver need not read it back out of the prepared records)
 *   points       n x 5 x 12 words: A', Abar, d, T1 (sc_resp_1.t), T2 of proof i at points + 60 i
 *   resp_fixed   n x 4 scalars: z1, z2 (sc_resp_1.response1 / .response2, over A' and h_0), z3 (over d, for -r3), z4 (over h_0, for s')
 *   values       n rows of L scalars, row i at values + 4 * row_stride * i: entry j is the revealed message m_ij, or the response z_ij of a hidden one.  A proof
 *                with partial responses (sc_partial_resp_2 and missing_responses) needs no path of its own: the caller writes the missing responses into the row
 *   revealed     n x L bytes, non-zero = revealed; every row carries its own pattern
 *   challenge    n scalars
 * The reference's four checks, with the second Schnorr check in row form over params: row i = (c_i, z4_i, y_i1 .. y_iL), y_ij = c_i m_ij where j is revealed and
 * z_ij where it is hidden, P_i = <row_i, params>:
 *     1  A'_i != O                                                                    else ZeroSignature
 *     2  z1 A' + z2 h_0 - c (Abar - d) - T1 = O                                       else FirstSchnorrVerificationFailed
 *     3  P_i + z3_i d_i - T2_i = O                                                    else SecondSchnorrVerificationFailed
 *     4  e(A'_i, w) e(-Abar_i, g2) = 1                                                else PairingCheckFailed
 *
 * dgpu_bbs_plus_pok_verify_each_g1 writes status[i] = 0 (verified) or the number of the FIRST check that fails, in the order the reference returns its errors.
 * Per chunk of rows one device pipeline: the rows and the own-point scalars (k_bbs_pok_rows, k_bbs_pok_own), P_i by the many-row MSM, the five-term sum of check 2
 * and z3 d - T2 as two segments per row of the segmented small MSM over points staged on the device (k_bbs_pok_stage: -Abar is a flip of y there), the
 * two-pair pairing check with the shared lines of w and g2, and k_bbs_pok_verdict; only the n status bytes come back.
 *
 * dgpu_bbs_plus_pok_verify_batch_g1: ONE verdict.  With rho = random (rho = 0 mod r: DGPU_E_BADARG, decided on the host) row i weighs check 2 with
 * u_i = rho^(2i), check 3 with v_i = rho^(2i+1) and the pairing with t_i = rho^i; *ok = 1 iff no A'_i is the identity and
 *     sum_k C_k H_k + sum_i [ u_i z1_i A'_i - u_i c_i Abar_i + (u_i c_i + v_i z3_i) d_i - u_i T1_i - v_i T2_i ] = O,
 *         C_0 = sum v_i c_i,  C_1 = sum (u_i z2_i + v_i z4_i),  C_(j+1) = sum v_i y_ij,  H = the L + 2 points of params
 *     e(sum t_i A'_i, w) e(-sum t_i Abar_i, g2) = 1
 * — the C_k and every weight on the device (k_bbs_pok_col_sums, k_col_finish: two passes, no atomics), one variable-base MSM over the chunk's 5 n own
 * points and one each over the A' and the Abar, ONE MSM over params, one two-pair Miller loop and final exponentiation.  n = 0 gives *ok = 1.  For a random
 * rho a batch with a failing proof passes with probability at most 3n / r per equation (the G1 equation is a polynomial of degree < 2n in rho, the pairing's of
 * degree < n); rho = 1 adds the rows up unweighted, so errors that cancel between rows pass, as they would in the reference with that scalar.
 *
 * Both take the points as members of the prime-order subgroup, as the reference does after deserialising with validation: validate untrusted ones first
 * (dgpu_g1_validate_batch).  n = 0 is DGPU_OK without touching a device or any pointer; with n > 0 a NULL pointer, row_stride < L, L = 0, n or row_stride
 * >= 2^31 is DGPU_E_BADARG before the device is looked at; then DGPU_E_NODEVICE, then the handle.  Never DGPU_E_TOO_SMALL.  Chunks: each
 * min(4096, 2^17 / (L + 2)) rows (below ~0.6 GB), batch min(65536, 2^20 / L); the development surface's dgpu_set_many_chunk_rows cuts both.  Nothing secret passes through.
 * Stage timers bbs.pok_rows, bbs.pok_stage, bbs.pok_verdict, bbs.pok_columns beside bbs.lines .. bbs.final_exp and those of the MSMs. */
int32_t dgpu_bbs_plus_pok_verify_each_g1(uint64_t params, size_t L, const uint64_t h_0[12], const uint64_t *pk_pc, const uint64_t *g2_pc,
                                         const uint64_t *points /* n*60 */, const uint64_t *resp_fixed /* n*16 */, const uint64_t *values /* n rows */,
                                         size_t row_stride, const uint8_t *revealed /* n*L */, const uint64_t *challenge /* n*4 */, size_t n,
                                         int32_t montgomery, uint8_t *status /* n */);
int32_t dgpu_bbs_plus_pok_verify_batch_g1(uint64_t params, size_t L, const uint64_t h_0[12], const uint64_t *pk_pc, const uint64_t *g2_pc,
                                          const uint64_t *points /* n*60 */, const uint64_t *resp_fixed /* n*16 */, const uint64_t *values /* n rows */,
                                          size_t row_stride, const uint8_t *revealed /* n*L */, const uint64_t *challenge /* n*4 */, size_t n,
                                          int32_t montgomery, const uint64_t random[4], int32_t *ok);

/* ---- BBS (2023) in bulk: sign, verify, and both proofs of knowledge (crypto_amd/csrc/dock_bbs.hip, bbs_kernels.hip.h, bbs23_kernels.hip.h) ----
 * The other half of the reference's bbs_plus crate: Signature23G1 (bbs_plus/src/signature_23.rs) and the two protocols that prove knowledge of one,
 * proof_23_cdl.rs (the prelude's PoKOfSignature23G1Proof, proof_system's PoKBBSSignature23G1) and proof_23_ietf.rs (the IETF draft's, PoKBBSSignature23IETFG1).
 * The scheme has no s and no h_0: params is a PLAIN G1 bases handle [g1, h_1 .. h_L] of exactly L + 1 points (another length, a precomputed handle or no
 * handle: DGPU_E_BADARG); pk_pc, g2_pc, messages, row_stride, e, montgomery, random and the identity as all-zero words are as in the BBS+ calls above.
 *
 * dgpu_bbs23_sign_many_g1 is Signature23G1::new (signature_23.rs:38-103, commitment = O) for n rows: A_i = (x + e_i)^-1 (g1 + sum_j m_ij h_j), row i of the
 * many-row MSM = (x + e_i)^-1 (1, m_i1 .. m_iL).  bad[i] = 1 and zero words where x + e_i = 0 or b_i = O.  The inverses are made on the host; their host and
 * device copies and the rows that carry them are zeroed on every return path, as in dgpu_bbs_plus_sign_many_g1.
 * dgpu_bbs23_verify_each_g1 is Signature23G1::verify (:136-160): ok[i] = 1 iff A_i != O and e(A_i, w) e(e_i A_i - b_i, g2) = 1.
 * dgpu_bbs23_verify_batch_g1: one verdict under the weights rho^i — the L + 1 column sums c_k, P1 = sum rho^i A_i, P2 = sum rho^i e_i A_i - sum_k c_k H_k, one
 * merged pair.  These three are the BBS+ drivers and kernels with ONE fixed column in front of the messages instead of two (k_bbs_rows, k_bbs_col_sums take
 * the count), so chunks, stage timers and every remark of the BBS+ block hold with L + 1 in place of L + 2.
 *
 * The two proofs of knowledge, n proofs under ONE key; values, revealed, challenge as in dgpu_bbs_plus_pok_verify_each_g1; row i = (c_i, y_i1 .. y_iL),
 * y_ij = c_i m_ij where j is revealed and z_ij where it is hidden, P_i = <row_i, params>:
 *   CDL (dgpu_bbs23_pok_verify_*; proof_23_cdl.rs:302-549)
 *     points      n x 5 x 12 words: Abar, Bbar, d, T1 (sc_resp_1.t), T2
 *     resp_fixed  n x 3 scalars: z1 (sc_resp_1.response1, over Abar), z2 (.response2, over d), z3 (the last response of sc_resp_2, over d)
 *     1  Abar != O                                                    else ZeroSignature
 *     2  z1 Abar + z2 d - c Bbar - T1 = O                             else FirstSchnorrVerificationFailed
 *     3  P_i + z3 d - T2 = O                                          else SecondSchnorrVerificationFailed
 *     4  e(Abar, w) e(-Bbar, g2) = 1                                  else PairingCheckFailed
 *   IETF (dgpu_bbs23_pok_ietf_verify_*; proof_23_ietf.rs:244-479)
 *     points      n x 3 x 12 words: Abar, Bbar, T
 *     resp_fixed  n x 2 scalars: z_a, z_b, the last two responses of sc_resp, over Abar and Bbar
 *     1  Abar != O                                                    else ZeroSignature
 *     3  P_i + z_a Abar + z_b Bbar - T = O                            else SecondSchnorrVerificationFailed (the name this protocol gives its only Schnorr check)
 *     4  e(Abar, w) e(-Bbar, g2) = 1                                  else PairingCheckFailed
 * ..._verify_each_g1 writes status[i] = 0 or the number of the FIRST failing check (the IETF call never writes 2).  Per chunk one device pipeline: the rows
 * and the own scalars (z1, z2, -c, -1 | z3, -1), respectively (z_a, z_b, -1) (k_bbs23_rows, k_bbs23_own), the bases [Abar, d, Bbar, T1 | d, T2], respectively
 * [Abar, Bbar, T] with Abar and -Bbar for the pairing (k_bbs23_stage), P_i by the many-row MSM, the segments by the segmented small MSM, the two-pair check,
 * k_bbs23_verdict (the segment over the parameters' check is compared with -P_i); only the n status bytes come back.
 * ..._verify_batch_g1: ONE verdict, rho = random (rho = 0 mod r: DGPU_E_BADARG).  *ok = 1 iff no Abar_i is the identity and
 *   CDL, u_i = rho^(2i), v_i = rho^(2i+1), t_i = rho^i:
 *     sum_k C_k H_k + sum_i [ u z1 Abar - u c Bbar + (u z2 + v z3) d - u T1 - v T2 ]_i = O,    C_0 = sum v_i c_i,  C_j = sum v_i y_ij
 *   IETF, u_i = t_i = rho^i:
 *     sum_k C_k H_k + sum_i u_i [ z_a Abar + z_b Bbar - T ]_i = O,                              C_0 = sum u_i c_i,  C_j = sum u_i y_ij
 *   both: e(sum t_i Abar_i, w) e(-sum t_i Bbar_i, g2) = 1
 * (k_bbs23_col_sums, k_col_finish: two passes, no atomics; one MSM over the chunk's own points, one each over the Abar and the Bbar, ONE over params; a
 * G1 sum that is not the identity refuses before the pairing).  For a random rho a batch with a failing proof passes with probability at most 2n / r (CDL) or
 * n / r (IETF) per equation; rho = r - 1 makes every CDL u_i one and rho = 1 every IETF u_i: errors that cancel between rows then pass.
 *
 * All seven: n = 0 is DGPU_OK without touching a device or any pointer (an empty batch verifies); with n > 0 a NULL pointer, row_stride < L, L = 0, n or
 * row_stride >= 2^31 is DGPU_E_BADARG before the device is looked at; then DGPU_E_NODEVICE, then the handle.  Points are taken as validated members of the
 * subgroup.  Chunks (UNMEASURED): the BBS+ rules with L + 1 in place of L + 2; dgpu_set_many_chunk_rows of the development surface cuts all seven.  Stage
 * timers bbs23.pok_rows, bbs23.pok_stage, bbs23.pok_verdict, bbs23.pok_columns beside the BBS+ block's. */
int32_t dgpu_bbs23_sign_many_g1(uint64_t params, size_t L, const uint64_t sk[4], const uint64_t *messages /* n rows */, size_t row_stride,
                                const uint64_t *e /* n*4 */, size_t n, int32_t montgomery, uint64_t *out_a /* n*12 */, uint8_t *bad /* n */);
int32_t dgpu_bbs23_verify_each_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a /* n*12 */,
                                  const uint64_t *e /* n*4 */, const uint64_t *messages /* n rows */, size_t row_stride, size_t n, int32_t montgomery,
                                  uint8_t *ok /* n */);
int32_t dgpu_bbs23_verify_batch_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *sig_a /* n*12 */,
                                   const uint64_t *e /* n*4 */, const uint64_t *messages /* n rows */, size_t row_stride, size_t n, int32_t montgomery,
                                   const uint64_t random[4], int32_t *ok);
int32_t dgpu_bbs23_pok_verify_each_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points /* n*60 */,
                                      const uint64_t *resp_fixed /* n*12 */, const uint64_t *values /* n rows */, size_t row_stride,
                                      const uint8_t *revealed /* n*L */, const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery, uint8_t *status /* n */);
int32_t dgpu_bbs23_pok_verify_batch_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points /* n*60 */,
                                       const uint64_t *resp_fixed /* n*12 */, const uint64_t *values /* n rows */, size_t row_stride,
                                       const uint8_t *revealed /* n*L */, const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery,
                                       const uint64_t random[4], int32_t *ok);
int32_t dgpu_bbs23_pok_ietf_verify_each_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points /* n*36 */,
                                           const uint64_t *resp_fixed /* n*8 */, const uint64_t *values /* n rows */, size_t row_stride,
                                           const uint8_t *revealed /* n*L */, const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery,
                                           uint8_t *status /* n */);
int32_t dgpu_bbs23_pok_ietf_verify_batch_g1(uint64_t params, size_t L, const uint64_t *pk_pc, const uint64_t *g2_pc, const uint64_t *points /* n*36 */,
                                            const uint64_t *resp_fixed /* n*8 */, const uint64_t *values /* n rows */, size_t row_stride,
                                            const uint8_t *revealed /* n*L */, const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery,
                                            const uint64_t random[4], int32_t *ok);

/* ---- PS (Coconut) signatures in bulk: sign, verify, proofs of knowledge (crypto_amd/csrc/dock_ps.hip, ps_kernels.hip.h) ----
 * The Pointcheval-Sanders signature of the reference's coconut crate (coconut/src/signature/ps_signature.rs, proof_system's PoKPSSignature) and the proof of
 * knowledge of one (coconut/src/proof/signature_pok/).  A signature is TWO G1 points (sigma_1, sigma_2), 2 x 12 words; its verification lives in G2:
 *   pk_g2   ONE plain G2 bases handle [alpha_tilde, beta_tilde_1 .. beta_tilde_L, g_tilde] of exactly L + 2 points (another length, a precomputed handle, a G1
 *           handle or no handle: DGPU_E_BADARG).  PublicKey::beta, the G1 copies, is needed by none of the four calls.
 *   g_table a dgpu_window_table_g1 handle of SignatureParams::g.
 *   g_tilde_pc / all_pc   the prepared coefficients (dgpu_g2_prepare) of g_tilde, respectively of all L + 2 points in the handle's order.
 * messages, row_stride, montgomery, random and the identity as all-zero words are as in the BBS+ calls above.
 *
 * dgpu_ps_sign_many_g1 is Signature::new (ps_signature.rs:46-64) for n rows with r_i standing in for its `rand` draw: sigma_1_i = r_i g and
 * sigma_2_i = (r_i (x + sum_j y_j m_ij)) g — the reference's h = g r; sigma_2 = h (..) as the same group elements, hence the same bytes.  sk = (x, y_1 .. y_L).
 * The 2n scalars are made on the device (k_ps_sign_rows), the points are fixed-base products over g's window table.  bad[i] = 1 where either element is the
 * identity (r_i = 0, or x + sum y_j m_ij = 0): the reference returns such a signature and every verifier refuses it.  The device copies of sk, r and the u_i
 * are zeroed on every return path; the host makes no copy of them.
 * dgpu_ps_verify_each is Signature::verify (:95-142): ok[i] = 1 iff neither element is the identity (ZeroSignature) and
 *   e(sigma_1_i, alpha_tilde + sum_j m_ij beta_tilde_j) e(-sigma_2_i, g_tilde) = 1.
 * Per chunk one device pipeline: the rows (1, m_i ..), Q_i by the many-row G2 MSM over pk_g2[0 .. L], the first pair through the fused prepare + line kernel,
 * the second through the lines of the prepared g_tilde, the products of every slice, the loop's tail, the final exponentiation.  An identity Q_i is skipped
 * like every identity in the library: the row then fails on its second pair, as in the reference.
 * dgpu_ps_verify_batch: ONE verdict, rho = random (rho = 0 mod r: DGPU_E_BADARG), w_i = rho^i.  *ok = 1 iff no signature element is the identity and
 *   e(sum_i w_i sigma_1_i, alpha_tilde) prod_j e(sum_i w_i m_ij sigma_1_i, beta_tilde_j) e(-sum_i w_i sigma_2_i, g_tilde) = 1
 * — L + 2 pairs whose G2 sides are fixed: L + 2 MSMs of n terms per chunk (k_ps_col_scalars writes their scalars), the host adds the chunks' points, one
 * multi-pairing, one final exponentiation.  The exponent is a polynomial of degree < n in rho: a batch with a failing row passes with probability at most n / r;
 * rho = 1 lets errors that cancel unweighted pass.
 * dgpu_ps_pok_verify_each is SignaturePoK::verify (proof_system's PoKPSSignature; proof.rs:32-56) for n proofs:
 *   sigs       n x 2 x 12 words: the randomized signature sigma_1', sigma_2'
 *   g2_points  n x 2 x 24 words: k_i (the proof's K) and t_i (the Schnorr commitment)
 *   resp_r     n scalars: the last response, over g_tilde
 *   values, revealed, challenge   as in dgpu_bbs_plus_pok_verify_each_g1: entry j is the revealed message where revealed[i][j] != 0, else the response of the
 *              hidden message j (a dense mask: the reference's index-order and length errors cannot occur)
 *   3  sum_hidden z_ij beta_tilde_j + z_r,i g_tilde - c_i k_i = t_i                                  else the Schnorr error (this protocol's only one)
 *   1  sigma_1' != O and sigma_2' != O                                                               else ZeroSignature
 *   4  e(sigma_1', alpha_tilde + sum_revealed m_ij beta_tilde_j + k_i) e(-sigma_2', g_tilde) = 1     else PairingCheckFailed
 * status[i] = 0 or the number of the first failing check IN THIS ORDER, 3 before 1 before 4: the reference returns proof_res.and(sig_res) (proof.rs:46-55).
 * This is not the order of the BBS calls; 2 is never written.  Per chunk: two rows of L + 2 entries per proof (k_ps_pok_rows), ONE many-row G2 MSM of both,
 * two launches of the GLS mul-add kernel (S_i + (-c_i) k_i; R_i + k_i), the pairing check above, k_ps_verdict.
 *
 * All four: n = 0 is DGPU_OK without touching a device or any pointer (an empty batch verifies); with n > 0 a NULL pointer, row_stride < L, L = 0 (the
 * reference's NoMessages), n or row_stride >= 2^31 is DGPU_E_BADARG before the device is looked at; then DGPU_E_NODEVICE, then the handle.  Points are taken
 * as validated members of the subgroups.  A row count or L + 2 beyond the many-row kernels' reach runs the single-row driver inside the call.  Chunks
 * (UNMEASURED): sign and verify_each min(4096, 2^17 / (L + 1)) rows, the proof call half the rows of min(4096, 2^17 / (L + 2)), the batch
 * min(65536, 2^20 / L); dgpu_set_many_chunk_rows of the development surface cuts all four (the proof call keeps whole pairs of MSM rows: an odd forced count is
 * rounded down, one row up to two).  Stage timers ps.sign_rows, ps.rows, ps.lines, ps.columns,
 * ps.pok_rows, ps.mul_add, ps.pok_verdict beside the BBS+ block's. */
int32_t dgpu_ps_sign_many_g1(uint64_t g_table, size_t L, const uint64_t *sk /* (1+L)*4: x, y_1..y_L */, const uint64_t *messages /* n rows */, size_t row_stride,
                             const uint64_t *r /* n*4 */, size_t n, int32_t montgomery, uint64_t *out_sig /* n*2*12 */, uint8_t *bad /* n */);
int32_t dgpu_ps_verify_each(uint64_t pk_g2, size_t L, const uint64_t *g_tilde_pc, const uint64_t *sigs /* n*2*12 */, const uint64_t *messages /* n rows */,
                            size_t row_stride, size_t n, int32_t montgomery, uint8_t *ok /* n */);
int32_t dgpu_ps_verify_batch(uint64_t pk_g2, size_t L, const uint64_t *all_pc /* (L+2) * DGPU_G2_PREPARED_WORDS */, const uint64_t *sigs /* n*2*12 */,
                             const uint64_t *messages /* n rows */, size_t row_stride, size_t n, int32_t montgomery, const uint64_t random[4], int32_t *ok);
int32_t dgpu_ps_pok_verify_each(uint64_t pk_g2, size_t L, const uint64_t *g_tilde_pc, const uint64_t *sigs /* n*2*12: sigma_1', sigma_2' */,
                                const uint64_t *g2_points /* n*2*24: k_i, t_i */, const uint64_t *resp_r /* n*4 */, const uint64_t *values /* n rows */,
                                size_t row_stride, const uint8_t *revealed /* n*L */, const uint64_t *challenge /* n*4 */, size_t n, int32_t montgomery,
                                uint8_t *status /* n */);

/* ---- the LegoGroth16 prover as one call ----
 * replaces create_proof_and_committed_witnesses_with_assignment (legogroth16/src/prover.rs:267-383, with calculate_coeff :585-594) and — when
 * the circuit is resident (r1cs != 0) — the QAP::witness_map call in front of it (create_proof_with_reduction, :153-180): the whole schedule
 * (one upload of z, witness map, one partition sort shared by the A / B-in-G1 / B-in-G2 / l MSMs when the queries are tables of one shape, the
 * G2 MSM issued first, the O(1) scalar multiplications on a host core meanwhile, the final fold) runs on host threads inside the library.
 *   pk        the proving key: five query handles (dgpu_bases_upload_* / dgpu_window_table_mul_to_bases_*, plain or dgpu_bases_precompute_*d)
 *             on one device, and its O(1) elements on the host in the ABI's affine layout (an all-zero point is the identity)
 *   r1cs      dgpu_r1cs_upload handle of the circuit, or 0 with h_scalars = a resident vector of the D coefficients of h (dgpu_witness_map*)
 *   z         the full assignment (1, instance..., witness...), num_vars scalars; n_inst = number of instance variables incl. the leading 1;
 *             montgomery != 0: &[Fr] limbs.  The first commit_witness_count witnesses are the committed ones (proof.d).
 *   r, s, v   the prover's randomness (canonical limbs, reduced mod r inside)
 *   out       A (G1), B (G2), C (G1), D (G1) as affine points; out_inf[k] = 1 marks an identity (then zero words)
 * Same group elements as the reference computes (asserted limb for limb against the Python mirror and the toxic-waste closed form,
 * tests/test_gpu_prove_abi.py, and from the compiled C++ driver). */
typedef struct dgpu_lego_pk {
    uint64_t a_query, b_g1_query, b_g2_query, h_query, l_query;                                     /* bases handles (query[0] included) */
    const uint64_t *alpha_g1, *beta_g1, *delta_g1, *eta_delta_inv_g1, *eta_gamma_inv_g1;             /* 12 u64 each */
    const uint64_t *beta_g2, *delta_g2;                                                              /* 24 u64 each */
    const uint64_t *a0, *b1_0, *b2_0;                                                                /* query[0] of a / b_g1 (12) / b_g2 (24) */
    const uint64_t *gamma_abc_g1; size_t gamma_abc_len;                                              /* vk.gamma_abc_g1: (n_inst + commit_witness_count) x 12 */
    size_t commit_witness_count;
} dgpu_lego_pk;
int32_t dgpu_legogroth16_prove(const dgpu_lego_pk *pk, uint64_t r1cs, uint64_t h_scalars, const uint64_t *z, size_t num_vars, size_t n_inst,
                               int32_t montgomery, const uint64_t r[4], const uint64_t s[4], const uint64_t v[4],
                               uint64_t out_a[12], uint64_t out_b[24], uint64_t out_c[12], uint64_t out_d[12], uint8_t out_inf[4]);
/* The same prover for a host that holds the proving key the way the reference does — `pk_common: &ProvingKeyCommon<E>` with its queries as `Vec<G1Affine>` /
 * `Vec<G2Affine>` (legogroth16/src/data_structures.rs, prover.rs:267-383) and h as the `&[E::ScalarField]` QAP::witness_map returned (prover.rs:153-180,577-581):
 * every query is a VIEW of host memory (dgpu_msm_*_strided's description of a slice of ark-ec Affine structs; for a_query / b_g1_query / b_g2_query the WHOLE
 * query, element 0 included) which the resident-bases cache above resolves — at a key's second proof the queries are uploaded once and become tables (the a / b / l
 * queries of DGPU_TABLE_C_WITNESS), later proofs run dgpu_legogroth16_prove's schedule on them and only the assignment and h cross PCIe.  A view the cache does not
 * hold (a key's first proof, the cache off or full) is uploaded for the duration of the call.  instance: n_inst scalars (the leading 1 included), witness: n_wit
 * scalars (montgomery != 0: &[Fr]).  Exactly one source of h: r1cs = a resident circuit (dgpu_r1cs_upload; the witness map then runs inside the call and h
 * never leaves the device — create_proof_with_reduction, prover.rs:153-180, as one call) or h = h_len coefficients in host memory (h_montgomery != 0: &[Fr] — the
 * prover's `into_bigint` then happens on the device; create_proof_with_assignment's contract, prover.rs:237-265).  Same proof, limb for limb, as
 * dgpu_legogroth16_prove on uploaded handles (tests/test_gpu_prove_abi.py). */
typedef struct dgpu_bases_view { const void *p; size_t stride, x_off, y_off, inf_off, n; } dgpu_bases_view;
typedef struct dgpu_lego_pk_host {
    dgpu_bases_view a_query, b_g1_query, b_g2_query, h_query, l_query;
    const uint64_t *alpha_g1, *beta_g1, *delta_g1, *eta_delta_inv_g1, *eta_gamma_inv_g1;             /* 12 u64 each */
    const uint64_t *beta_g2, *delta_g2;                                                              /* 24 u64 each */
    const uint64_t *a0, *b1_0, *b2_0;                                                                /* query[0] of a / b_g1 (12) / b_g2 (24) */
    const uint64_t *gamma_abc_g1; size_t gamma_abc_len;
    size_t commit_witness_count;
} dgpu_lego_pk_host;
int32_t dgpu_legogroth16_prove_host(const dgpu_lego_pk_host *pk, uint64_t r1cs, const uint64_t *h, size_t h_len, int32_t h_montgomery,
                                    const uint64_t *instance, size_t n_inst, const uint64_t *witness, size_t n_wit, int32_t montgomery,
                                    const uint64_t r[4], const uint64_t s[4], const uint64_t v[4],
                                    uint64_t out_a[12], uint64_t out_b[24], uint64_t out_c[12], uint64_t out_d[12], uint8_t out_inf[4]);
/* The same call accepts a key that is resident across several device contexts (every query a dgpu_bases_upload_*_sharded handle, optionally
 * dgpu_bases_precompute_*d; the five queries over the same contexts): context g multiplies its rows by the matching slices of z and h from a host
 * thread of its own inside the call, the witness map runs once on the circuit's context (r1cs must be given), the partial points are folded on
 * the host.  Same proof as the single-device call (tests/test_gpu_prove_abi.py, two contexts on one GPU). */
/* ---- the LegoGroth16 verifier as one call (SURVEY.md 8a rows a4 - a7 as the reference uses them together) ----
 * replaces verify_proof (legogroth16/src/verifier.rs:62-99): d = gamma_abc[0] + sum x_j gamma_abc[1 + j] + proof.d (calculate_d, :29-50,:101-109),
 * then e(A, B) e(C, -delta) e(d, -gamma) == e(alpha, beta) (verify_qap_proof, :62-84) with the PreparedVerifyingKey's members (:17-25):
 *   alpha_beta_gt  pvk.alpha_g1_beta_g2 (72 words); delta_neg_pc / gamma_neg_pc: the two G2Prepared values (DGPU_G2_PREPARED_WORDS each,
 *   dgpu_g2_prepare's / arkworks' layout); gamma_abc_g1: vk.gamma_abc_g1, gamma_abc_len x 12 words
 *   proof (a, b, c, d) affine, proof_inf[k] != 0 (or all-zero words) marks an identity; public_inputs: n_pub scalars (montgomery != 0: &[Fr])
 * The host's share (the scalar multiplications of calculate_d) runs while the device computes the chain of the pair (A, B).
 * *ok = 1: the proof verifies, 0: it does not.  DGPU_E_BADARG: n_pub + 1 > gamma_abc_len (MalformedVerifyingKey) or n_pub + 2 >
 * DGPU_MAX_LINCOMB (then: dgpu_msm_g1 + dgpu_multi_miller_loop_mixed + dgpu_final_exponentiation); DGPU_E_ZERO where the reference answers
 * UnexpectedIdentity. */
int32_t dgpu_legogroth16_verify(const uint64_t alpha_beta_gt[72], const uint64_t *delta_neg_pc, const uint64_t *gamma_neg_pc, const uint64_t *gamma_abc_g1, size_t gamma_abc_len,
                                const uint64_t proof_a[12], const uint64_t proof_b[24], const uint64_t proof_c[12], const uint64_t proof_d[12], const uint8_t *proof_inf,
                                const uint64_t *public_inputs, size_t n_pub, int32_t montgomery, int32_t *ok);
/* n proofs of ONE verifying key in one call — the classical Groth16 batch check: what the reference reaches through RandomizedPairingChecker
 * (utils/src/randomized_pairing_check.rs:116-138,204-214: three pairs and one GT power per proof, proof_system/src/verifier.rs hands every statement to one lazy
 * checker) with the pairs that share -delta / -gamma merged BEFORE the pairing: n scalings by the powers of `random`, two variable-base MSMs, ONE Miller
 * loop over n + 2 pairs, one final exponentiation, one GT power (crypto_amd/csrc/dock_aggregation.cpp).  proofs_a / _c / _d: n x 12 words, proofs_b: n x 24
 * (all-zero words: identity); public_inputs: n rows of n_pub scalars; random: the batching scalar (drawn AFTER the proofs are fixed; non-zero mod r, else
 * DGPU_E_BADARG).  *ok = 1 iff every proof verifies (up to the 2^-255 soundness error of the random combination).  n = 0: *ok = 1. */
int32_t dgpu_legogroth16_verify_batch(const uint64_t alpha_beta_gt[72], const uint64_t *delta_neg_pc, const uint64_t *gamma_neg_pc, const uint64_t *gamma_abc_g1, size_t gamma_abc_len,
                                      const uint64_t *proofs_a, const uint64_t *proofs_b, const uint64_t *proofs_c, const uint64_t *proofs_d, size_t n,
                                      const uint64_t *public_inputs, size_t n_pub, int32_t montgomery, const uint64_t random[4], int32_t *ok);
/* n proofs of ONE verifying key, one verdict EACH: verify_proof (legogroth16/src/verifier.rs:62-99) per statement, as the reference's
 * proof_system runs it without a pairing checker (proof_system/src/sub_protocols/r1cs_legogorth16.rs:187, bound_check_legogroth16.rs:205).
 * Arguments as dgpu_legogroth16_verify_batch without `random`; ok[i] = 1: proof i verifies, 0: it does not (a zero Miller output, the
 * reference's UnexpectedIdentity, is a rejection too).  Identities are all-zero words; a pair with an identity member is skipped per proof as in
 * dgpu_legogroth16_verify.  Any n_pub (no DGPU_MAX_LINCOMB limit); DGPU_E_BADARG: n_pub + 1 > gamma_abc_len or a NULL pointer.  n = 0: DGPU_OK.
 * Everything runs on the device: d_i through dgpu_g1_mul_add_batch, one segmented Miller loop with the key's two prepared points shared by every
 * proof, the tails, final exponentiations and comparisons with alpha_beta_gt in k_gt.hip; only the verdicts come back.  Chunks of 4096 proofs
 * (~0.5 GB of device memory). */
int32_t dgpu_legogroth16_verify_each(const uint64_t alpha_beta_gt[72], const uint64_t *delta_neg_pc, const uint64_t *gamma_neg_pc, const uint64_t *gamma_abc_g1, size_t gamma_abc_len,
                                     const uint64_t *proofs_a, const uint64_t *proofs_b, const uint64_t *proofs_c, const uint64_t *proofs_d, size_t n,
                                     const uint64_t *public_inputs, size_t n_pub, int32_t montgomery, uint8_t *ok /* n */);
/* ---- SnarkPack aggregation of Groth16 / LegoGroth16 proofs (crypto_amd/csrc/dock_aggregation.cpp) ----
 * replaces aggregate_proofs (legogroth16/src/aggregation/groth16/prover.rs:47-147; legogroth16/prover.rs:38-127 when `d` is given) and
 * verify_aggregate_proof (groth16/verifier.rs:36-100, legogroth16/verifier.rs:34-96, legogroth16/using_groth16.rs:45-128) as the reference
 * calls them; the group, pairing and GT work goes through the entry points above from host threads inside the call.
 * The Fiat-Shamir transcript is the caller's (`&mut impl Transcript`, utils/src/transcript.rs:45-63): append_message receives the label and the
 * bytes `Transcript::append` would serialize (`serialize_compressed`: 48 / 96-byte Zcash points, 32 / 48-byte little-endian canonical field
 * elements, a PairCommitment as t then u), challenge_scalar returns the transcript's `challenge_scalar::<Fr>(label)` as 4 canonical words.
 * Points are affine ABI words (identity: all-zero words).  The aggregate proof is a flat array of 64-bit words,
 *   nproofs, n_mipp | com_ab(t, u) com_c [com_d] | z_ab z_c [z_d] | comms_ab[L](l.t l.u r.t r.u) comms_c[L] [comms_d[L]] | z_ab[L](l r) z_c[L] [z_d[L]]
 *   | final_a final_b final_c [final_d] final_vkey(2) final_wkey(2) | vkey_opening(2) wkey_opening(2)          (L = log2 nproofs; GT 72, G1 12, G2 24 words)
 * i.e. the fields of AggregateProof / GipaProof / TippMippProof in their declaration order (groth16/proof.rs:12-24,76-84,117-121). */
#define DGPU_SNARKPACK_MAX_SRS_SIZE (((size_t)2 << 19) + 1)          /* srs.rs MAX_SRS_SIZE */
#define DGPU_SNARKPACK_VALIDATE_POINTS 2                             /* verify flag: every G1 / G2 element of the proof (and of d_list) must be on its curve and in the prime-order subgroup (the other half of Validate::Yes) */
#define DGPU_SNARKPACK_VALIDATE_GT 1                                 /* verify flag: every GT element of the proof must have order r (Validate::Yes on a deserialised proof) */
typedef struct dgpu_transcript {
    void *ctx;
    void (*append_message)(void *ctx, const uint8_t *label, size_t label_len, const uint8_t *bytes, size_t len);
    void (*challenge_scalar)(void *ctx, const uint8_t *label, size_t label_len, uint64_t out[4]);
} dgpu_transcript;
typedef struct dgpu_snarkpack_prover_srs {                           /* ProverSRS specialised to n proofs (srs.rs:60-93,180-237) */
    size_t n;
    const uint64_t *g_alpha_powers_table, *g_beta_powers_table;      /* 2n x 12 */
    const uint64_t *h_alpha_powers_table, *h_beta_powers_table;      /* n x 24 */
    const uint64_t *vkey_a, *vkey_b;                                 /* n x 24 (h^{alpha^i}, h^{beta^i}) */
    const uint64_t *wkey_a, *wkey_b;                                 /* n x 12 (g^{alpha^{n+i}}, g^{beta^{n+i}}) */
} dgpu_snarkpack_prover_srs;
typedef struct dgpu_snarkpack_verifier_srs { size_t n; const uint64_t *g, *h, *g_alpha, *g_beta, *h_alpha, *h_beta; } dgpu_snarkpack_verifier_srs;   /* srs.rs:95-110 */
typedef struct dgpu_groth16_vk { const uint64_t *alpha_g1, *beta_g2, *gamma_g2, *delta_g2, *gamma_abc_g1; size_t gamma_abc_len; } dgpu_groth16_vk;
/* words of an aggregate proof of n proofs (0: n is not a power of two in [2, MAX_SRS_SIZE]) */
size_t dgpu_snarkpack_proof_words(size_t n, int32_t with_d);
/* a, c (, d): n x 12; b: n x 24; d = NULL: Groth16 proofs.  *len_words is set to the proof's length even when cap_words is too small
 * (DGPU_E_LENGTH).  DGPU_E_BADARG: n < 2, not a power of two, or srs->n != n. */
int32_t dgpu_snarkpack_aggregate(const dgpu_snarkpack_prover_srs *srs, const uint64_t *a, const uint64_t *b, const uint64_t *c, const uint64_t *d,
                                 size_t n, const dgpu_transcript *transcript, uint64_t *proof, size_t cap_words, size_t *len_words);
/* variant 0: Groth16 proofs; 1: LegoGroth16 (the proof carries the MIPP for d); 2: LegoGroth16 proofs under the Groth16 aggregator, d_list = the
 * n commitments d (using_groth16.rs).  public_inputs: n_rows x inputs_per_proof canonical scalars (n_rows must equal nproofs); random: the
 * pairing checker's batching scalar (RandomizedPairingChecker::new_using_rng draws it; must be non-zero mod r — a zero would scale every equation after
 * the first out of the check: DGPU_E_BADARG).  flags: DGPU_SNARKPACK_VALIDATE_GT | DGPU_SNARKPACK_VALIDATE_POINTS for a proof from an untrusted source (what
 * CanonicalDeserialize with Validate::Yes checks before the reference ever sees an AggregateProof).  *ok = 1: the aggregate verifies, 0: it does not (a failed
 * pairing / final_z check, a GT / G1 / G2 element outside its subgroup under the validation flags).  DGPU_E_BADARG: a malformed proof (parsing_check), a key that does not match
 * the public inputs (MalformedVerifyingKey), a row count that is not nproofs. */
int32_t dgpu_snarkpack_verify(const dgpu_snarkpack_verifier_srs *srs, const dgpu_groth16_vk *vk, const uint64_t *public_inputs, size_t n_rows, size_t inputs_per_proof,
                              const uint64_t *proof, size_t len_words, int32_t variant, const uint64_t *d_list, const uint64_t random[4],
                              const dgpu_transcript *transcript, int32_t flags, int32_t *ok);
/* elements behind a bases / scalars / sorted handle; constraints of a resident circuit */
int32_t dgpu_handle_len(uint64_t handle, size_t *n);
int32_t dgpu_handle_context(uint64_t handle, int32_t *context);
/* layout of a sharded handle: number of parts (0: not sharded); part k holds elements [lo, hi) as a handle of its own on `context` */
int32_t dgpu_shard_count(uint64_t handle, int32_t *count);
int32_t dgpu_shard_part(uint64_t handle, size_t k, uint64_t *sub_handle, size_t *lo, size_t *hi, int32_t *context);

/* ---- canonical (de)serialisation of group elements (host code) ----
 * The format ark-bls12-381 0.4 emits for `CanonicalSerialize` (Zcash / IETF BLS12-381): big-endian coordinates, top three bits of
 * byte 0 = compressed / infinity / y-lexicographically-largest; G1 48 B (compressed) or 96 B, G2 96 or 192 B with c1 before c0.
 * Used to load keys and proofs written by the Rust side (legogroth16/src/data_structures.rs:7-186) into the ABI layout.
 * `mode` of the deserialisers: bit 0 = compressed; DGPU_SERDE_NO_VALIDATE = arkworks' Validate::No (skip the subgroup test).
 * DGPU_E_BADARG: wrong compression flag, coordinate >= p, not on the curve, a non-canonical infinity encoding, or — Validate::Yes,
 * the default, what `deserialize_compressed` does — a point outside the prime-order subgroup ([r]P != O). */
#define DGPU_SERDE_NO_VALIDATE 2
int32_t dgpu_g1_serialize(const uint64_t *xy /* n*12 */, const uint8_t *is_inf, size_t n, int32_t compressed, uint8_t *out);
int32_t dgpu_g1_deserialize(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy /* n*12 */, uint8_t *is_inf /* n */);
int32_t dgpu_g2_serialize(const uint64_t *xy /* n*24 */, const uint8_t *is_inf, size_t n, int32_t compressed, uint8_t *out);
int32_t dgpu_g2_deserialize(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy /* n*24 */, uint8_t *is_inf /* n */);

/* ---- the same decoding and validation on the device (one point per lane; the calling thread's context, dgpu_set_device) ----
 * dgpu_g1/g2_deserialize_device: the mode bits, verdict and (when accepted) words and flags of dgpu_g1/g2_deserialize.  first_bad (may be NULL):
 * n on success, else the LOWEST refused index (DGPU_E_BADARG).  Outputs are unspecified on refusal.  n = 0: DGPU_OK.
 * dgpu_bases_upload_g1/g2_serialized: bytes -> a resident plain bases handle, what dgpu_bases_upload_* makes of the decoded points (MSMs, precompute,
 * dgpu_handle_len as for those); xy / is_inf (may be NULL): the decoded words too.  On refusal or error no handle exists and no device memory is kept.
 * dgpu_g1/g2_validate_batch: Validate::Yes of affine ABI words already in memory: ok[i] = 1 iff point i is the identity (is_inf[i] or all-zero
 * words) or reduced (< p), on the curve and in G1 / G2 — the checks an aggregate proof's points get on the host (g1_words_valid / g2_words_valid).
 * Argument checks come first (DGPU_E_BADARG); without a device n >= 1 is DGPU_E_NODEVICE, never a host result. */
int32_t dgpu_g1_deserialize_device(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy /* n*12 */, uint8_t *is_inf /* n */, size_t *first_bad);
int32_t dgpu_g2_deserialize_device(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy /* n*24 */, uint8_t *is_inf /* n */, size_t *first_bad);
int32_t dgpu_bases_upload_g1_serialized(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy, uint8_t *is_inf, uint64_t *handle, size_t *first_bad);
int32_t dgpu_bases_upload_g2_serialized(const uint8_t *in, size_t n, int32_t mode, uint64_t *xy, uint8_t *is_inf, uint64_t *handle, size_t *first_bad);
int32_t dgpu_g1_validate_batch(const uint64_t *xy /* n*12 */, const uint8_t *is_inf, size_t n, uint8_t *ok /* n */);
int32_t dgpu_g2_validate_batch(const uint64_t *xy /* n*24 */, const uint8_t *is_inf, size_t n, uint8_t *ok /* n */);

/* ---- the encoding on the device, and resident bases read back (one point per lane) ----
 * dgpu_g1/g2_serialize_device: the contract and the bytes of dgpu_g1/g2_serialize, on the calling thread's context (dgpu_set_device).  Argument checks
 * come first (DGPU_E_BADARG); without a device n >= 1 is DGPU_E_NODEVICE, never a host result.  n = 0: DGPU_OK.
 * dgpu_bases_read_g1/g2: the affine ABI words (xy, may be NULL) and identity flags (is_inf, may be NULL; not both) of points [offset, offset + n) of
 * a G1 / G2 bases handle: a plain one (dgpu_bases_upload_*, *_serialized, *_strided, dgpu_window_table_mul_to_bases_*, the queries of
 * dgpu_legogroth16_setup), its precomputed table (dgpu_bases_precompute_*) or a sharded set (dgpu_bases_upload_*_sharded: every part is read on its
 * own context, the results land in global index order).  An identity comes back as zero words with is_inf = 1.
 * dgpu_bases_serialize_g1/g2: the same points as the bytes dgpu_g1/g2_serialize writes for them (compressed: 48 / 96 B per point, else 96 / 192 B):
 * the inverse of dgpu_bases_upload_g1/g2_serialized.
 * The handle calls run on the context that owns the handle and pin it for the call (a racing dgpu_bases_free waits).  DGPU_E_BADARG: an unknown or
 * freed handle, another kind (window table, scalars, circuit, ...), the other curve's handle, offset + n > its length, NULL out / both xy and is_inf
 * NULL (n >= 1).  n = 0 on a valid handle: DGPU_OK.  A refused or failing call keeps no device memory of its own.  The results leave in pieces of
 * STAGE_CHUNK_BYTES, each copied to the host while the next one encodes (stage timer serde.encode). */
int32_t dgpu_g1_serialize_device(const uint64_t *xy /* n*12 */, const uint8_t *is_inf, size_t n, int32_t compressed, uint8_t *out);
int32_t dgpu_g2_serialize_device(const uint64_t *xy /* n*24 */, const uint8_t *is_inf, size_t n, int32_t compressed, uint8_t *out);
int32_t dgpu_bases_read_g1(uint64_t handle, size_t offset, size_t n, uint64_t *xy /* n*12 or NULL */, uint8_t *is_inf /* n or NULL */);
int32_t dgpu_bases_read_g2(uint64_t handle, size_t offset, size_t n, uint64_t *xy /* n*24 or NULL */, uint8_t *is_inf /* n or NULL */);
int32_t dgpu_bases_serialize_g1(uint64_t handle, size_t offset, size_t n, int32_t compressed, uint8_t *out);
int32_t dgpu_bases_serialize_g2(uint64_t handle, size_t offset, size_t n, int32_t compressed, uint8_t *out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
