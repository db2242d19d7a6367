// crypto_amd/csrc/wm_block_args.hip.h — arguments of the block witness map (wm_block_kernels.hip.h), shared by the kernel, its launcher
// (qap_launch.hip.h) and the driver (dock_qap.hip).  Plain structs: no HIP types.
#pragma once
#include <stddef.h>
#include <stdint.h>
namespace ntt {
constexpr int WM_BLOCK_MAX_LOG = 10;        // the largest domain a block holds: three arrays of 2^10 elements = 120 KB of the CU's 160 KB of LDS
constexpr int WM_BLOCK_THREADS = 768;       // at most: one radix-4 unit per lane over the three arrays of a full tile
// the resident circuit: CSR per matrix, values limb-major with stride nnz[k]
struct WmCircuit { const uint64_t *rowptr[3]; const uint32_t *cols[3]; const uint32_t *vals[3]; size_t nnz[3]; size_t rows, extra; };
// the cached tables of the domain (NttDomain): twiddles with their per-stage tables, coset factors in the order of bit-reversed data, 1 / Z(g) as words
struct WmTables { const uint32_t *tw_f, *tw_i, *pwr_f, *pwr_i, *zinv; };
// one launch: statement j reads its num_vars scalars at z_words + j * row_words (8 words per scalar) and writes its D scalars at out_words + j * D * 8
struct WmJob { const uint32_t *z_words; size_t row_words; int z_mont; uint32_t nrows; uint32_t *out_words; int out_mont; int logn; uint32_t rows_per_block; };
// statements per block when the caller has no wish: domains of up to 128 elements share a block, so that a block is never a single wave's worth of
// work (256 elements: 192 radix-4 units over the three arrays)
inline uint32_t wm_rows_per_block(int logn) { return logn >= 8 ? 1u : (256u >> logn); }
inline uint32_t wm_max_rows_per_block(int logn) { return 1u << (WM_BLOCK_MAX_LOG - logn); }
}  // namespace ntt
