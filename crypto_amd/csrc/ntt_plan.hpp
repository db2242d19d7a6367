// crypto_amd/csrc/ntt_plan.hpp — how run_passes (k_ntt.hip) cuts the log2 D stages of a transform into launches: pure host arithmetic, no HIP, so that
// tests/native/ntt_plan_host_shim.cpp can compile it with g++ and tests/test_ntt_plan_host.py can check every domain size without a device.
// Groups are in LAUNCH order.  Group k runs stages s0 .. s0 + S - 1 (s0 = sum of the groups before it) over tiles whose columns are L bits apart:
// L = logn - s0 - S for decimation in frequency, L = s0 for decimation in time — so exactly one group has L = 0 (a tile is one contiguous
// run): the last one for DIF, the first one for DIT, and the DIT schedule is the DIF schedule reversed.
#pragma once
namespace ntt {
constexpr int PLAN_PIPE_TILE_LOG = 10;      // k_ntt_r4: 2^10-element tiles (PIPE_TILE_LOG), domains 2^10 .. 2^26
constexpr int PLAN_PIPE_MAX_LOGN = 26;
constexpr int PLAN_PIPE_MAX_GROUPS = 12;
constexpr int PLAN_FUSE_TILE_LOG = 11;      // k_ntt_fused: 2^11-element tiles (FUSE_TILE_LOG), groups of up to 7 stages, domains 2^11 .. 2^28
constexpr int PLAN_FUSE_MAX_STAGES = 7;
constexpr int PLAN_FUSE_MAX_LOGN = 28;
constexpr int PLAN_FUSE_MAX_GROUPS = 8;

// Pipelined passes (k_ntt_r4), logn in 10 .. 26.  One pass is "flat" (L = 0, up to TILE_LOG stages), the others are strided and a tile
// holds 2^(TILE_LOG - S) consecutive columns: S = TILE_LOG - 5 keeps every access a full 128-byte line (32 columns), one more stage halves it.
inline int plan_piped(int logn, int dif, int groups[PLAN_PIPE_MAX_GROUPS]) {
    constexpr int tile_log = PLAN_PIPE_TILE_LOG;
    const int pref = tile_log - 5, maxs = tile_log - 4;
    const int over = logn > tile_log ? logn - tile_log : 0;
    const int n_str = (over + maxs - 1) / maxs;
    int flat = logn - pref * n_str;
    if (flat > tile_log) flat = tile_log;
    if (flat < 1) flat = 1;
    int strided[PLAN_PIPE_MAX_GROUPS], rest = logn - flat, ng = 0;
    for (int k = 0; k < n_str; k++) { strided[k] = rest / (n_str - k); rest -= strided[k]; }
    if (dif) { for (int k = n_str - 1; k >= 0; k--) groups[ng++] = strided[k]; groups[ng++] = flat; }
    else { groups[ng++] = flat; for (int k = 0; k < n_str; k++) groups[ng++] = strided[k]; }
    return ng;
}

// Staged passes (k_ntt_fused), logn in 11 .. 28: groups of up to 7 stages; the short group goes where its L is largest (first for DIF, last
// for DIT).  k_ntt_fused wants L = 0 or L >= log2(columns) = 11 - S: a short group of S < 4 stages next to the L = 0 group would break that, so
// it is merged with its neighbour by splitting 7 + S evenly.
inline int plan_staged(int logn, int dif, int groups[PLAN_FUSE_MAX_GROUPS]) {
    constexpr int SMAX = PLAN_FUSE_MAX_STAGES;
    int ng = 0; const int rest = logn % SMAX;
    if (dif) { if (rest) groups[ng++] = rest; for (int k = 0; k < logn / SMAX; k++) groups[ng++] = SMAX; }
    else { for (int k = 0; k < logn / SMAX; k++) groups[ng++] = SMAX; if (rest) groups[ng++] = rest; }
    if (ng >= 2) {
        int &shortg = dif ? groups[0] : groups[ng - 1]; int &nb = dif ? groups[1] : groups[ng - 2];
        if (shortg < 4) { int tot = shortg + nb; shortg = tot / 2; nb = tot - shortg; }
    }
    return ng;
}
}  // namespace ntt
