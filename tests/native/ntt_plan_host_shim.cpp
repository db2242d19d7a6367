// tests/native/ntt_plan_host_shim.cpp — the pass planners of the Fr NTT (crypto_amd/csrc/ntt_plan.hpp: what run_passes of k_ntt.hip calls to cut a transform
// into launches) behind a C interface.  The header is plain host arithmetic; tests/test_ntt_plan_host.py builds this file with g++ alone.
#include "../../crypto_amd/csrc/ntt_plan.hpp"

extern "C" {
// groups in launch order into out[0 .. cap); returns the group count (also when it exceeds cap: nothing is written past cap)
int shim_plan_piped(int logn, int dif, int *out, int cap) {
    int g[32] = {0};      // (no schedule has more groups than stages: a planner that outgrows the caller's array fails the test, not the stack)
    const int n = ntt::plan_piped(logn, dif, g);
    for (int k = 0; k < n && k < cap; k++) out[k] = g[k];
    return n;
}
int shim_plan_staged(int logn, int dif, int *out, int cap) {
    int g[32] = {0};
    const int n = ntt::plan_staged(logn, dif, g);
    for (int k = 0; k < n && k < cap; k++) out[k] = g[k];
    return n;
}
// what the planners and their callers are sized for: {piped tile log, piped max logn, piped array, staged tile log, staged max stages, staged max logn, staged array}
void shim_plan_limits(int out[7]) {
    out[0] = ntt::PLAN_PIPE_TILE_LOG; out[1] = ntt::PLAN_PIPE_MAX_LOGN; out[2] = ntt::PLAN_PIPE_MAX_GROUPS;
    out[3] = ntt::PLAN_FUSE_TILE_LOG; out[4] = ntt::PLAN_FUSE_MAX_STAGES; out[5] = ntt::PLAN_FUSE_MAX_LOGN; out[6] = ntt::PLAN_FUSE_MAX_GROUPS;
}
}
