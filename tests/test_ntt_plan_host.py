"""CPU: the pass planners of the Fr NTT (crypto_amd/csrc/ntt_plan.hpp plan_piped / plan_staged, what run_passes of k_ntt.hip calls), compiled for the host
by g++ alone (tests/native/ntt_plan_host_shim.cpp) and checked for every log2 D each route can receive, both directions: the stage counts sum to log2 D,
every group fits its kernel's tile, exactly one group has L = 0 and sits where the kernels expect it, every other staged group meets the precondition
k_ntt_fused states (L >= 11 - S), the group count fits the fixed arrays of run_passes, and the decimation-in-time schedule is the decimation-in-frequency
one reversed.  The production schedules tests/test_gpu_ntt_paths.py imitates at small sizes (2^27, 2^28 staged; 2^23 .. 2^26 piped with three strided
passes) and the merge of a short staged group are pinned as literal values.  The development knob's host contract (dgpu_dev_set_ntt) is checked on the twin."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(HERE, "..", "crypto_amd", "csrc", "ntt_plan.hpp")
SRC = os.path.join(HERE, "native", "ntt_plan_host_shim.cpp")
SO = os.path.join(HERE, "native", "libntt_plan_host_shim.so")
OK, BADARG = 0, -3


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in (SRC, HDR)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", SO, SRC])
    L = C.CDLL(SO)
    for f in (L.shim_plan_piped, L.shim_plan_staged):
        f.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
        f.restype = C.c_int
    L.shim_plan_limits.argtypes = [C.POINTER(C.c_int)]
    L.shim_plan_limits.restype = None
    return L


def plan(fn, logn, dif):
    out = (C.c_int * 32)()
    n = fn(logn, dif, out, 32)
    assert 0 < n <= 32
    return list(out[:n])


def limits(shim):
    lim = (C.c_int * 7)()
    shim.shim_plan_limits(lim)
    return dict(zip(("pipe_tile", "pipe_max", "pipe_cap", "fuse_tile", "fuse_stages", "fuse_max", "fuse_cap"), lim))


def column_bits(groups, logn, dif):
    """L of every group as the kernels compute it: logn - s0 - S for decimation in frequency, s0 for decimation in time"""
    out, s0 = [], 0
    for S in groups:
        out.append(logn - s0 - S if dif else s0)
        s0 += S
    return out


def test_the_limits_the_planners_are_built_for(shim):
    assert limits(shim) == dict(pipe_tile=10, pipe_max=26, pipe_cap=12, fuse_tile=11, fuse_stages=7, fuse_max=28, fuse_cap=8)


@pytest.mark.parametrize("dif", [1, 0])
def test_piped_schedules(shim, dif):
    lim = limits(shim)
    for logn in range(lim["pipe_tile"], lim["pipe_max"] + 1):
        g = plan(shim.shim_plan_piped, logn, dif)
        assert sum(g) == logn, (logn, g)
        assert all(1 <= S <= lim["pipe_tile"] for S in g), (logn, g)
        assert len(g) <= lim["pipe_cap"], (logn, g)
        L = column_bits(g, logn, dif)
        assert L.count(0) == 1 and L[-1 if dif else 0] == 0, (logn, g, L)
        # what include/dock_gpu_dev.h says of the automatic choice: a flat pass of at least 6 stages, strided passes of 5 or 6 (32 or 16 columns per tile)
        flat = g[-1 if dif else 0]
        strided = g[:-1] if dif else g[1:]
        assert flat >= 6 and all(S in (5, 6) for S in strided), (logn, g)
        assert plan(shim.shim_plan_piped, logn, 1 - dif) == g[::-1]


@pytest.mark.parametrize("dif", [1, 0])
def test_staged_schedules(shim, dif):
    lim = limits(shim)
    for logn in range(lim["fuse_tile"], lim["fuse_max"] + 1):
        g = plan(shim.shim_plan_staged, logn, dif)
        assert sum(g) == logn, (logn, g)
        assert all(1 <= S <= lim["fuse_stages"] for S in g), (logn, g)
        assert len(g) <= lim["fuse_cap"], (logn, g)
        L = column_bits(g, logn, dif)
        assert L.count(0) == 1 and L[-1 if dif else 0] == 0, (logn, g, L)
        for S, l in zip(g, L):
            assert l == 0 or l >= lim["fuse_tile"] - S, "log2 D = %d: the group of %d stages has 0 < L = %d < log2(columns)" % (logn, S, l)
        assert plan(shim.shim_plan_staged, logn, 1 - dif) == g[::-1]


def test_the_staged_route_cannot_start_below_one_tile(shim):
    """2^10 staged would be [5, 5]: the first group's columns are 5 bits apart, its tile 64 columns wide — why dgpu_dev_set_ntt's path 2 leaves domains below
    2^11 on the automatic route (and a tile of 2^11 elements does not exist there)"""
    g = plan(shim.shim_plan_staged, 10, 1)
    assert g == [5, 5] and column_bits(g, 10, 1)[0] < 11 - g[0]


PRODUCTION = [(27, "staged", [6, 7, 7, 7]), (28, "staged", [7, 7, 7, 7]),
              (23, "piped", [5, 5, 5, 8]), (24, "piped", [5, 5, 5, 9]), (25, "piped", [5, 5, 5, 10]), (26, "piped", [6, 5, 5, 10]),
              # the staged sizes the GPU tests run: production group sizes and L (13, 14), the three-group prefixes (20, 21), the merge rule (15, 16, 17), the smallest tiles
              (11, "staged", [4, 7]), (12, "staged", [5, 7]), (13, "staged", [6, 7]), (14, "staged", [7, 7]),
              (15, "staged", [4, 4, 7]), (16, "staged", [4, 5, 7]), (17, "staged", [5, 5, 7]), (20, "staged", [6, 7, 7]), (21, "staged", [7, 7, 7]),
              (13, "piped", [5, 8])]


@pytest.mark.parametrize("logn,route,dif_groups", PRODUCTION)
def test_pinned_schedules(shim, logn, route, dif_groups):
    fn = shim.shim_plan_staged if route == "staged" else shim.shim_plan_piped
    assert plan(fn, logn, 1) == dif_groups
    assert plan(fn, logn, 0) == dif_groups[::-1]


def test_the_knob_lives_in_the_twin_and_refuses_what_it_cannot_mean():
    from crypto_amd._native import lib, dev_lib
    T = dev_lib()
    for name in ("dgpu_dev_set_ntt", "dgpu_dev_get_ntt_last"):
        assert hasattr(T, name) and not hasattr(lib(), name)
    arr = lambda v: np.array(v, dtype=np.int32)
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)
    good = arr([5, 5, 5, 1])
    try:
        assert T.dgpu_dev_set_ntt(0, p_(good), 4) == OK
        for path, split, n in ((0, arr([5, 0, 5]), 3), (0, arr([5, 11]), 2), (0, arr([1] * 13), 13), (-1, None, 0), (3, None, 0), (0, None, 2), (0, good, -1)):
            assert T.dgpu_dev_set_ntt(path, None if split is None else p_(split), n) == BADARG, (path, split, n)
        assert T.dgpu_dev_set_ntt(2, None, 0) == OK and T.dgpu_dev_set_ntt(1, p_(arr([10] * 12)), 12) == OK
        route = C.c_int32(-7)
        assert T.dgpu_dev_get_ntt_last(None, None, 0) == BADARG and T.dgpu_dev_get_ntt_last(C.byref(route), None, 4) == BADARG
        assert T.dgpu_dev_get_ntt_last(C.byref(route), None, 0) >= 0 and route.value in (0, 1, 2)
    finally:
        assert T.dgpu_dev_set_ntt(0, None, 0) == OK
