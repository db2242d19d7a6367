"""CPU: the host side of the MSM sort stage's checks (tests/test_gpu_sort_stage.py has the device side).
  * the chunk rule: util.dyn_chunk_model, written from the description of choose_chunk in unbounded integers, against the host's copy itself
    (dgpu_selftest_choose_chunk of the development twin) at and around every branch, for G1's and G2's parameters;
  * the two rules of launch_psort that crypto_amd/csrc/sort_launch.hip.h now holds as inline functions — ps_use_wc at its border, ps_scatter_lds_bytes against
    the limit the scatter is launched under — and plain_geometry's condition on the latter (a forced width of 22 must take the sweeps);
  * every input of the GPU cases reaches the branch it is named after: the builders of tests/sort_stage_cases.py assert that themselves, here they run without
    a GPU;
  * the model and check_sort: check_sort accepts the model's own output in any order inside a bucket and refuses each kind of damage it is there to find."""
import ctypes as C
import numpy as np
import pytest
import util as U
import sort_stage_cases as SC
from crypto_amd._native import lib, dev_lib, DEV_SYMBOLS
from test_digit_codes_device_code_on_host import shim  # noqa: F401  (the host build of sort_launch.hip.h's inline functions)

HOOKS = ["dgpu_selftest_psort", "dgpu_selftest_sort_sweep", "dgpu_selftest_scan", "dgpu_selftest_dyn_chunk", "dgpu_selftest_choose_chunk"]


def test_hooks_live_in_the_twin_only():
    L, T = lib(), dev_lib()
    for name in HOOKS:
        assert name in DEV_SYMBOLS and hasattr(T, name) and not hasattr(L, name), name
    z = np.zeros(8, np.uint32)
    p = z.ctypes.data_as(C.c_void_p)
    # arguments are checked before a device is looked for
    assert T.dgpu_selftest_psort(p, 1, 15, 18, 0, 0, 0, None, 0, 0, 0, None, 0, p, p, p, None, p, C.byref(C.c_int32())) == -3        # W > 16
    assert T.dgpu_selftest_psort(p, 1, 22, 12, 1 << 21, 0, 0, None, 0, 0, 0, None, 0, p, p, p, None, p, C.byref(C.c_int32())) == -3  # the scatter's LDS does not fit
    assert T.dgpu_selftest_psort(p, 1, 16, 16, 5, 0, 0, None, 0, 0, 0, None, 0, p, p, p, None, p, C.byref(C.c_int32())) == -3        # key_wstride is 0 or B
    assert T.dgpu_selftest_psort(p, 1, 16, 16, 0, 0, 0, None, 0, 0, 0, None, 3, p, p, p, None, p, C.byref(C.c_int32())) == -3        # place is 0, 1 or 2
    assert T.dgpu_selftest_sort_sweep(p, 1, 6, 0, None, 0, 0, p, p, p, p, p, p) == -3
    assert T.dgpu_selftest_scan(p, 0, 0, p, None) == -3 and T.dgpu_selftest_scan(p, 1, 1, p, None) == -3
    assert T.dgpu_selftest_dyn_chunk(5, 0, 0, 1, 1, 0, 0, p) == -3 and T.dgpu_selftest_dyn_chunk(5, 0, 16, 1, 0, 0, 0, p) == -3
    assert T.dgpu_selftest_choose_chunk(5, 0, 1, 1, 0) == -3 and T.dgpu_selftest_choose_chunk(5, 16, 1, 0, 0) == -3


@pytest.mark.parametrize("rule", [SC.G1_RULE, SC.G2_RULE], ids=["G1", "G2"])
def test_chunk_rule_model_equals_the_host_copy(rule):
    """choose_chunk (dock_core.hip) == dyn_chunk_model wherever the host's rule applies (no forced length, no cap), and the table reaches every branch"""
    T = dev_lib()
    assert T.dgpu_set_chunk(0) == 0
    seen = set()
    m, mc, lanes = rule["min_chunk"], rule["max_chunks"], rule["lanes_per_chunk"]
    rows = SC.chunk_rule_table(rule)
    for E, fixed, T_max, nb in rows:
        want = U.dyn_chunk_model(E, fixed, m, mc, lanes, T_max, nb, seen)
        assert want[1] == -(-E // want[0]) and want[2] == 16 * want[0] < 1 << 32 and (not T_max or want[1] <= T_max), (E, fixed, T_max, nb, want)
        if not fixed and not T_max:
            assert T.dgpu_selftest_choose_chunk(E, m, mc, lanes, nb) == want[0], (E, nb, want)
    if lanes == 1:
        assert seen == set(SC.CHUNK_BRANCHES), set(SC.CHUNK_BRANCHES) ^ seen
    else:                                                   # G2's shortest chunk is 32: its rounds are never shorter than 16
        assert seen == set(SC.CHUNK_BRANCHES) - {"len below 16"}, set(SC.CHUNK_BRANCHES) ^ seen
    # a forced length is the host's answer as well
    assert T.dgpu_set_chunk(19) == 0
    try:
        assert T.dgpu_selftest_choose_chunk(10 ** 7, m, mc, lanes, 0) == 19
    finally:
        assert T.dgpu_set_chunk(0) == 0


def test_chunk_rule_named_points():
    """the branch points of the table, spelled out for G1 (131072 resident chunks, 300000 chunks before the length doubles)"""
    f = lambda E, nb=0, T=0: U.dyn_chunk_model(E, 0, 16, 300000, 1, T, nb)[:2]
    r = 131072
    assert f(0) == (16, 0) and f(1) == (16, 1)
    assert f(300000 * 16 + 15)[0] == 19 and f(300000 * 16 + 16)[0] == 37          # 300000 chunks of 16 snap to two rounds; one chunk more doubles to 32 first: one round
    assert f(r * 16) == (16, r) and f(r * 16 + 1) == (17, 123362)                 # a full round stays; one term more is one round of 17 (the last lanes idle)
    assert f(16 * (3 * r // 2) - 16)[0] == 24 and f(16 * (3 * r // 2))[0] == 16   # 1.5 rounds less a chunk: one round of 24; 1.5 rounds: two of 12, refused (below 16)
    assert f(32 * r) == (16, 2 * r) and f(32 * r + 1)[0] == 17
    assert f(4096 * 3 * r) == (4096, 3 * r) and f(4096 * 3 * r + 1) == (4096, 3 * r + 1)
    assert f(48 * r, 2 * r)[0] == 48 and f(48 * r - 1, 2 * r)[0] == 24 and f(48 * r, 0)[0] == 24
    assert f(4096 * r, 1 << 15)[0] == 4096 and f(4096 * r + 1, 1 << 15)[0] == 2049
    assert f((1 << 32) - 1) == (4096, 1 << 20) and f((1 << 32) - 4096) == (4096, (1 << 20) - 1)
    assert f(10 ** 6, 0, 1000) == (1000, 1000) and f(10 ** 6, 0, 62500) == (16, 62500) and f(10 ** 6 + 1, 0, 62500) == (17, 58824)


def test_write_combining_rule_at_its_border(shim):  # noqa: F811
    shim.shim_ps_use_wc.argtypes = [C.c_size_t, C.c_int, C.c_uint32]
    wc = lambda n, W, P: shim.shim_ps_use_wc(n, W, P)
    assert SC.PS_WC_MIN_PAIRS == 65536
    assert wc((1 << 22) - 1, 16, 1024) == 0 and wc(1 << 22, 16, 1024) == 1
    n13 = -(-65536 * 1024 // 13)                            # the first n with n * 13 // 1024 >= 65536
    assert (n13 * 13) // 1024 == 65536 and ((n13 - 1) * 13) // 1024 == 65535
    assert wc(n13 - 1, 13, 1024) == 0 and wc(n13, 13, 1024) == 1
    assert wc(1 << 31, 16, 1024) == 1                       # (the product is taken in 64 bits)
    for case in (1539, 4173, 8192, 41600, 16500):
        assert wc(case, 16, 1024) == 0                      # every GPU case reports the direct form under the product's rule


def test_scatter_lds_fits_every_shape_the_sort_is_launched_for(shim):  # noqa: F811
    """ps_scatter_lds_bytes == the kernel's layout (four arrays of P counters, two words, 512 W staged pairs of 8 bytes) and stays below the limit launch_psort
    sets for every width 16 .. 22 in both key modes — except a set per window at width 22, which plain_geometry therefore leaves to the sweeps"""
    shim.shim_ps_scatter_lds_bytes.argtypes = [C.c_uint32, C.c_int]
    shim.shim_ps_scatter_lds_bytes.restype = shim.shim_ps_scatter_lds_max.restype = C.c_size_t
    shim.shim_plain_psort_fits.argtypes = [C.c_int, C.c_uint32]
    limit = shim.shim_ps_scatter_lds_max()
    assert limit == 160 * 1024 - 2 * 1024
    for c in range(16, 23):
        for mode in SC.MODES:
            W, B, kws, NB, pl, P = SC.geometry(c, mode)
            assert W <= 16
            got = shim.shim_ps_scatter_lds_bytes(P, W)
            assert got == 4 * (4 * P + 2) + 8 * 512 * W
            fits = got <= limit
            assert fits == ((c, mode) != (22, "window")), (c, mode, P, got)
            if mode == "window":
                assert shim.shim_plain_psort_fits(W, NB) == int(fits)
    assert SC.geometry(22, "window")[5] == 12288 and shim.shim_ps_scatter_lds_bytes(12288, 12) == 245768
    for c in range(7, 16):                                  # more than 16 windows: the sweeps, whatever the size
        W, B, _, _ = U.window_shape(c)
        assert W > 16 and shim.shim_plain_psort_fits(W, W * B) == 0


# ---- every GPU case reaches its branch (the builders assert it) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", SC.MODES)
@pytest.mark.parametrize("c,W", SC.PSORT_SHAPES)
def test_inputs_of_the_shape_cases(c, W, mode):
    for n in SC.PSORT_SIZES:
        case = SC.shape_case(c, mode, n)
        assert case["W"] == W and len(case["pairs"]) <= n * W and case["counts"].sum() == len(case["pairs"])


def test_inputs_of_the_branch_cases():
    for kind in SC.HOT:
        SC.hot_case(kind, 16, "shared"); SC.hot_case(kind, 16, "window"); SC.hot_case(kind, 20, "shared")
    for target in (16384, 16385, 32768, 41600):
        SC.direct_cap_case(target)
    SC.direct_cap_window_case()
    SC.sparse_partitions_case()
    for kind in SC.FILTERS:
        SC.filter_case(kind)
    for kind in SC.BAD:
        SC.bad_case(kind)
    for kind in SC.HEAVY:
        SC.heavy_case(kind, 16, "shared", 300); SC.heavy_case(kind, 16, "window", 256); SC.heavy_case(kind, 12, "window", 304)


@pytest.mark.parametrize("c", SC.SWEEP_WIDTHS)
def test_inputs_of_the_sweep_cases(c):
    SC.sweep_case(c)


@pytest.mark.parametrize("NB", SC.SCAN_SIZES)
def test_inputs_of_the_scan_cases(NB):
    SC.scan_case(NB)


# ---- the model and the checker ------------------------------------------------------------------------------------------------------------------------
def test_sort_model_is_signed_digits_and_is_quick():
    import time
    case = SC.shape_case(16, "shared", 4173)
    t0 = time.time()
    pairs, counts = U.sort_model(case["sc"], 16, 0, 37, 5000, None, 0)
    assert time.time() - t0 < 1.0 and len(pairs) > 60000
    want = sorted((abs(d) - 1, (37 + w * 5000 + i) | ((d < 0) << 31)) for i, s in enumerate(case["sc"]) for w, d in enumerate(U.signed_digits(s, 16)) if d)
    assert [tuple(r) for r in pairs.tolist()] == want
    B = 1 << 15
    pw, cw = U.sort_model(case["sc"][:300], 16, B, 0, 0, np.array([1] * 5 + [0] * 295, np.uint8), 0)
    want = sorted((w * B + abs(d) - 1, i | ((d < 0) << 31)) for i, s in enumerate(case["sc"][:300]) if i >= 5 for w, d in enumerate(U.signed_digits(s, 16)) if d)
    assert [tuple(r) for r in pw.tolist()] == want and len(cw) == 16 * B and cw.sum() == len(want)


def device_like(case, seed=1):
    """off[] and entries[] as a correct sort would leave them, guards included, with the order inside every bucket shuffled"""
    rng = np.random.default_rng(seed)
    pairs, counts, NB, cap = case["pairs"], case["counts"], case["NB"], case["n"] * case["W"]
    off = np.full(NB + 1 + U.SORT_GUARD, U.SORT_SENTINEL, np.uint32)
    off[:NB + 1] = np.concatenate([[0], np.cumsum(counts)])
    ent = np.full(cap + U.SORT_GUARD, U.SORT_SENTINEL, np.uint32)
    order = np.lexsort((rng.random(len(pairs)), pairs[:, 0]))
    ent[:len(pairs)] = pairs[order, 1]
    return off, ent, NB, cap


def test_check_sort_accepts_any_order_inside_a_bucket_and_refuses_damage():
    case = SC.hot_case("witness", 16, "shared")
    off, ent, NB, cap = device_like(case)
    E = len(case["pairs"])
    U.check_sort(off, ent, NB, cap, case["pairs"], case["counts"])

    def refused(mutate):
        o, e = off.copy(), ent.copy()
        mutate(o, e)
        with pytest.raises(AssertionError):
            U.check_sort(o, e, NB, cap, case["pairs"], case["counts"])
    b = int(np.nonzero(case["counts"] > 1)[0][3])
    nxt = int(off[b + 1])                                   # the first slot of the next bucket
    refused(lambda o, e: o.__setitem__(0, 1))
    refused(lambda o, e: o.__setitem__(NB, E + 1))
    refused(lambda o, e: o.__setitem__(b + 1, int(o[b + 1]) - 1))                          # a term moves to the next bucket
    refused(lambda o, e: o.__setitem__(NB + 1, 0))                                         # the guard of off[]
    refused(lambda o, e: e.__setitem__(E, 5))                                              # one slot past the last pair
    refused(lambda o, e: e.__setitem__(cap + U.SORT_GUARD - 1, 5))                         # the last guard word
    refused(lambda o, e: e.__setitem__(nxt - 1, int(e[nxt - 1]) ^ (1 << 31)))              # a sign
    refused(lambda o, e: e.__setitem__(nxt - 1, int(e[nxt - 2])))                          # a term twice, its neighbour lost
    refused(lambda o, e: e.__setitem__(slice(nxt - 1, nxt + 1), e[nxt - 1:nxt + 1][::-1].copy()))   # two terms swapped across a bucket border
