"""GPU: the sort stage every bucket MSM starts with, run ALONE through the development twin's hooks (include/dock_gpu_dev.h dgpu_selftest_psort, _sort_sweep,
_scan, _dyn_chunk: the product's launchers on buffers of the hook's own, outputs and 64 guard words behind each pre-filled with a sentinel) and compared,
in exact integers, with the big-integer model of tests/util.py (sort_model / dyn_chunk_model / check_sort; numpy.cumsum for the scan):
off[] and its last word, the multiset of entries[] bucket by bucket, no write past either, the heavy list and its count, the bad word, the chunk rule.
The inputs come from tests/sort_stage_cases.py, whose builders assert on the host that each reaches the branch it is named after (the same builders run
without a GPU in tests/test_sort_stage_host.py)."""
import ctypes as C
import numpy as np
import pytest
import torch
import util as U
import sort_stage_cases as SC
import crypto_amd as ca

pytestmark = pytest.mark.gpu

G = U.SORT_GUARD
NOTHING = 0xFFFFFFFF                        # the static threshold of a sort that flags no bucket (the shared sorts, the sweeps)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)


def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def out(words):
    return np.zeros(words + G, np.uint32)


def run_psort(T, case, heavy_thr=NOTHING, heavy_cap=8, dyn_args=None, place=0):
    """dgpu_selftest_psort on a case of sort_stage_cases: dict(off, entries, heavy, dyn, bad, placed)"""
    n, W, NB = case["n"], case["W"], case["NB"]
    r = dict(off=out(NB + 1), entries=out(n * W), heavy=out(1 + heavy_cap), dyn=out(5) if dyn_args is not None else None, bad=out(1))
    placed = C.c_int32(0)
    da = None if dyn_args is None else np.array(dyn_args, np.uint32)
    rc = T.dgpu_selftest_psort(p_(U.scalar_words(case["sc"])), n, case["c"], W, case["key_wstride"], case["val_base"], case["val_wstride"], p_(case["idflag"]), case["flag_base"],
                               heavy_thr, heavy_cap, p_(da), place, p_(r["off"]), p_(r["entries"]), p_(r["heavy"]), p_(r["dyn"]), p_(r["bad"]), C.byref(placed))
    assert rc == 0, rc
    r["placed"] = placed.value
    return r


def check_psort(case, r, want_bad=0, want_placed=1, what=""):
    U.check_sort(r["off"], r["entries"], case["NB"], case["n"] * case["W"], case["pairs"], case["counts"], what)
    assert r["bad"][0] == want_bad and (r["bad"][1:] == U.SORT_SENTINEL).all(), (what, r["bad"][:2])
    assert r["placed"] == want_placed, (what, r["placed"])


def check_heavy(heavy, cap, want, what=""):
    """heavy[0] counts every heavy bucket, also past the list's end; min(count, cap) distinct keys are written, all of them heavy; the rest is untouched"""
    heavy = heavy.astype(np.int64)
    assert heavy[0] == len(want), (what, int(heavy[0]), want)
    k = min(len(want), cap)
    keys = heavy[1:1 + k].tolist()
    assert len(set(keys)) == k and set(keys) <= set(want), (what, keys, want)
    if len(want) <= cap:
        assert sorted(keys) == want, (what, keys, want)
    assert (heavy[1 + k:] == U.SORT_SENTINEL).all(), (what, "heavy[] written past its entries", heavy[1 + k:1 + k + 4])


# ---- the partition sort: shapes, key modes, tile counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.PSORT_SIZES)
@pytest.mark.parametrize("mode", SC.MODES)
@pytest.mark.parametrize("c,W", SC.PSORT_SHAPES)
def test_psort_shapes(twin, c, W, mode, n):
    case = SC.shape_case(c, mode, n)
    assert case["W"] == W
    check_psort(case, run_psort(twin, case), what=(c, mode, n))


@pytest.mark.parametrize("c,mode", [(16, "shared"), (16, "window"), (20, "shared")])
@pytest.mark.parametrize("kind", SC.HOT)
def test_psort_hot_keys(twin, kind, c, mode):
    case = SC.hot_case(kind, c, mode)
    check_psort(case, run_psort(twin, case), what=(kind, c, mode))
    check_psort(case, run_psort(twin, case, place=2), want_placed=2, what=(kind, c, mode, "write combining"))


# ---- P4's two placements at the borders of their 16384-slot stages -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [16384, 16385, 32768, 41600])
def test_psort_direct_placement_past_its_cap(twin, target):
    case = SC.direct_cap_case(target)
    check_psort(case, run_psort(twin, case), what=target)                     # place = 0: the product's rule, which takes the direct form at these sizes
    check_psort(case, run_psort(twin, case, place=1), what=(target, "forced"))


def test_psort_direct_placement_past_its_cap_per_window_keys(twin):
    case = SC.direct_cap_window_case()
    check_psort(case, run_psort(twin, case))


@pytest.mark.parametrize("target", [16384, 16385, 32768, 41600])
def test_psort_write_combining_tiles(twin, target):
    case = SC.direct_cap_case(target)
    check_psort(case, run_psort(twin, case, place=2), want_placed=2, what=target)


def test_psort_write_combining_sparse_and_empty_partitions(twin):
    case = SC.sparse_partitions_case()
    check_psort(case, run_psort(twin, case, place=2), want_placed=2)
    case = SC.shape_case(16, "shared", 4173)                  # uniform scalars on the shared set: about 65 pairs in every partition, a small part of one tile
    check_psort(case, run_psort(twin, case, place=2), want_placed=2)
    case = SC.direct_cap_window_case()
    check_psort(case, run_psort(twin, case, place=2), want_placed=2)


# ---- identity filter, offsets, the bad word ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SC.FILTERS)
def test_psort_identity_filter_and_offsets(twin, kind):
    case = SC.filter_case(kind)
    assert (case["flag_base"], case["val_base"], case["val_wstride"]) == (37, 37, case["n"] + 37)
    check_psort(case, run_psort(twin, case), what=kind)


@pytest.mark.parametrize("kind", SC.BAD)
def test_psort_bad_word(twin, kind):
    case = SC.bad_case(kind)
    check_psort(case, run_psort(twin, case), want_bad=case["want_bad"], what=kind)


# ---- the heavy list -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", SC.MODES)
def test_psort_heavy_list_static_threshold(twin, mode):
    case = SC.heavy_case(SC.HEAVY[0], 16, mode, 300)
    r = run_psort(twin, case, heavy_thr=300, heavy_cap=case["heavy_cap"])
    check_psort(case, r)
    check_heavy(r["heavy"], case["heavy_cap"], case["want_heavy"])
    r = run_psort(twin, case, heavy_thr=300, heavy_cap=case["heavy_cap"], place=2)
    check_heavy(r["heavy"], case["heavy_cap"], case["want_heavy"], "write combining")
    r = run_psort(twin, case, heavy_thr=NOTHING, heavy_cap=case["heavy_cap"])          # the shared-sort form flags nothing
    check_heavy(r["heavy"], case["heavy_cap"], [])


@pytest.mark.parametrize("mode", SC.MODES)
def test_psort_heavy_list_longer_than_its_buffer(twin, mode):
    case = SC.heavy_case(SC.HEAVY[1], 16, mode, 300)
    assert case["heavy_cap"] == 4 and len(case["want_heavy"]) == 9
    r = run_psort(twin, case, heavy_thr=300, heavy_cap=4)
    check_psort(case, r)
    check_heavy(r["heavy"], 4, case["want_heavy"])


@pytest.mark.parametrize("rule,nb_shared", [(SC.G1_RULE, 0), (SC.G1_RULE, 1 << 15), (SC.G2_RULE, 0)], ids=["G1", "G1 table", "G2"])
def test_psort_heavy_list_threshold_from_the_chunk_rule(twin, rule, nb_shared):
    """with dyn: k_dyn_chunk runs between the scan and P4, the threshold is 16 ch of the dyn it wrote, and the static one passed beside it is ignored"""
    m = rule["min_chunk"]
    case = SC.heavy_case(SC.HEAVY[2], 16, "shared" if nb_shared else "window", 16 * m)
    E = len(case["pairs"])
    args = (0, m, rule["max_chunks"], rule["lanes_per_chunk"], 0, nb_shared)
    want = U.dyn_chunk_model(E, *args)
    assert want[2] == 16 * m == case["thr"]                                            # the vector's borders sit at the threshold the rule gives for its E
    r = run_psort(twin, case, heavy_thr=5, heavy_cap=case["heavy_cap"], dyn_args=args)
    check_psort(case, r)
    assert r["dyn"][:5].tolist() == list(want) and (r["dyn"][5:] == U.SORT_SENTINEL).all()
    check_heavy(r["heavy"], case["heavy_cap"], sorted(int(b) for b in np.nonzero(case["counts"] >= int(r["dyn"][2]))[0]))
    # a forced length moves the threshold: 19 terms a chunk, heavy from 304
    case = SC.heavy_case(SC.HEAVY[0], 16, "window", 304)
    r = run_psort(twin, case, heavy_thr=5, heavy_cap=8, dyn_args=(19,) + args[1:])
    assert r["dyn"][:5].tolist() == list(U.dyn_chunk_model(len(case["pairs"]), 19, *args[1:])) and r["dyn"][2] == 304
    check_heavy(r["heavy"], 8, case["want_heavy"])


# ---- the sweep route -----------------------------------------------------------------------------------------------------------------------------------------
def run_sweep(T, case, g2=0, bases=None, fixed_ch=0, heavy_cap=0):
    n, W, NB = case["n"], case["W"], case["NB"]
    cap = heavy_cap if heavy_cap else n * W // 256 + 1
    r = dict(off=out(NB + 1), cursor=out(NB), entries=out(n * W), heavy=out(1 + cap), dyn=out(5), bad=out(1), cap=cap)
    rc = T.dgpu_selftest_sort_sweep(p_(U.scalar_words(case["sc"])), n, case["c"], g2, p_(bases), fixed_ch, heavy_cap, p_(r["off"]), p_(r["cursor"]), p_(r["entries"]), p_(r["heavy"]),
                                    p_(r["dyn"]), p_(r["bad"]))
    assert rc == 0, rc
    return r


def base_records(flags, g2):
    """prepared base records that are all zero but for the identity flag word (G1: 32 words, flag in word 28; G2: 64 words, flag in word 56)"""
    stride, word = (64, 56) if g2 else (32, 28)
    rec = np.zeros((len(flags), stride), np.uint32)
    rec[:, word] = flags
    return rec


def check_sweep(case, r, rule, pairs, counts, fixed_ch=0, what=""):
    NB, n, W = case["NB"], case["n"], case["W"]
    U.check_sort(r["off"], r["entries"], NB, n * W, pairs, counts, what)
    assert (r["cursor"][:NB] == r["off"][:NB]).all() and (r["cursor"][NB:] == U.SORT_SENTINEL).all(), what
    assert r["bad"][0] == 0 and (r["bad"][1:] == U.SORT_SENTINEL).all(), what
    T_max = U.dyn_chunk_model(n * W, 0, rule["min_chunk"], rule["max_chunks"], rule["lanes_per_chunk"], 0, 0)[1]          # acc_geometry's partial slots
    want = U.dyn_chunk_model(len(pairs), fixed_ch, rule["min_chunk"], rule["max_chunks"], rule["lanes_per_chunk"], T_max, 0)
    assert r["dyn"][:5].tolist() == list(want) and (r["dyn"][5:] == U.SORT_SENTINEL).all(), (what, r["dyn"][:5], want)
    check_heavy(r["heavy"], r["cap"], sorted(int(b) for b in np.nonzero(counts >= want[2])[0]), what)


@pytest.mark.parametrize("c", SC.SWEEP_WIDTHS)
def test_sweep_route(twin, c):
    case = SC.sweep_case(c)
    g2 = 1 if c in (12, 17) else 0
    rule = SC.G2_RULE if g2 else SC.G1_RULE
    check_sweep(case, run_sweep(twin, case, g2), rule, case["pairs"], case["counts"], what=(c, "no bases"))
    r = run_sweep(twin, case, g2, base_records(case["flags"], g2))
    check_sweep(case, r, rule, case["pairs_flagged"], case["counts_flagged"], what=(c, "identity flags"))


def test_sweep_route_bad_word(twin):
    case = dict(SC.sweep_case(13))
    sc = list(case["sc"]); sc[5] |= 1 << 255
    flags = case["flags"].copy(); flags[5] = 1
    case["sc"] = sc
    pairs, counts = U.sort_model(sc, 13, case["B"], 0, 0, flags, 0)
    r = run_sweep(twin, case, 0, base_records(flags, 0))
    U.check_sort(r["off"], r["entries"], case["NB"], case["n"] * case["W"], pairs, counts)
    assert r["bad"][0] == 1 and (r["bad"][1:] == U.SORT_SENTINEL).all()          # reported for a row the sort drops, as on the partition sort


@pytest.mark.parametrize("kind", SC.HEAVY)
def test_sweep_route_heavy_list(twin, kind):
    """k_flag_heavy: the threshold is 16 ch of the dyn the sweep route's own k_dyn_chunk wrote (19 forced: 304; the rule at this size: 256)"""
    fixed = 19 if kind == SC.HEAVY[0] else 0
    case = SC.heavy_case(kind, 12, "window", 304 if fixed else 256)
    cap = case["heavy_cap"]
    r = run_sweep(twin, case, 0, fixed_ch=fixed, heavy_cap=cap)
    assert r["dyn"][2] == case["thr"]
    check_sweep(case, r, SC.G1_RULE, case["pairs"], case["counts"], fixed_ch=fixed, what=kind)
    assert int(r["heavy"][0]) == len(case["want_heavy"]) == (9 if kind == SC.HEAVY[1] else 2)


# ---- the scan ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NB", SC.SCAN_SIZES)
def test_scan(twin, NB):
    cnt = SC.scan_case(NB)
    want = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    c32 = cnt.astype(np.uint32)
    off, cur = out(NB + 1), out(NB)
    assert twin.dgpu_selftest_scan(p_(c32), NB, 1, p_(off), p_(cur)) == 0
    assert off[NB] == want[NB], (int(off[NB]), int(want[NB]))
    bad = np.nonzero(off[:NB + 1] != want)[0]
    assert len(bad) == 0, (bad[:4], off[bad[:4]], want[bad[:4]])
    assert (cur[:NB] == want[:NB]).all()
    assert (off[NB + 1:] == U.SORT_SENTINEL).all() and (cur[NB:] == U.SORT_SENTINEL).all()
    off2 = out(NB + 1)
    assert twin.dgpu_selftest_scan(p_(c32), NB, 0, p_(off2), None) == 0               # no cursor buffer: P2 of the partition sort
    assert (off2 == off).all()


# ---- the chunk rule on the device ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [SC.G1_RULE, SC.G2_RULE], ids=["G1", "G2"])
def test_chunk_rule_on_the_device(twin, rule):
    m, mc, lanes = rule["min_chunk"], rule["max_chunks"], rule["lanes_per_chunk"]
    dyn = out(5)
    wrong = []
    for E, fixed, T_max, nb in SC.chunk_rule_table(rule):
        want = U.dyn_chunk_model(E, fixed, m, mc, lanes, T_max, nb)
        assert twin.dgpu_selftest_dyn_chunk(E, fixed, m, mc, lanes, T_max, nb, p_(dyn)) == 0
        assert (dyn[5:] == U.SORT_SENTINEL).all()
        assert not T_max or dyn[1] <= T_max, (E, fixed, T_max, nb, dyn[:5])             # never more chunks than partial slots
        if dyn[:5].tolist() != list(want):
            wrong.append(((E, fixed, T_max, nb), dyn[:5].tolist(), want))
    assert not wrong, (len(wrong), wrong[:6])


def test_chunk_rule_at_the_top_of_32_bits(twin):
    """E + ch - 1 no longer fits 32 bits from E = 2^32 - ch + 1 on; plain_geometry admits every n W < 2^32, so k_dyn_chunk takes its quotients in 64 bits and
    agrees with the host's choose_chunk (4096 terms a chunk, 2^20 chunks) — in 32 bits it reported no chunk at all"""
    dyn = out(5)
    for E, want in (((1 << 32) - 1, (4096, 1 << 20)), ((1 << 32) - 4095, (4096, 1 << 20)), ((1 << 32) - 4096, (4096, (1 << 20) - 1))):
        for T_max in (0, 1 << 20):
            assert twin.dgpu_selftest_dyn_chunk(E, 0, 16, 300000, 1, T_max, 0, p_(dyn)) == 0
            assert tuple(dyn[:2].tolist()) == want and dyn[2] == 65536 and dyn[3] == E and dyn[4] == 0, (E, T_max, dyn[:5])
            assert twin.dgpu_selftest_choose_chunk(E, 16, 300000, 1, 0) == want[0]
        assert twin.dgpu_selftest_dyn_chunk(E, 16, 16, 300000, 1, 0, 0, p_(dyn)) == 0      # a forced 16: 2^28 chunks
        assert dyn[0] == 16 and dyn[1] == -(-E // 16)
