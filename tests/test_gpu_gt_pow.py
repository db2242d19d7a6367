"""GPU: GT powers, products of powers and membership on the device (crypto_amd/csrc/k_gt_pow.hip, dock_gt_dev.hip) through dgpu_fp12_pow_batch,
dgpu_fp12_multi_pow_device and dgpu_gt_in_subgroup_device.  Every answer is compared word for word with the host entry points dgpu_fp12_pow,
dgpu_fp12_multi_pow and dgpu_gt_in_subgroup: on GT members, cyclotomic elements outside GT, raw Miller outputs, zero and one; at the sizes where the
lane groups, the waves, the chunks and the automatic geometry change; with every setting of dgpu_set_gt_pow on the development twin."""
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd import pairing_check as PC
from crypto_amd.aggregation import ops
from crypto_amd._native import lib
from test_gt_host import elements

pytestmark = pytest.mark.gpu
R, P = U.R, U.P
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
EDGE = [0, 1, 7, 8, 9, int("8" * 64, 16), int("8" * 63 + "9", 16), 2 ** 255, 2 ** 256 - 1, R - 1, R]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)


def lim(vals):
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


@pytest.fixture(scope="module")
def pool():
    """the kinds of base, and the 8 x 16 table of host powers every tiled case is compared against (computed once)"""
    raw, gt, cyc = elements()
    one = np.asarray(O.fp12_one(), np.uint64); zero = np.zeros(72, np.uint64)
    rng = np.random.default_rng(41)
    exps = EDGE + [int.from_bytes(rng.bytes(32), "little") for _ in range(5)]
    gts = [np.asarray(g, np.uint64) for g in gt]
    more_gt = [host_pow_all(np.stack(gts), lim([3 + i] * 3))[i % 3] for i in range(8)]      # further members of GT
    bases8 = np.stack(gts + [np.asarray(cyc[0], np.uint64), np.asarray(cyc[1], np.uint64), one] + more_gt[:2])      # all cyclotomic: the short path
    tab = np.stack([host_pow_all(bases8, lim([e] * 8)) for e in exps])                      # tab[j][i] = bases8[i]^exps[j]
    return {"raw": [np.asarray(r, np.uint64) for r in raw], "gt": gts + more_gt, "cyc": [np.asarray(c, np.uint64) for c in cyc], "one": one, "zero": zero,
            "exps": exps, "bases8": bases8, "tab": tab}


def mixed(pool, n, seed=0):
    """n bases of every kind in turn with the edge exponents in turn"""
    kinds = [pool["gt"][0], pool["raw"][0], pool["cyc"][0], pool["zero"], pool["gt"][1], pool["one"], pool["raw"][1], pool["cyc"][1], pool["gt"][2], pool["raw"][2]]
    a = np.stack([kinds[(i + seed) % len(kinds)] for i in range(n)])
    e = lim([pool["exps"][(3 * i + seed) % len(pool["exps"])] for i in range(n)])
    return np.ascontiguousarray(a), np.ascontiguousarray(e)


def host_pow_all(a, e):
    def one(i):
        out = np.zeros(72, np.uint64)
        assert lib().dgpu_fp12_pow(p_(np.ascontiguousarray(a[i])), p_(np.ascontiguousarray(e[i])), p_(out)) == 0
        return out
    with ThreadPoolExecutor(16) as ex:
        return np.stack(list(ex.map(one, range(len(a)))))


def host_multi(a, e):
    out = np.zeros(72, np.uint64)
    assert lib().dgpu_fp12_multi_pow(p_(a), p_(e), len(a), p_(out)) == 0
    return out


def host_member(a):
    ok = np.zeros(len(a), np.uint8)
    assert lib().dgpu_gt_in_subgroup(p_(a), len(a), p_(ok)) == 0
    return ok


def dev_pow(a, e, stride=4, L=None):
    out = np.zeros((len(a), 72), np.uint64)
    assert (L or lib()).dgpu_fp12_pow_batch(p_(a), p_(e), stride, len(a), p_(out)) == 0
    return out


def dev_multi(a, e, L=None):
    out = np.zeros(72, np.uint64)
    assert (L or lib()).dgpu_fp12_multi_pow_device(p_(a), p_(e), len(a), p_(out)) == 0
    return out


def dev_member(a, L=None):
    ok = np.full(len(a), 7, np.uint8)
    assert (L or lib()).dgpu_gt_in_subgroup_device(p_(a), len(a), p_(ok)) == 0
    return ok


@pytest.mark.parametrize("n", [1, 6, 10, 11])
def test_pow_batch_automatic_geometry(pool, n):
    a, e = mixed(pool, n, seed=n)
    assert (dev_pow(a, e) == host_pow_all(a, e)).all()
    e0 = lim([pool["exps"][-1]])                                          # one exponent for all
    assert (dev_pow(a, e0, stride=0) == host_pow_all(a, np.repeat(e0, n, axis=0))).all()
    # the Python surface
    got = PC.fp12_pow_batch(a, [int(sum(int(w) << (64 * k) for k, w in enumerate(row))) for row in e])
    assert (got == host_pow_all(a, e)).all()


@pytest.mark.parametrize("G", [2, 3, 10])
def test_pow_batch_groups_per_wave(twin, pool, G):
    try:
        assert twin.dgpu_set_gt_pow(G, 0, 0) == 0
        for n in (G - 1, G, G + 1, 2 * G + 1):
            a, e = mixed(pool, n, seed=G + n)
            assert (dev_pow(a, e, L=twin) == host_pow_all(a, e)).all(), (G, n)
        if G == 10:
            a = np.ascontiguousarray(np.stack(pool["gt"][:10])); e = lim([pool["exps"][(i + 2) % 16] for i in range(10)])
            assert (dev_pow(a, e, L=twin) == host_pow_all(a, e)).all()                       # ten members of GT: the short path
            a = a.copy(); a[4] = pool["raw"][0]; a[7] = pool["zero"]
            assert (dev_pow(a, e, L=twin) == host_pow_all(a, e)).all()                       # the whole wave falls to the generic path
    finally:
        twin.dgpu_set_gt_pow(0, 0, 0)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 64, 65, 1000])
def test_multi_pow(twin, pool, n):
    rng = np.random.default_rng(n)
    gt = pool["gt"] + pool["cyc"] + [pool["one"]]
    a = np.ascontiguousarray(np.stack([gt[i % len(gt)] for i in range(n)]))
    e = lim([pool["exps"][i % 16] if i % 3 else int.from_bytes(rng.bytes(32), "little") for i in range(n)])
    b = a.copy(); b[n // 2] = pool["raw"][1]
    want_a, want_b = host_multi(a, e), host_multi(b, e)
    assert (dev_multi(a, e) == want_a).all() and (dev_multi(b, e) == want_b).all()          # automatic geometry, the product library
    assert (PC.fp12_multi_pow(pool["gt"][:3], [5, 6, R - 7], device=True) == PC.fp12_multi_pow(pool["gt"][:3], [5, 6, R - 7])).all()
    try:
        for k in (1, 2, 8):
            assert twin.dgpu_set_gt_pow(0, k, 0) == 0
            assert (dev_multi(a, e, L=twin) == want_a).all(), (n, k)
            assert (dev_multi(b, e, L=twin) == want_b).all(), (n, k, "one raw element")
    finally:
        twin.dgpu_set_gt_pow(0, 0, 0)


@pytest.mark.parametrize("n", [16, 17, 33])
def test_chunk_borders(twin, pool, n):
    a, e = mixed(pool, n, seed=1)
    nz = np.ascontiguousarray(np.stack([x if x.any() else pool["gt"][3] for x in a]))       # (a zero base would make the product zero)
    try:
        assert twin.dgpu_set_gt_pow(0, 0, 16) == 0
        assert (dev_pow(a, e, L=twin) == host_pow_all(a, e)).all()
        assert (dev_multi(nz, e, L=twin) == host_multi(nz, e)).all()
        assert (dev_multi(a, e, L=twin) == host_multi(a, e)).all()
        assert (dev_member(a, L=twin) == host_member(a)).all()
        assert twin.dgpu_set_gt_pow(3, 2, 16) == 0
        assert (dev_multi(nz, e, L=twin) == host_multi(nz, e)).all()
    finally:
        twin.dgpu_set_gt_pow(0, 0, 0)
    assert twin.dgpu_set_gt_pow(11, 0, 0) == -3 and twin.dgpu_set_gt_pow(0, 9, 0) == -3 and twin.dgpu_set_gt_pow(0, 0, -1) == -3


@pytest.mark.parametrize("n", [4096 + 5, 20480 + 7])
def test_where_the_automatic_geometry_changes(pool, n):
    """G becomes 2 at 4096 elements; at 20480 + 7 the second chunk's last wave is partial.  8 bases x 16 exponents tiled."""
    idx = np.arange(n)
    bi, ei = idx % 8, (idx // 8 + idx) % 16
    a = np.ascontiguousarray(pool["bases8"][bi]); e = np.ascontiguousarray(lim(pool["exps"])[ei])
    got = dev_pow(a, e)
    assert (got == pool["tab"][ei, bi]).all()
    ok = dev_member(a)
    assert (ok == host_member(pool["bases8"])[bi]).all()
    # the product of the tiled powers, folded on the host from the 128 entries: count of each (j, i) pair as an exponent of the table entry
    cnt = np.zeros((16, 8), np.int64); np.add.at(cnt, (ei, bi), 1)
    want = host_multi(np.ascontiguousarray(pool["tab"].reshape(128, 72)), lim(cnt.reshape(128)))
    assert (dev_multi(a, e) == want).all()


@pytest.mark.parametrize("n", [1, 10, 11, 61])
def test_membership(pool, n):
    a, _ = mixed(pool, n, seed=n)
    want = host_member(a)
    assert (dev_member(a) == want).all()
    assert ops.gt_in_subgroup(a, device=True) == bool(want.all())
    members = np.ascontiguousarray(np.stack(pool["gt"][:n]))
    assert ops.gt_in_subgroup(members, device=True) and ops.gt_in_subgroup(members)


def test_two_threads_at_once(pool):
    a, e = mixed(pool, 40, seed=5)
    nz = np.ascontiguousarray(np.stack([x if x.any() else pool["gt"][4] for x in a]))
    want_p, want_m = host_pow_all(a, e), host_multi(nz, e)
    res = {}
    def t1():
        res["p"] = [dev_pow(a, e) for _ in range(3)]
    def t2():
        res["m"] = [dev_multi(nz, e) for _ in range(3)]
    th = [threading.Thread(target=t1), threading.Thread(target=t2)]
    [t.start() for t in th]; [t.join() for t in th]
    assert all((r == want_p).all() for r in res["p"]) and all((r == want_m).all() for r in res["m"])


def test_a_second_call_of_the_same_shape_allocates_nothing(pool):
    a, e = mixed(pool, 300, seed=9)
    dev_pow(a, e); dev_multi(a, e); dev_member(a)
    a0 = ca.device_alloc_count()
    dev_pow(a, e); dev_multi(a, e); dev_member(a)
    assert ca.device_alloc_count() == a0
