"""GPU (-m gpu): dgpu_accumulator_d_for_batch[_resident], dgpu_accumulator_non_membership_witnesses_g1 and dgpu_accumulator_membership_witnesses_g1 —
issuing witnesses (crypto_amd/csrc/acc_kernels.hip.h d_chunk / k_acc_d / k_acc_d_combine / k_acc_issue_scalars, dock_accumulator.hip) against
 (a) the big-integer model of tests/acc_issue_model.py, limb for limb, at every shape where the kernels take another path: the switch between one and four
     non-members per lane, tail lanes, block edges, forced chunk counts and forced pass lengths;
 (b) a second, independent route to d: the d_factors of dgpu_accumulator_update_witnesses_public_g1 with additions = members and no removals;
 (c) the oracle's scalar multiplication for the points, bit for bit, and the defining relation (y + alpha) C + d P = f_V P in oracle point arithmetic;
 (d) the closed form of the existing update scenario, for membership witnesses issued here and then updated with the secret key.
One scenario (1025 non-members, 1000 members) is built once; every shape is a prefix of it."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import acc_model as AM
import acc_issue_model as IM
import crypto_amd as ca
from crypto_amd import accumulator as ACC
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu
R = AM.R
R2 = pow(2, 256, R)
G = O.G1
BADARG = -3
NS = [0, 1, 31, 32, 33, 1000]
MS = [1, 3, 4, 5, 255, 256, 257, 1025]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)
    yield


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def mont(vals):
    return limbs([v * R2 % R for v in vals])


def ints(a):
    return [O.limbs_to_int(row) for row in np.asarray(a).reshape(-1, 4)]


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def g_times(scalars):
    """k G as affine ABI words, on a pool of host threads"""
    return np.stack(U.pmap(lambda k: G.to_affine(G.mul(G.generator(), O.int_to_limbs(k % R, 4)))[0], scalars))


class Scenario:
    """1000 members, 1025 non-members, the secret key alpha, f_V, the accumulator V = v G and params_gen P = p G; the model's d for every prefix length in NS,
    computed once (one walk over the members)"""
    def __init__(self):
        rng = np.random.default_rng(5151)
        self.alpha, self.f_v, self.v, self.p = rand(rng, 4)
        self.members, self.ys = rand(rng, 1000), rand(rng, 1025)
        self.members[1], self.members[2], self.ys[0], self.ys[2] = R - 1, 0, R - 2, 1
        self.ym, self.ymm = limbs(self.ys), mont(self.ys)
        self.am, self.amm = limbs(self.members), mont(self.members)
        self.d, run = {0: [1] * 1025}, [1] * 1025
        for j, a in enumerate(self.members):
            run = [(a - y) * t % R for y, t in zip(self.ys, run)]
            if j + 1 in NS:
                self.d[j + 1] = run
        assert self.d[33][:5] == IM.d_for_batch(self.members[:33], self.ys[:5])
        self.V, self.P = g_times([self.v, self.p])
        self._pts = {}

    def non_membership_points(self):
        """(c) for the first 257 non-members against all 1000 members"""
        if "n" not in self._pts:
            sc = IM.non_membership_scalars(self.d[1000][:257], self.ys[:257], self.f_v, self.alpha)
            assert all(ok for _, ok in sc)
            self._pts["n"] = g_times([s * self.p for s, _ in sc])
        return self._pts["n"]

    def membership_points(self):
        if "m" not in self._pts:
            self._pts["m"] = g_times([t * self.v for t in IM.membership_scalars(self.ys[:257], self.alpha)])
        return self._pts["m"]


_S = []


def scenario():
    if not _S:
        _S.append(Scenario())
    return _S[0]


def d_both_forms(S, m, n, d_in=None):
    """(canonical words, Montgomery words) of one call in each form; the flags must agree"""
    dc, nzc = ACC.d_for_batch(S.am[:n], S.ym[:m], d_in=None if d_in is None else limbs(d_in))
    dm, nzm = ACC.d_for_batch(S.amm[:n], S.ymm[:m], d_in=None if d_in is None else mont(d_in), montgomery=True)
    assert (nzc == nzm).all()
    return dc, dm, nzc


@pytest.mark.parametrize("m", MS)
def test_d_every_shape_chunk_count_and_pass_length(twin, m):
    """every n, both word forms, K forced to 1, 2, 5 and automatic, and passes of seven members: the model's words every time"""
    S = scenario()
    try:
        for n in NS:
            want = S.d[n][:m]
            wc, wm, wnz = limbs(want), mont(want), np.array([int(d != 0) for d in want], np.uint8)
            for K in (1, 2, 5, 0):
                assert twin.dgpu_dev_set_acc_split(K) == 0
                dc, dm, nz = d_both_forms(S, m, n)
                assert (dc == wc).all() and (dm == wm).all() and (nz == wnz).all(), (n, K)
                if K:
                    assert twin.dgpu_dev_get_acc_split() == K
                if K == 1:                                                  # the switch: four non-members per lane from 256 on, when a chunk holds 512 members
                    assert twin.dgpu_dev_get_acc_d_unroll() == (4 if m >= 256 and n >= 512 else 1), (m, n)
            assert twin.dgpu_dev_set_acc_d_pass(7) == 0                      # n = 33: five passes, the last one short; n = 1000: 143
            for K in (1, 5):
                assert twin.dgpu_dev_set_acc_split(K) == 0
                dc, dm, nz = d_both_forms(S, m, n)
                assert (dc == wc).all() and (dm == wm).all() and (nz == wnz).all(), (n, K, "passes")
            assert twin.dgpu_dev_set_acc_d_pass(0) == 0
    finally:
        twin.dgpu_dev_set_acc_split(0); twin.dgpu_dev_set_acc_d_pass(0)


@pytest.mark.parametrize("m", [5, 255, 257])
def test_d_one_and_four_non_members_per_lane_agree(twin, m):
    """the form the automatic switch does not pick at this m, forced: the same words"""
    S = scenario()
    try:
        for u in (1, 4):
            assert twin.dgpu_dev_set_acc_d_unroll(u) == 0
            for n in (33, 1000):
                for K in (1, 5, 0):
                    assert twin.dgpu_dev_set_acc_split(K) == 0
                    dc, nz = ACC.d_for_batch(S.am[:n], S.ym[:m])
                    assert (dc == limbs(S.d[n][:m])).all() and nz.all(), (u, n, K)
                    assert twin.dgpu_dev_get_acc_d_unroll() == u
    finally:
        twin.dgpu_dev_set_acc_split(0); twin.dgpu_dev_set_acc_d_unroll(0)
    assert twin.dgpu_dev_set_acc_d_unroll(2) == BADARG and twin.dgpu_dev_set_acc_d_pass(-1) == BADARG


def test_d_long_list_few_points_splits_by_itself(twin):
    S = scenario()
    assert twin.dgpu_dev_set_acc_split(0) == 0
    dc, nz = ACC.d_for_batch(S.am, S.ym[:3])
    assert twin.dgpu_dev_get_acc_split() > 1                               # three non-members against 1000 members: chunks fill the device
    assert (dc == limbs(S.d[1000][:3])).all() and nz.all()


@pytest.mark.parametrize("n", [33, 1000])
def test_d_is_the_public_updates_d_factor(n):
    """(b): additions = members, no removals, no omega: d_A / d_D = d"""
    S = scenario()
    d, nz = ACC.d_for_batch(S.am[:n], S.ym[:257])
    f, _, ok = ACC.update_witnesses_public(S.am[:n], [], np.zeros((0, 12), np.uint64), S.ym[:257], np.zeros((257, 12), np.uint64))
    assert ok.all() and (f == d).all() and nz.all()


def test_partitions_chain_through_d_in():
    S = scenario()
    whole, wnz = ACC.d_for_batch(S.am, S.ym[:257])
    assert (whole == limbs(S.d[1000][:257])).all()
    for cut in (0, 1, 500, 999, 1000):
        d1, _ = ACC.d_for_batch(S.am[:cut], S.ym[:257])
        d2, nz = ACC.d_for_batch(S.am[cut:], S.ym[:257], d_in=d1)
        assert (d2 == whole).all() and (nz == wnz).all(), cut
    m1, _ = ACC.d_for_batch(S.amm[:500], S.ymm[:257], montgomery=True)      # Montgomery words through d_in too
    m2, _ = ACC.d_for_batch(S.amm[500:], S.ymm[:257], d_in=m1, montgomery=True)
    assert (m2 == mont(S.d[1000][:257])).all()


def test_resident_members_equal_the_host_form_on_the_same_slice(twin):
    S = scenario()
    res = ca.DeviceScalars(S.amm, montgomery=True)                          # uploaded as Montgomery words: the handle holds canonical ones
    pts = ca.DeviceBases(ca.G1, np.stack([S.V, S.P]))
    try:
        for off in (0, 1, 7):
            for n in (33, 1000 - off):
                want = ACC.d_for_batch(S.am[off:off + n], S.ym[:257])
                got = ACC.d_for_batch(res, S.ym[:257], offset=off, n=n)
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (off, n)
                gm = ACC.d_for_batch(res, S.ymm[:257], offset=off, n=n, montgomery=True)      # montgomery speaks for the non-members and d only
                assert (gm[0] == mont(ints(want[0]))).all()
        assert (ACC.d_for_batch(res, S.ym[:5])[0] == limbs(S.d[1000][:5])).all()              # the whole handle by default
        twin.dgpu_dev_set_acc_d_pass(7)                                     # the resident form in passes too
        got = ACC.d_for_batch(res, S.ym[:257], offset=1, n=33)
        assert (got[0] == ACC.d_for_batch(S.am[1:34], S.ym[:257])[0]).all()
        twin.dgpu_dev_set_acc_d_pass(0)
        d1, _ = ACC.d_for_batch(res, S.ym[:257], offset=0, n=500)          # partitions of one handle chained
        d2, _ = ACC.d_for_batch(res, S.ym[:257], offset=500, n=500, d_in=d1)
        assert (d2 == limbs(S.d[1000][:257])).all()
        for bad in (dict(offset=0, n=1001), dict(offset=1001, n=0), dict(offset=7, n=994)):   # past the end
            with pytest.raises(ca.DockGpuError) as e:
                ACC.d_for_batch(res, S.ym[:5], **bad)
            assert e.value.code == BADARG
        with pytest.raises(ca.DockGpuError) as e:                          # a handle of the wrong kind
            ACC.d_for_batch(pts.handle, S.ym[:5], n=2)
        assert e.value.code == BADARG
    finally:
        twin.dgpu_dev_set_acc_d_pass(0)
        res.free(); pts.free()


def test_a_non_member_that_is_a_member_gives_zero_and_the_witness_call_marks_it(twin):
    """member 0, member n - 1 and the last member of a forced chunk (K = 5, n = 33: chunk 0 is [0, 6)): d = 0, nonzero = 0; the witness call then gives ok = 0 and
    the identity for exactly those entries"""
    S = scenario()
    n, m = 33, 65
    ys = list(S.ys[:m])
    hit = {3: S.members[0], 64: S.members[n - 1], 17: S.members[5]}
    for i, a in hit.items():
        ys[i] = a
    want = IM.d_for_batch(S.members[:n], ys)
    assert [i for i, d in enumerate(want) if d == 0] == sorted(hit)
    try:
        for K in (1, 5):
            assert twin.dgpu_dev_set_acc_split(K) == 0
            d, nz = ACC.d_for_batch(S.am[:n], ys)
            assert (d == limbs(want)).all() and list(nz) == [0 if i in hit else 1 for i in range(m)], K
    finally:
        twin.dgpu_dev_set_acc_split(0)
    (rows, inf), ok = ACC.non_membership_witnesses(d, ys, S.f_v, S.alpha, S.P)
    assert list(ok) == [0 if i in hit else 1 for i in range(m)]
    for i in hit:
        assert inf[i] == 1 and not rows[i].any()
    clean = list(S.ys[:m])                                                   # the same batch without the members: every other entry is unchanged
    dc, _ = ACC.d_for_batch(S.am[:n], clean)
    (rows_c, inf_c), ok_c = ACC.non_membership_witnesses(dc, clean, S.f_v, S.alpha, S.P)
    others = [i for i in range(m) if i not in hit]
    assert ok_c.all() and (rows[others] == rows_c[others]).all() and not inf[others].any()
    with pytest.raises(ValueError):
        ACC.get_non_membership_witnesses_for_batch(S.am[:n], ys, S.f_v, S.alpha, S.P)


@pytest.mark.parametrize("m", [1, 64, 257])
def test_witness_points_bit_for_bit(m):
    S = scenario()
    d, (rows, inf) = ACC.get_non_membership_witnesses_for_batch(S.am, S.ym[:m], S.f_v, S.alpha, S.P)
    assert (d == limbs(S.d[1000][:m])).all() and not inf.any()
    assert (rows == S.non_membership_points()[:m]).all()
    rows_m, inf_m = ACC.membership_witnesses(S.ym[:m], S.alpha, S.V)
    assert not inf_m.any() and (rows_m == S.membership_points()[:m]).all()
    # Montgomery words in: the same points
    (rm, _), okm = ACC.non_membership_witnesses(mont(S.d[1000][:m]), S.ymm[:m], mont([S.f_v])[0], mont([S.alpha])[0], S.P, montgomery=True)
    assert okm.all() and (rm == rows).all()
    assert (ACC.membership_witnesses(S.ymm[:m], mont([S.alpha])[0], S.V, montgomery=True)[0] == rows_m).all()


def test_the_defining_relation_and_the_edges_of_the_witness_calls():
    S = scenario()
    d, (rows, inf) = ACC.get_non_membership_witnesses_for_batch(S.am, S.ym[:8], S.f_v, S.alpha, S.P)
    # (y_i + alpha) C_i + d_i P == f_V P, by the oracle's point arithmetic
    lhs = U.mul_add_oracle(G, rows, None, limbs([(y + S.alpha) % R for y in S.ys[:8]]), g_times([di * S.p for di in S.d[1000][:8]]), None)
    assert not lhs[1].any() and (lhs[0] == np.tile(g_times([S.f_v * S.p])[0], (8, 1))).all()
    # f_V = d: a zero scalar, the identity with ok = 1
    (r0, i0), ok0 = ACC.non_membership_witnesses(limbs([S.f_v, 5]), S.ym[:2], S.f_v, S.alpha, S.P)
    assert list(ok0) == [1, 1] and list(i0) == [1, 0] and not r0[0].any()
    # an identity base gives identities
    zero = np.zeros(12, np.uint64)
    (rz, iz), okz = ACC.non_membership_witnesses(d, S.ym[:8], S.f_v, S.alpha, zero)
    assert okz.all() and iz.all() and not rz.any()
    rz, iz = ACC.membership_witnesses(S.ym[:8], S.alpha, zero)
    assert iz.all() and not rz.any()
    # y = -alpha has no inverse
    for call in (lambda ys: ACC.membership_witnesses(ys, S.alpha, S.V), lambda ys: ACC.non_membership_witnesses(d, ys, S.f_v, S.alpha, S.P)):
        for pos in (0, 7):
            ys = list(S.ys[:8]); ys[pos] = R - S.alpha
            with pytest.raises(ca.DockGpuError) as e:
                call(ys)
            assert e.value.code == BADARG


def test_issued_membership_witnesses_pass_through_the_update_call():
    """(d): C_i = v / (y_i + alpha) G issued here, then five additions and three removals with the secret key: v' / (y_i + alpha) G"""
    S = scenario()
    rng = np.random.default_rng(53)
    adds, rems = rand(rng, 5), rand(rng, 3)
    ys = S.ys[:65]
    C_, inf = ACC.membership_witnesses(ys, S.alpha, S.V)
    assert (C_ == S.membership_points()[:65]).all()
    d, (rows, rinf) = ACC.update_witnesses(adds, rems, S.alpha, ys, C_, S.V)
    vn = S.v
    for a in adds:
        vn = vn * (a + S.alpha) % R
    for r in rems:
        vn = vn * pow(r + S.alpha, R - 2, R) % R
    assert not rinf.any() and (rows == g_times([vn * t for t in IM.membership_scalars(ys, S.alpha)])).all()


def test_a_second_call_of_each_shape_allocates_nothing():
    S = scenario()
    L = lib()
    res = ca.DeviceScalars(S.am)
    try:
        calls = [lambda: ACC.d_for_batch(S.am, S.ym[:257]), lambda: ACC.d_for_batch(S.am, S.ym[:3], d_in=S.ym[:3]), lambda: ACC.d_for_batch(res, S.ym[:257]),
                 lambda: ACC.non_membership_witnesses(limbs(S.d[1000][:257]), S.ym[:257], S.f_v, S.alpha, S.P), lambda: ACC.membership_witnesses(S.ym[:257], S.alpha, S.V)]
        first = [c() for c in calls]                                         # the first call of each shape (it readies the context's idle slots too)
        before = L.dgpu_device_alloc_count()
        second = [c() for c in calls]
        assert L.dgpu_device_alloc_count() == before
        assert (second[0][0] == first[0][0]).all() and (second[4][0] == first[4][0]).all()
    finally:
        res.free()


def test_four_threads_at_once_agree_with_the_serial_results():
    S = scenario()
    jobs = [(S.am[:33], S.ym[:257]), (S.am, S.ym[:5]), (S.am[:1000], S.ym[:1025]), (S.am[:32], S.ym[:256])]
    alone = [ACC.d_for_batch(*j) for j in jobs]
    assert (alone[2][0] == limbs(S.d[1000])).all()
    with ThreadPoolExecutor(4) as ex:
        for _ in range(3):
            for got, one in zip(ex.map(lambda j: ACC.d_for_batch(*j), jobs), alone):
                assert (got[0] == one[0]).all() and (got[1] == one[1]).all()
