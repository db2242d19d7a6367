"""GPU (-m gpu): dgpu_accumulator_omega_g1 / dgpu_accumulator_update_witnesses_public_g1 — the two halves of the accumulator's update from public
information (crypto_amd/csrc/acc_kernels.hip.h, dock_accumulator.hip) against three oracles.
 (a) the big-integer model of Poly_v_AD::generate (tests/acc_public_model.py: the recurrences on coefficient lists, trimmed), its values checked here
     against acc_model.poly_v_ad_eval_direct at random points; Omega's points are those coefficients times V by the oracle's scalar multiplication,
     bit for bit, the length included;
 (b) the closed form, which uses no polynomial: with V = v G and C_i = v / (y_i + alpha) G the publicly updated witness is v' / (y_i + alpha) G,
     v' = v prod (a + alpha) / prod (r + alpha);
 (c) limb-for-limb equality with dgpu_accumulator_update_witnesses_g1, the secret-key call, on the same inputs, d_factors included.
The public update is always fed the omega this library produced."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import acc_model as AM
import acc_public_model as PM
import crypto_amd as ca
from crypto_amd import accumulator as ACC
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu
R = AM.R
R2 = pow(2, 256, R)
G = O.G1
OMEGA_SHAPES = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (5, 3), (0, 6), (4, 4), (33, 31), (64, 65)]      # N = 1, 1, 1, 1, 2, 8, 8, 4, 64, 128
LONG_SHAPES = [(1024, 3), (1025, 1000)]                                                                 # N = 1024 (the first piped transform), 2048
MORE_SHAPES = [(16, 9), (20, 32), (200, 256), (300, 512)]                                               # N = 16, 32, 256, 512: the transform sizes between the others
N_OMEGA = [0, 1, 31, 32, 33, 128, 129, 300]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)
    yield


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def ints(a):
    return [O.limbs_to_int(row) for row in np.asarray(a).reshape(-1, 4)]


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def g_times(scalars):
    """k G as affine ABI words, on a pool of host threads"""
    return np.stack(U.pmap(lambda k: G.to_affine(G.mul(G.generator(), O.int_to_limbs(k % R, 4)))[0], scalars))


class Scenario:
    """an accumulator V = v G over the secret key alpha, 257 holders with valid witnesses C_i = v / (y_i + alpha) G, and lists to add and remove; built once"""
    def __init__(self):
        rng = np.random.default_rng(4141)
        self.alpha, self.v = rand(rng, 2)
        self.ys, self.adds, self.rems = rand(rng, 257), rand(rng, 1025), rand(rng, 1000)
        self.V = g_times([self.v])[0]
        self.C = g_times([self.v * pow(y + self.alpha, R - 2, R) for y in self.ys])
        self._omega, self._closed = {}, {}

    def omega(self, na, nr):
        """this library's Omega for the first na additions and nr removals"""
        if (na, nr) not in self._omega:
            self._omega[na, nr] = ACC.omega(self.adds[:na], self.rems[:nr], self.alpha, self.V)
        return self._omega[na, nr]

    def closed_form(self, na, nr):
        """(b) for all 257 holders"""
        if (na, nr) not in self._closed:
            vn = self.v
            for a in self.adds[:na]:
                vn = vn * (a + self.alpha) % R
            for r in self.rems[:nr]:
                vn = vn * pow(r + self.alpha, R - 2, R) % R
            self._closed[na, nr] = g_times([vn * pow(y + self.alpha, R - 2, R) for y in self.ys])
        return self._closed[na, nr]


_S = []


def scenario():
    if not _S:
        _S.append(Scenario())
    return _S[0]


def lists_for(n_omega):
    """list lengths whose v_AD has n_omega coefficients: the longer list is the additions for an even count, the removals for an odd one"""
    short = n_omega // 2
    return (n_omega, short) if n_omega % 2 == 0 else (short, n_omega)


def model_omega(S, adds, rems, V=None):
    """(a): (coefficients, rows, identity flags)"""
    c = PM.v_ad_coefficients(adds, rems, S.alpha)
    rng = np.random.default_rng(len(adds) * 4099 + len(rems))
    for x in rand(rng, 2) + [0, 1]:                                 # the coefficient model against the reference's evaluation formulas
        assert PM.poly_eval(c, x) == AM.poly_v_ad_eval_direct(adds, rems, S.alpha, x)
    V = S.V if V is None else V
    if not c:
        return c, np.zeros((0, 12), np.uint64), np.zeros(0, np.uint8)
    rows, inf = U.mul_add_oracle(G, np.tile(V, (len(c), 1)), None, limbs(c), None, None)
    return c, rows, inf


def check_omega(got, want):
    pts, inf = got
    c, rows, winf = want
    assert len(pts) == len(c) == len(inf)                           # omega_len
    bad = U.first_bad(pts, inf, rows, winf)
    assert len(bad) == 0, bad


@pytest.mark.parametrize("na,nr", OMEGA_SHAPES)
def test_omega_every_small_shape_and_chunk_count(twin, na, nr):
    S = scenario()
    adds, rems = S.adds[:na], S.rems[:nr]
    want = model_omega(S, adds, rems)
    assert len(want[0]) == max(na, nr)
    try:
        for K in (1, 2, 5):
            assert twin.dgpu_dev_set_acc_split(K) == 0
            check_omega(ACC.omega(adds, rems, S.alpha, S.V), want)
            if max(na, nr):
                assert twin.dgpu_dev_get_acc_split() == K
    finally:
        twin.dgpu_dev_set_acc_split(0)


@pytest.mark.parametrize("na,nr", LONG_SHAPES)
def test_omega_long_lists_split_by_themselves(twin, na, nr):
    S = scenario()
    adds, rems = S.adds[:na], S.rems[:nr]
    want = model_omega(S, adds, rems)
    assert twin.dgpu_dev_set_acc_split(0) == 0
    check_omega(ACC.omega(adds, rems, S.alpha, S.V), want)
    assert twin.dgpu_dev_get_acc_split() > 1


@pytest.mark.parametrize("na,nr", MORE_SHAPES)
def test_omega_the_transform_sizes_in_between(na, nr):
    S = scenario()
    adds, rems = S.adds[:na], S.rems[:nr]
    check_omega(ACC.omega(adds, rems, S.alpha, S.V), model_omega(S, adds, rems))


def test_omega_of_a_long_batch_by_evaluation():
    """(5000, 4000): N = 8192, the piped transform with a strided pass and the un-reversal at 13 bits.  The quadratic coefficient model would take the better
    part of a minute here, so the 5000 points are checked through what they must satisfy instead, each check O(n): sum_j x^j omega_j = v_AD(x) V at two
    random x (a random combination of ALL coefficients: a wrong or misplaced one passes with probability 5000 / r), omega_0 = v_AD(0) V, and the leading
    coefficient, which is (-1)^(n_add - 1) for n_add > n_rem (S <- S (a - x) + F starts from F_0 = 1)."""
    S = scenario()
    rng = np.random.default_rng(5040)
    adds, rems = rand(rng, 5000), rand(rng, 4000)
    pts, inf = ACC.omega(adds, rems, S.alpha, S.V)
    assert len(pts) == 5000 and not inf.any()

    def times_v(k):
        return g_times([k % R * S.v])[0]
    assert (pts[0] == times_v(AM.poly_v_ad_eval_direct(adds, rems, S.alpha, 0))).all()
    assert (pts[4999] == times_v(-1)).all()                          # (-1)^4999
    for x in rand(rng, 2):
        powers = PM.scaled_powers(x, 1, 5000)
        got, ginf = G.to_affine(G.msm(pts, limbs(powers), threads=16))
        assert not ginf and (got == times_v(AM.poly_v_ad_eval_direct(adds, rems, S.alpha, x))).all()


def test_omega_vanishing_polynomial_identity_accumulator_and_word_forms():
    S = scenario()
    a = S.adds[0]
    pts, inf = ACC.omega([a], [a], S.alpha, S.V)                    # 1 - (a + alpha) / (a + alpha) = 0: the leading (only) coefficient vanishes
    assert len(pts) == 0 and len(inf) == 0
    assert PM.v_ad_coefficients([a], [a], S.alpha) == []
    # the identity accumulator: every entry an identity, the length from the coefficients
    zero = np.zeros(12, np.uint64)
    pts, inf = ACC.omega(S.adds[:5], S.rems[:3], S.alpha, zero)
    assert len(pts) == 5 and inf.all() and not pts.any()
    # inputs >= r and Montgomery words: the same points
    want = ACC.omega(S.adds[:33], S.rems[:31], S.alpha, S.V)
    up = lambda vals: [v + R for v in vals]
    got = ACC.omega(up(S.adds[:33]), up(S.rems[:31]), S.alpha + R, S.V)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    mont = lambda vals: limbs([v * R2 % R for v in vals])
    got = ACC.omega(mont(S.adds[:33]), mont(S.rems[:31]), mont([S.alpha])[0], S.V, montgomery=True)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    # an addition equal to -alpha is refused
    with pytest.raises(ca.DockGpuError):
        ACC.omega([R - S.alpha], S.rems[:2], S.alpha, S.V)


def same(got, want):
    return (got[0] == want[0]).all() and (got[1][0] == want[1][0]).all() and (got[1][1] == want[1][1]).all()


@pytest.mark.parametrize("n_omega", N_OMEGA)
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_public_update_every_shape_against_the_closed_form_and_the_secret_key_call(m, n_omega):
    S = scenario()
    na, nr = lists_for(n_omega)
    adds, rems, ys, C_ = S.adds[:na], S.rems[:nr], S.ys[:m], S.C[:m]
    om = S.omega(na, nr)
    assert len(om[0]) == n_omega
    d, (rows, inf), ok = ACC.update_witnesses_public(adds, rems, om, ys, C_)
    assert ok.all() and not inf.any()
    assert (rows == S.closed_form(na, nr)[:m]).all()                                                    # (b)
    sk = ACC.update_witnesses(adds, rems, S.alpha, ys, C_, S.V)                                         # (c)
    assert same((d, (rows, inf)), sk)
    assert ints(d) == [PM.public_factors(adds, rems, y)[0] for y in ys]


def edge_case():
    """65 holders, five additions, three removals: holder 3 was removed, holder 5 was just added, holder 7 holds the identity"""
    S = scenario()
    adds, rems, ys, C_ = S.adds[:5], S.rems[:3], list(S.ys[:65]), S.C[:65].copy()
    ys[3], ys[5] = rems[1], adds[2]
    C_[7] = 0
    return S, adds, rems, ys, C_


def test_removed_added_and_identity_holders():
    S, adds, rems, ys, C_ = edge_case()
    om = S.omega(5, 3)
    d, (rows, inf), ok = ACC.update_witnesses_public(adds, rems, om, ys, C_)
    assert list(ok) == [0 if i == 3 else 1 for i in range(65)]
    assert ints(d)[3] == 0 and inf[3] == 1 and not rows[3].any()      # the reference's CannotBeZero, for that holder alone
    assert ints(d)[5] == 0 and inf[5] == 0
    sk = ACC.update_witnesses(adds, rems, S.alpha, ys, C_, S.V)       # (c): the secret-key call treats all three the same way
    assert same((d, (rows, inf)), sk)
    regular = [i for i in range(65) if i not in (3, 5, 7)]
    assert (rows[regular] == S.closed_form(5, 3)[:65][regular]).all()  # (b)
    # holder 7 (the identity witness) gets T_7 alone: the model's scaled powers against omega, by the oracle
    f7, s7, _ = PM.public_factors(adds, rems, ys[7])
    c = PM.v_ad_coefficients(adds, rems, S.alpha)
    want7 = g_times([PM.poly_eval(c, ys[7]) * s7 % R * S.v])[0]
    assert (rows[7] == want7).all() and inf[7] == 0


def test_omega_with_an_identity_in_the_middle_and_no_flags():
    S, adds, rems, ys, C_ = edge_case()
    pts, oinf = S.omega(5, 3)
    pts = pts.copy(); pts[2] = 0                                       # as if c_2 were zero: zero words, and no flag array at all
    got = ACC.update_witnesses_public(adds, rems, pts, ys, C_)
    flagged = ACC.update_witnesses_public(adds, rems, (pts, np.array([0, 0, 1, 0, 0], np.uint8)), ys, C_)
    assert same(got, flagged) and (got[2] == flagged[2]).all()
    c = PM.v_ad_coefficients(adds, rems, S.alpha)
    c[2] = 0
    i = 11
    f, s, _ = PM.public_factors(adds, rems, ys[i])
    want = U.mul_add_oracle(G, C_[i:i + 1], None, limbs([f]), g_times([PM.poly_eval(c, ys[i]) * s % R * S.v]), None)
    assert (got[1][0][i] == want[0][0]).all()
    # n_omega is not tied to the list lengths: no omega at all gives f_i C_i
    d0, (rows0, inf0), ok0 = ACC.update_witnesses_public(adds, rems, np.zeros((0, 12), np.uint64), ys, C_)
    w0 = U.mul_add_oracle(G, C_, None, d0, None, None)
    assert len(U.first_bad(rows0, inf0, w0[0], w0[1])) == 0 and (d0 == got[0]).all()


def test_the_single_row_route_beyond_the_many_row_kernels_reach():
    S = scenario()
    na, nr = lists_for(33)
    adds, rems, ys, C_ = S.adds[:na], S.rems[:nr], S.ys[:5], S.C[:5]
    om = S.omega(na, nr)
    want = ACC.update_witnesses_public(adds, rems, om, ys, C_)
    assert (want[1][0] == S.closed_form(na, nr)[:5]).all()
    try:
        assert lib().dgpu_set_small_msm_max(16) == 0
        got = ACC.update_witnesses_public(adds, rems, om, ys, C_)
    finally:
        lib().dgpu_set_small_msm_max(8192)                             # the header's default: the ABI has no getter, and the suite's other users of the knob restore it the same way
    assert same(got, want) and (got[2] == want[2]).all()


def test_identity_rows_on_the_single_row_route():
    """three holders against an omega of 17 identities: every T_i is the identity, the rows at index 1 and 2 among them, so the witness is f_i C_i; the
    single-row route gives the bytes of the many-row route"""
    S = scenario()
    na, nr = lists_for(17)
    adds, rems, ys, C_ = S.adds[:na], S.rems[:nr], S.ys[:3], S.C[:3]
    om = (np.zeros((17, 12), np.uint64), np.ones(17, np.uint8))
    want = ACC.update_witnesses_public(adds, rems, om, ys, C_)
    w0 = U.mul_add_oracle(G, C_, None, want[0], None, None)
    assert want[2].all() and len(U.first_bad(want[1][0], want[1][1], w0[0], w0[1])) == 0
    try:
        assert lib().dgpu_set_small_msm_max(16) == 0
        got = ACC.update_witnesses_public(adds, rems, om, ys, C_)
    finally:
        lib().dgpu_set_small_msm_max(8192)
    assert same(got, want) and (got[2] == want[2]).all()


def test_inputs_above_r_and_montgomery_words_give_the_same_points():
    S, adds, rems, ys, C_ = edge_case()
    om = S.omega(5, 3)
    want = ACC.update_witnesses_public(adds, rems, om, ys, C_)
    up = lambda vals: [v + R for v in vals]                            # 2 r < 2^256: the same residues, not reduced
    got = ACC.update_witnesses_public(up(adds), up(rems), om, up(ys), C_)
    assert same(got, want) and (got[2] == want[2]).all()
    mont = lambda vals: limbs([v * R2 % R for v in vals])
    gm = ACC.update_witnesses_public(mont(adds), mont(rems), om, mont(ys), C_, montgomery=True)
    assert (gm[0] == mont(ints(want[0]))).all()                        # d_factors come back as Montgomery limbs
    assert (gm[1][0] == want[1][0]).all() and (gm[1][1] == want[1][1]).all() and (gm[2] == want[2]).all()


def test_two_threads_with_different_inputs():
    S = scenario()
    jobs = [(S.adds[:32], S.rems[:16], S.omega(32, 16), S.ys[:130], S.C[:130]), (S.adds[:64], S.rems[:129], S.omega(64, 129), S.ys[100:257], S.C[100:257])]
    alone = [ACC.update_witnesses_public(*j) for j in jobs]
    assert (alone[0][1][0] == S.closed_form(32, 16)[:130]).all() and (alone[1][1][0] == S.closed_form(64, 129)[100:257]).all()
    with ThreadPoolExecutor(2) as ex:
        for _ in range(3):
            both = list(ex.map(lambda j: ACC.update_witnesses_public(*j), jobs))
            for got, one in zip(both, alone):
                assert same(got, one) and (got[2] == one[2]).all()


def test_a_call_of_several_chunks_of_rows(twin):
    S = scenario()
    na, nr = lists_for(33)
    adds, rems = S.adds[:na], S.rems[:nr]
    om = ACC.omega(adds, rems, S.alpha, S.V)                           # (the twin's own: nothing crosses the border)
    try:
        assert twin.dgpu_set_many_chunk_rows(7) == 0                    # 65 holders: nine full chunks and a tail of two
        d, (rows, inf), ok = ACC.update_witnesses_public(adds, rems, om, S.ys[:65], S.C[:65])
    finally:
        twin.dgpu_set_many_chunk_rows(0)
    assert ok.all() and not inf.any()
    assert (rows == S.closed_form(na, nr)[:65]).all()


def test_a_second_call_of_a_shape_allocates_nothing():
    S = scenario()
    L = lib()
    adds, rems, ys, C_ = S.adds[:64], S.rems[:65], S.ys[:65], S.C[:65]
    om = ACC.omega(adds, rems, S.alpha, S.V)                           # the first call of each shape (it readies the context's idle slots too)
    ACC.update_witnesses_public(adds, rems, om, ys, C_)
    before = L.dgpu_device_alloc_count()
    om2 = ACC.omega(adds, rems, S.alpha, S.V)
    got = ACC.update_witnesses_public(adds, rems, om2, ys, C_)
    assert L.dgpu_device_alloc_count() == before
    assert (om2[0] == om[0]).all() and (got[1][0] == S.closed_form(64, 65)[:65]).all()
