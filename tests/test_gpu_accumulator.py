"""GPU (-m gpu): dgpu_accumulator_update_factors / dgpu_accumulator_update_witnesses_g1 — the accumulator manager's batch witness update (crypto_amd/csrc/
acc_kernels.hip.h, dock_accumulator.hip) against two independent oracles.
 (a) the Python transcription of the reference's memoized formulas (tests/acc_model.py): the factors limb for limb, and the new witnesses bit for bit,
     identity flags included, against tests/util.py's mul_add_oracle applied twice to those factors (T = g V, then T + f C);
 (b) the closed form, which uses none of the polynomials: with V = v G and C_i = v / (y_i + alpha) G every new witness is v' / (y_i + alpha) G,
     v' = v prod (a + alpha) / prod (r + alpha), by the oracle's scalar multiplication.
Shapes: one element to several blocks, list lengths around the minimum chunk length, the chunk count forced to 1, 2 and 5 through the development twin,
and a call of three holders and long lists that must split by itself."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import acc_model as AM
import crypto_amd as ca
from crypto_amd import accumulator as ACC
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu
R = AM.R
R2 = pow(2, 256, R)
CH = 32                                    # acck::ACC_MIN_CHUNK
SHAPES = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (5, 3), (0, 6), (CH - 1, CH + 1), (3 * CH + 1, 2 * CH)]
G = O.G1


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
    """an accumulator V = v G over the secret key alpha, `m` holders with valid witnesses C_i = v / (y_i + alpha) G, and lists to add and remove; built once"""
    def __init__(self, m, n_add, n_rem, seed):
        rng = np.random.default_rng(seed)
        self.alpha, self.v = rand(rng, 2)
        self.ys, self.adds, self.rems = rand(rng, m), rand(rng, n_add), rand(rng, n_rem)
        self.V = g_times([self.v])[0]
        self.C = g_times([self.v * pow(y + self.alpha, R - 2, R) for y in self.ys])

    def closed_form(self, na, nr, m):
        vn = self.v
        for a in self.adds[:na]:
            vn = vn * (a + self.alpha) % R
        for r in self.rems[:nr]:
            vn = vn * pow(r + self.alpha, R - 2, R) % R
        return g_times([vn * pow(y + self.alpha, R - 2, R) for y in self.ys[:m]])


_SC = {}


def scenario(key, *args):
    if key not in _SC:
        _SC[key] = Scenario(*args)
    return _SC[key]


def oracle_witnesses(f, g, C_, V):
    """(a): T_i = g_i V, then T_i + f_i C_i — rows and identity flags"""
    m = len(f)
    T, Tinf = U.mul_add_oracle(G, np.tile(V, (m, 1)), None, limbs(g), None, None)
    return U.mul_add_oracle(G, C_, None, limbs(f), T, Tinf)


def check(got, want_f, want_rows, want_inf):
    d, (rows, inf) = got
    assert ints(d) == want_f
    bad = U.first_bad(rows, inf, want_rows, want_inf)
    assert len(bad) == 0, bad


@pytest.mark.parametrize("na,nr", SHAPES)
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_every_shape_and_chunk_count_against_both_oracles(twin, m, na, nr):
    S = scenario("main", 257, 3 * CH + 1, 2 * CH, 41)
    adds, rems, ys, C_ = S.adds[:na], S.rems[:nr], S.ys[:m], S.C[:m]
    f, g = AM.update_factors(adds, rems, S.alpha, ys)
    rows, inf = oracle_witnesses(f, g, C_, S.V)
    assert not inf.any() and (rows == S.closed_form(na, nr, m)).all()          # the two oracles agree with each other
    try:
        for K in (1, 2, 5):
            assert twin.dgpu_dev_set_acc_split(K) == 0
            gf, gg = ACC.update_factors(adds, rems, S.alpha, ys)
            assert ints(gf) == f and ints(gg) == g, K
            assert twin.dgpu_dev_get_acc_split() == K
            check(ACC.update_witnesses(adds, rems, S.alpha, ys, C_, S.V), f, rows, inf)
    finally:
        twin.dgpu_dev_set_acc_split(0)


def test_few_holders_and_long_lists_split_by_themselves(twin):
    S = scenario("long", 3, 1000, 700, 43)
    f, g = AM.update_factors(S.adds, S.rems, S.alpha, S.ys)
    assert twin.dgpu_dev_set_acc_split(0) == 0
    gf, gg = ACC.update_factors(S.adds, S.rems, S.alpha, S.ys)
    assert twin.dgpu_dev_get_acc_split() > 1                                   # automatic: chunks of at least 32 entries
    assert ints(gf) == f and ints(gg) == g
    rows, inf = oracle_witnesses(f, g, S.C, S.V)
    assert (rows == S.closed_form(1000, 700, 3)).all()
    check(ACC.update_witnesses(S.adds, S.rems, S.alpha, S.ys, S.C, S.V), f, rows, inf)
    assert twin.dgpu_dev_get_acc_split() > 1


def edge_case():
    """65 holders, five additions, three removals: holder 3 was removed, holder 5 was just added, holder 7 holds the identity"""
    S = scenario("main", 257, 3 * CH + 1, 2 * CH, 41)
    adds, rems, ys, C_ = S.adds[:5], S.rems[:3], list(S.ys[:65]), S.C[:65].copy()
    ys[3], ys[5] = rems[1], adds[2]
    C_[7] = 0
    return S, adds, rems, ys, C_


def test_removed_added_and_identity_holders():
    S, adds, rems, ys, C_ = edge_case()
    f, g = AM.update_factors(adds, rems, S.alpha, ys)
    assert f[3] == 0 and g[3] == 0 and f[5] == 0 and g[5] != 0
    rows, inf = oracle_witnesses(f, g, C_, S.V)
    assert inf[3] == 1 and not rows[3].any() and inf.sum() == 1
    gf, gg = ACC.update_factors(adds, rems, S.alpha, ys)
    assert ints(gf) == f and ints(gg) == g
    got = ACC.update_witnesses(adds, rems, S.alpha, ys, C_, S.V)
    check(got, f, rows, inf)
    # (b) for the ordinary holders
    regular = [i for i in range(65) if i not in (3, 5, 7)]
    assert (got[1][0][regular] == S.closed_form(5, 3, 65)[regular]).all()
    # the identity accumulator: the new witnesses are f_i C_i
    zero = np.zeros(12, np.uint64)
    rows0, inf0 = U.mul_add_oracle(G, C_, None, limbs(f), None, None)
    assert inf0[3] == 1 and inf0[5] == 1 and inf0[7] == 1
    check(ACC.update_witnesses(adds, rems, S.alpha, ys, C_, zero), f, rows0, inf0)


def test_inputs_above_r_and_montgomery_words_give_the_same_points():
    S, adds, rems, ys, C_ = edge_case()
    want = ACC.update_witnesses(adds, rems, S.alpha, ys, C_, S.V)
    up = lambda vals: [v + R for v in vals]                                    # 2 r < 2^256: the same residues, not reduced
    got = ACC.update_witnesses(up(adds), rems, S.alpha + R, up(ys), C_, S.V)
    assert (got[0] == want[0]).all() and (got[1][0] == want[1][0]).all() and (got[1][1] == want[1][1]).all()
    allones = [(1 << 256) - 1]                                                 # the largest word pattern, as an addition and as an element
    f1, g1 = ACC.update_factors(adds + allones, rems, S.alpha, ys[:4] + allones)
    f2, g2 = AM.update_factors(adds + allones, rems, S.alpha, ys[:4] + allones)
    assert ints(f1) == f2 and ints(g1) == g2
    mont = lambda vals: limbs([v * R2 % R for v in vals])
    gm = ACC.update_witnesses(mont(adds), mont(rems), mont([S.alpha])[0], mont(ys), C_, S.V, montgomery=True)
    assert (gm[0] == mont(ints(want[0]))).all()                                # d_factors come back as Montgomery limbs
    assert (gm[1][0] == want[1][0]).all() and (gm[1][1] == want[1][1]).all()
    fm, gm2 = ACC.update_factors(mont(adds), mont(rems), mont([S.alpha])[0], mont(ys), montgomery=True)
    fc, gc = ACC.update_factors(adds, rems, S.alpha, ys)
    assert (fm == mont(ints(fc))).all() and (gm2 == mont(ints(gc))).all()


def test_two_threads_with_different_inputs():
    S = scenario("main", 257, 3 * CH + 1, 2 * CH, 41)
    jobs = [(S.adds[:40], S.rems[:9], S.ys[:130], S.C[:130]), (S.adds[50:57], S.rems[20:60], S.ys[100:257], S.C[100:257])]
    alone = [ACC.update_witnesses(a, r, S.alpha, y, c, S.V) for a, r, y, c in jobs]
    for (a, r, y, c), one in zip(jobs, alone):
        f, g = AM.update_factors(a, r, S.alpha, y)
        assert ints(one[0]) == f
    with ThreadPoolExecutor(2) as ex:
        for _ in range(3):
            both = list(ex.map(lambda j: ACC.update_witnesses(j[0], j[1], S.alpha, j[2], j[3], S.V), jobs))
            for got, one in zip(both, alone):
                assert (got[0] == one[0]).all() and (got[1][0] == one[1][0]).all() and (got[1][1] == one[1][1]).all()
    # the first job's points against the closed form of its own lists
    vn = S.v
    for a in jobs[0][0]:
        vn = vn * (a + S.alpha) % R
    for r in jobs[0][1]:
        vn = vn * pow(r + S.alpha, R - 2, R) % R
    assert (alone[0][1][0] == g_times([vn * pow(y + S.alpha, R - 2, R) for y in jobs[0][2]])).all()
