"""GPU (-m gpu): dgpu_bbs_plus_sign_many_g1, dgpu_bbs_plus_verify_each_g1 and dgpu_bbs_plus_verify_batch_g1 (crypto_amd/csrc/dock_bbs.hip, bbs_kernels.hip.h)
through crypto_amd.bbs_plus.  The key and the valid signatures come from known discrete logs (tests/bbs_model.py) through the oracle's scalar multiplication, so
every expected point is k G for a k the model computes; a dozen of them are confirmed by the oracle's own pairing on the reference's equation before any GPU
verdict is trusted.  Every comparison is bit-exact.  One scenario (4097 rows of up to 31 messages) is built once; every shape is a prefix of it."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import bbs_model as BM
import crypto_amd as ca
from crypto_amd import bbs_plus as BBS
from crypto_amd import G1 as CG1
from crypto_amd.msm import DeviceBases
from crypto_amd.pairing import multi_pairings
from crypto_amd.aggregation.ops import mul_add
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu
R = BM.R
R2 = pow(2, 256, R)
G = O.G1
NS = [1, 2, 9, 10, 11, 63, 64, 65, 257]
LS = [1, 2, 29, 30, 31]
NBIG = 4097
KINDS = ["msg", "e", "s", "swap", "identity", "other"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)
    yield


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def mont(vals):
    return limbs([v * R2 % R for v in vals])


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def g_times(scalars):
    """k G as affine ABI words (k = 0: zero words), on the oracle's host threads"""
    scalars = [k % R for k in scalars]
    out, inf = O.g1_scale_batch(np.tile(G.generator(), (len(scalars), 1)), limbs(scalars), threads=16)
    out[inf.astype(bool)] = 0
    return out


class Scenario:
    def __init__(self):
        rng = np.random.default_rng(2718)
        x, gamma = rand(rng, 2)
        self.key = BM.Key(x, gamma, rand(rng, 32))
        self.e, self.s = rand(rng, NBIG), rand(rng, NBIG)
        self.msgs = [rand(rng, 31) for _ in range(257)] + [rand(rng, 1) + [0] * 30 for _ in range(NBIG - 257)]      # (rows beyond 257 are used at L = 1 only)
        self.s[3] = 0
        self.msgs[4][0], self.msgs[5][0], self.msgs[6] = 0, R - 1, [R - 1] * 31
        self.msgs[7][28], self.msgs[7][29], self.msgs[7][30] = 0, R - 1, 0
        self.g2 = O.G2.generator()
        self.w = O.G2.to_affine(O.G2.mul(self.g2, O.int_to_limbs(x, 4)))[0]
        self.other = g_times([0xC0FFEE])[0]
        self._a, self._pts = {}, {}

    def rows(self, L, n, lo=0):
        return self.e[lo:lo + n], self.s[lo:lo + n], [m[:L] for m in self.msgs[lo:lo + n]]

    def a_scalars(self, L, n):
        e, s, m = self.rows(L, n)
        return [self.key.a(*r) for r in zip(e, s, m)]

    def sigs(self, L, n=257):
        """the valid signatures of the first n rows for L messages per row, as ABI words"""
        if (L, n) not in self._a:
            sc = self.a_scalars(L, n)
            assert all(a is not None for a in sc)
            self._a[(L, n)] = g_times(sc)
        return self._a[(L, n)]

    def param_points(self, L):
        if L not in self._pts:
            self._pts[L] = g_times(self.key.params_scalars(L))
        return self._pts[L]

    def params(self, L):
        p = self.param_points(L)
        return BBS.Params(p[0], p[1], p[2:], self.g2, self.w)


_S = []


def scenario():
    if not _S:
        _S.append(Scenario())
    return _S[0]


def test_the_oracle_confirms_the_signatures_before_any_gpu_verdict():
    """a dozen signatures: e(A, w) e(e A - b, g2) = 1 by the oracle's Miller loop and final exponentiation, and a wrong message breaks it"""
    S = scenario()
    one = O.fp12_one()
    for L, i in [(1, 0), (1, 3), (2, 4), (2, 5), (29, 6), (29, 7), (30, 0), (30, 64), (31, 6), (31, 7), (31, 256), (30, 3)]:
        e, s, m = S.e[i], S.s[i], S.msgs[i][:L]
        a = S.key.a(e, s, m)
        assert S.key.verifies(a, e, s, m)
        pts = g_times([a, S.key.d(a, e, s, m)])
        assert (pts[0] == S.sigs(L)[i]).all()
        gt = O.final_exponentiation(O.multi_miller_loop(pts, np.stack([S.w, S.g2])))
        assert gt is not None and (gt == one).all(), (L, i)
    m = [S.msgs[0][0] + 1]
    bad = g_times([S.key.a(S.e[0], S.s[0], S.msgs[0][:1]), S.key.d(S.key.a(S.e[0], S.s[0], S.msgs[0][:1]), S.e[0], S.s[0], m)])
    assert not (O.final_exponentiation(O.multi_miller_loop(bad, np.stack([S.w, S.g2]))) == one).all()


@pytest.mark.parametrize("L", LS)
def test_sign_every_shape_and_both_forms(L):
    """out_a is the oracle's affine A_i word for word — s_i = 0, m_ij = 0 and m_ij = r - 1 among the rows — and nothing is flagged"""
    S = scenario()
    want = S.sigs(L)
    with S.params(L) as P:
        for n in NS:
            e, s, m = S.rows(L, n)
            for montgomery, f in ((False, limbs), (True, mont)):
                a, bad = BBS.sign_many(P, f([S.key.x])[0], f([v for r in m for v in r]).reshape(n, L, 4), f(e), f(s), montgomery=montgomery)
                assert not bad.any() and (a == want[:n]).all(), (n, montgomery)


def test_sign_rows_without_a_signature_are_flagged_and_their_neighbours_intact():
    """e_i = -x at the first and the last row (canonical, Montgomery, and as r + (r - x) in 256 bits): flagged, zero words, every other row as before; a
    row stride longer than L reads nothing between the rows"""
    S = scenario()
    L, n = 2, 65
    want = S.sigs(L)[:n].copy()
    want[0] = 0; want[n - 1] = 0
    e, s, m = S.rows(L, n)
    e = list(e); e[0] = e[n - 1] = (R - S.key.x) % R
    wide = np.full((n, 5, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    with S.params(L) as P:
        for montgomery, f in ((False, limbs), (True, mont)):
            wide[:, :L] = f([v for r in m for v in r]).reshape(n, L, 4)
            a, bad = BBS.sign_many(P, f([S.key.x])[0], wide[:, :L], f(e), f(s), montgomery=montgomery)
            assert bad.tolist() == [1] + [0] * (n - 2) + [1] and (a == want).all(), montgomery
        wide[:, :L] = limbs([v for r in m for v in r]).reshape(n, L, 4)
        ew = limbs(e); ew[0] = limbs([2 * R - S.key.x])[0]
        a, bad = BBS.sign_many(P, limbs([S.key.x + R])[0], wide[:, :L], ew, limbs(s))
        assert bad.tolist() == [1] + [0] * (n - 2) + [1] and (a == want).all()


def test_rows_longer_than_the_many_row_kernels_accept():
    """L + 2 = 32 above a lowered dgpu_set_small_msm_max: the single-row driver inside the calls gives the same signatures and verdicts"""
    S = scenario()
    L, n = 30, 9
    e, s, m = S.rows(L, n)
    with S.params(L) as P:
        try:
            assert lib().dgpu_set_small_msm_max(8) == 0
            a, bad = BBS.sign_many(P, S.key.x, m, e, s)
            assert not bad.any() and (a == S.sigs(L)[:n]).all()
            a[4] = S.other
            assert BBS.verify_each(P, a, e, s, m).tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]
            assert not BBS.verify_batch(P, a, e, s, m, 0x1234567)
            assert BBS.verify_batch(P, S.sigs(L)[:n], e, s, m, 0x1234567)
        finally:
            lib().dgpu_set_small_msm_max(8192)


def positions(n, chunk):
    """the ends and both sides of every chunk border"""
    pos = {0, n - 1}
    for b in range(chunk, n, chunk):
        pos |= {b - 1, b}
    return sorted(pos)


def plant(S, kind, i, n, a, e, s, m):
    """one fault of `kind` at row i; returns the rows it spoils"""
    if kind == "msg":
        m[i][0] = (m[i][0] + 1) % R
    elif kind == "e":
        e[i] = (e[i] + 1) % R
    elif kind == "s":
        s[i] = (s[i] + 1) % R
    elif kind == "swap":
        j = i + 1 if i + 1 < n else i - 1
        if j < 0:
            return set()
        a[[i, j]] = a[[j, i]]
        return {i, j}
    elif kind == "identity":
        a[i] = 0
    else:
        a[i] = S.other
    return {i}


def faulty(S, L, n, chunk, shift=0, sigs=None):
    """(a, e, s, m, planted): the first n rows with a fault at every position of positions(), the kinds taken in turn; rows next to a swap are left alone"""
    e, s, m = S.rows(L, n)
    a, e, s, m = (S.sigs(L, n) if sigs is None else sigs)[:n].copy(), list(e), list(s), [list(r) for r in m]
    planted, k = set(), shift
    for i in positions(n, chunk):
        if i in planted or (i + 1 in planted and KINDS[k % 6] == "swap"):
            k += 1
            continue
        kind = KINDS[k % 6]
        if kind == "swap" and ((i + 1 < n and i + 1 in planted) or (i + 1 >= n and i - 1 in planted)):
            kind = "msg"
        planted |= plant(S, kind, i, n, a, e, s, m)
        k += 1
    return a, e, s, m, planted


def each_both_forms(P, a, e, s, m):
    n, L = len(e), len(m[0])
    ok = BBS.verify_each(P, a, e, s, m)
    okm = BBS.verify_each(P, a, mont(e), mont(s), mont([v for r in m for v in r]).reshape(n, L, 4), montgomery=True)
    assert (ok == okm).all()
    return ok


@pytest.mark.parametrize("L", LS)
def test_verify_each_is_the_complement_of_the_planted_faults(L):
    S = scenario()
    with S.params(L) as P:
        for n in NS:
            e, s, m = S.rows(L, n)
            assert each_both_forms(P, S.sigs(L)[:n], e, s, m).all(), n
            for shift in (0, 3):
                a, e, s, m, planted = faulty(S, L, n, 4096, shift)
                ok = each_both_forms(P, a, e, s, m)
                assert ok.tolist() == [0 if i in planted else 1 for i in range(n)], (n, shift)


def test_verify_each_around_forced_chunk_borders(twin):
    """sixteen rows per chunk through the development surface: every kind of fault on both sides of every border, and the signatures of a chunked sign_many"""
    S = scenario()
    L, n = 30, 65
    with S.params(L) as P:
        try:
            assert twin.dgpu_set_many_chunk_rows(16) == 0
            e, s, m = S.rows(L, n)
            a, bad = BBS.sign_many(P, S.key.x, m, e, s)
            assert not bad.any() and (a == S.sigs(L)[:n]).all()
            for shift in range(6):
                a, e, s, m, planted = faulty(S, L, n, 16, shift)
                assert len(planted) >= 9
                assert BBS.verify_each(P, a, e, s, m).tolist() == [0 if i in planted else 1 for i in range(n)], shift
                assert not BBS.verify_batch(P, a, e, s, m, 0xABCDEF0123)
            e, s, m = S.rows(L, n)
            assert BBS.verify_batch(P, S.sigs(L)[:n], e, s, m, 0xABCDEF0123) and BBS.verify_batch(P, S.sigs(L)[:n], e, s, m, 1)
        finally:
            twin.dgpu_set_many_chunk_rows(0)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_verify_each_at_the_chunk_size(n):
    """L = 1, one row below, at and above the 4096 rows of a chunk: sign_many -> verify_each round-trips to all ones, the signatures are the oracle's, and
    faults at the ends and on both sides of the border are the only zeros"""
    S = scenario()
    want = S.sigs(1, NBIG)
    with S.params(1) as P:
        e, s, m = S.rows(1, n)
        a, bad = BBS.sign_many(P, S.key.x, m, e, s)
        assert not bad.any() and (a == want[:n]).all()
        assert BBS.verify_each(P, a, e, s, m).all()
        a, e, s, m, planted = faulty(S, 1, n, 4096, n % 6, sigs=want)
        assert BBS.verify_each(P, a, e, s, m).tolist() == [0 if i in planted else 1 for i in range(n)]
        assert not BBS.verify_batch(P, a, e, s, m, 0x5EED)
        e, s, m = S.rows(1, n)
        assert BBS.verify_batch(P, want[:n], e, s, m, 0x5EED)


def test_two_threads_at_once():
    S = scenario()
    with S.params(30) as P:
        def work(k):
            n = 64 + k
            e, s, m = S.rows(30, n)
            a, bad = BBS.sign_many(P, S.key.x, m, e, s)
            fa, fe, fs, fm, planted = faulty(S, 30, n, 4096, k)
            return (a == S.sigs(30)[:n]).all() and not bad.any() and BBS.verify_each(P, a, e, s, m).all() and \
                BBS.verify_each(P, fa, fe, fs, fm).tolist() == [0 if i in planted else 1 for i in range(n)] and BBS.verify_batch(P, a, e, s, m, 77 + k)
        with ThreadPoolExecutor(2) as ex:
            assert all(ex.map(work, [0, 1, 0, 1]))


@pytest.mark.parametrize("L", [2, 30])
def test_verify_batch_single_faults_and_a_compensating_pair(L):
    S = scenario()
    n = 65
    rho = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
    with S.params(L) as P:
        e, s, m = S.rows(L, n)
        good = S.sigs(L)[:n]
        for r in (1, rho):
            assert BBS.verify_batch(P, good, e, s, m, r)
            assert BBS.verify_batch(P, good, mont(e), mont(s), mont([v for q in m for v in q]).reshape(n, L, 4), mont([r])[0], montgomery=True)
            for kind in KINDS:
                for i in (0, n // 2, n - 1):
                    a, fe, fs, fm = good.copy(), list(e), list(s), [list(q) for q in m]
                    assert plant(S, kind, i, n, a, fe, fs, fm)
                    assert not BBS.verify_batch(P, a, fe, fs, fm, r), (kind, i, r)
        # m_i1 += delta, m_j1 -= delta: the unweighted sum cannot see it, a random weight and the per-row verdicts can
        i, j, delta = 7, 40, 0x123456789
        fm = [list(q) for q in m]
        fm[i][0], fm[j][0] = (fm[i][0] + delta) % R, (fm[j][0] - delta) % R
        assert BBS.verify_batch(P, good, e, s, fm, 1)
        assert not BBS.verify_batch(P, good, e, s, fm, rho)
        assert BBS.verify_each(P, good, e, s, fm).tolist() == [0 if k in (i, j) else 1 for k in range(n)]
        # one row: the batch is the row's own verdict
        for k in (0, 5):
            assert BBS.verify_batch(P, good[k:k + 1], e[k:k + 1], s[k:k + 1], m[k:k + 1], rho) and BBS.verify_each(P, good[k:k + 1], e[k:k + 1], s[k:k + 1], m[k:k + 1]).tolist() == [1]
            assert not BBS.verify_batch(P, good[k:k + 1], e[k:k + 1], s[k:k + 1], fm[7:8], rho) and BBS.verify_each(P, good[k:k + 1], e[k:k + 1], s[k:k + 1], fm[7:8]).tolist() == [0]


def test_handles_the_calls_refuse():
    """a handle of another length (MessageCountIncompatibleWithSigParams), a precomputed one, a G2 one, no handle at all: DGPU_E_BADARG from all three calls"""
    S = scenario()
    e, s, m = S.rows(2, 3)
    with S.params(2) as P:
        pre = DeviceBases(CG1, S.param_points(2)); pre.precompute(16)      # (a window width of its own: four bases would otherwise stay plain)
        g2b = DeviceBases(ca.G2, np.tile(S.g2, (4, 1)))
        for handle, L in ((P.handle, 1), (P.handle, 3), (pre.handle, 2), (g2b.handle, 2), (0xDEADBEEF, 2)):
            class Q:
                pass
            q = Q(); q.handle, q.L, q.pk_pc, q.g2_pc = handle, L, P.pk_pc, P.g2_pc
            mm = [r[:L] for r in S.msgs[:3]]
            for call in (lambda: BBS.sign_many(q, S.key.x, mm, e, s), lambda: BBS.verify_each(q, S.sigs(2)[:3], e, s, mm), lambda: BBS.verify_batch(q, S.sigs(2)[:3], e, s, mm, 5)):
                with pytest.raises(ca.DockGpuError) as err:
                    call()
                assert err.value.code == -3, (handle, L)
        pre.free(); g2b.free()


def test_a_second_call_of_a_shape_allocates_nothing():
    """eight rows of two messages: after one warming call of each of the three calls (it readies the context's idle slots too) a second identical call
    leaves dgpu_device_alloc_count where it was"""
    S = scenario()
    L, n = 2, 8
    e, s, m = S.rows(L, n)
    good = S.sigs(L)[:n]
    with S.params(L) as P:
        calls = [("sign_many", lambda: BBS.sign_many(P, S.key.x, m, e, s)[0], good), ("verify_each", lambda: BBS.verify_each(P, good, e, s, m), np.ones(n, np.uint8)),
                 ("verify_batch", lambda: np.array([BBS.verify_batch(P, good, e, s, m, 0x5EED)]), np.array([True]))]
        for name, call, want in calls:
            assert (call() == want).all(), name
            before = lib().dgpu_device_alloc_count()
            got = call()
            assert lib().dgpu_device_alloc_count() == before, name
            assert (got == want).all(), name


def test_the_b_inside_agree_with_the_many_row_msm_of_the_pieces():
    """n = 65, L = 30: b_i from a direct dgpu_msm_g1_handle_many on the rows (1, s_i, m_i ..), d_i = e_i A_i - b_i from dgpu_g1_mul_add_batch, the verdicts from
    dgpu_multi_pairing_segments — the caller's chain — equal verify_each's on rows with planted faults"""
    S = scenario()
    L, n = 30, 65
    one = O.fp12_one()
    neg_g2 = O.G2.to_affine(O.G2.mul(S.g2, O.int_to_limbs(R - 1, 4)))[0]
    a, e, s, m, planted = faulty(S, L, n, 16, 1)
    with S.params(L) as P:
        ok = BBS.verify_each(P, a, e, s, m)
        rows = limbs([v for i in range(n) for v in BM.row(s[i], m[i])]).reshape(n, L + 2, 4)
        jac = P.bases.msm_many(rows)
        b = np.stack([G.to_affine(j)[0] for j in jac])
        assert (b == g_times([S.key.b(s[i], m[i]) for i in range(n)])).all()
        # -d_i = (-e_i) A_i + b_i, paired with -g2
        live = [i for i in range(n) if a[i].any()]
        nd = mul_add(CG1, a[live], [(R - e[i]) % R for i in live], addend=b[live])
        gts = multi_pairings([(np.stack([a[i], nd[k]]), np.stack([S.w, neg_g2])) for k, i in enumerate(live)])
        chain = [0] * n
        for k, i in enumerate(live):
            chain[i] = int((gts[k] == one).all())
        assert chain == ok.tolist() == [0 if i in planted else 1 for i in range(n)]
