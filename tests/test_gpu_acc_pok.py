"""GPU (-m gpu): the four accumulator proof calls (crypto_amd/csrc/dock_acc_pok.hip, acc_pok_kernels.hip.h) through crypto_amd.accumulator.  The key, the
witnesses and the proofs come from known discrete logs (tests/acc_pok_model.py) through the oracle's scalar multiplication, so every point is k G for a k the
model computes and every expected status is decided in the exponent; a dozen proofs per kind are confirmed by the oracle's own MSMs and pairing on the
reference's equations before any GPU verdict is trusted.  Every comparison is exact.  One scenario of 257 proofs per kind is built once; every shape is a
prefix of it."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import acc_pok_model as AM
import crypto_amd as ca
from crypto_amd import accumulator as ACC
from crypto_amd import G1 as CG1
from crypto_amd.msm import msm_segments
from crypto_amd.pairing import multi_pairings
from crypto_amd._native import lib
from bbs_model import R

pytestmark = pytest.mark.gpu
R2 = pow(2, 256, R)
P_MOD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
G = O.G1
N = 257
NBIG = 4097
NS = [1, 2, 63, 64, 65, 257]
RHO = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
MEM, NM = 0, 1
NPTS = {MEM: 3, NM: 5}
# tamper kinds of a row and the status the reference's order of errors gives each
KINDS = {MEM: {"A_identity": 1, "T": 2, "z1": 2, "z2": 2, "c": 2, "Abar": 2, "forged": 3, "forged_and_T": 2},
         NM: {"C_identity": 1, "J_identity": 2, "both_identities": 1, "zero_d": 2, "T2": 3, "s_d": 3, "c": 3, "T1": 4, "s_r": 4, "s_y": 4, "Cbar": 4, "forged": 5}}
# what the verifier can be handed wrongly for the whole call
WRONG = {MEM: {"v": 2}, NM: {"q": 3, "pi": 4, "v": 4}}


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
        rng = np.random.default_rng(27182)
        self.key = AM.Key(*rand(rng, 4))
        self.y, self.d, self.r, self.c = (rand(rng, N) for _ in range(4))
        self.blind = [rand(rng, 3) for _ in range(N)]
        # valid edge rows: zero blindings (T, respectively T1 and T2, the identity), y in {0, r - 1}, c in {0, r - 1}
        self.blind[3] = [0, 0, 0]
        self.y[4], self.y[5], self.c[9], self.c[10] = 0, R - 1, 0, R - 1
        g2 = O.G2.generator()
        self.p_tilde, self.pk = g2, O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(self.key.alpha, 4)))[0]
        self.V, self.P, self.Q = g_times([self.key.v, self.key.pi, self.key.q])
        self._proofs, self._pts, self._big, self._shared = {}, {}, {}, {}

    def vkey(self):
        return ACC.VerifierKey(self.pk, self.p_tilde)

    def prove(self, kind, i, forged=False, r=None, d=None):
        y, r, c, (b_r, b_y, b_d) = self.y[i], (self.r[i] if r is None else r), self.c[i], self.blind[i]
        if kind == MEM:
            return AM.prove_membership(self.key, self.key.membership_witness(y) + (1 if forged else 0), y, r, b_r, b_y, c)
        d = self.d[i] if d is None else d
        return AM.prove_non_membership(self.key, self.key.non_membership_witness(y, d) + (1 if forged else 0), d, y, r, b_r, b_y, b_d, c)

    def proofs(self, kind):
        if kind not in self._proofs:
            self._proofs[kind] = [self.prove(kind, i) for i in range(N)]
            self._pts[kind] = g_times([k for p in self._proofs[kind] for k in p.pts]).reshape(N, NPTS[kind], 12)
        return self._proofs[kind]

    def points(self, kind):
        self.proofs(kind)
        return self._pts[kind]

    def big(self, kind):
        """4097 valid proofs: the 257 of the scenario over and over with a randomiser r of their own (so no two rows hold the same points)"""
        if kind not in self._big:
            proofs = [self.prove(kind, i % N, r=(self.r[i % N] + i) % R or 1) for i in range(NBIG)]
            self._big[kind] = (proofs, g_times([q for p in proofs for q in p.pts]).reshape(NBIG, NPTS[kind], 12))
        return self._big[kind]

    def shared(self, **wrong):
        """(V, P, Q) as points, one of them replaced by (its log + 1) G where named"""
        k = tuple(sorted(wrong))
        if k not in self._shared:
            self._shared[k] = g_times([self.key.v + (1 if "v" in wrong else 0), self.key.pi + (1 if "pi" in wrong else 0), self.key.q + (1 if "q" in wrong else 0)])
        return self._shared[k]

    def tampered(self, kind, n, plan, big=False):
        """(proofs, points) of the first n rows with the tamper plan[i] applied to row i; the changed points are k G again for the changed k"""
        src, spts = self.big(kind) if big else (self.proofs(kind), self.points(kind))
        proofs, pts = [p.copy() for p in src[:n]], spts[:n].copy()
        for i, kind_ in plan.items():
            proofs[i] = tamper(self, kind, i % N, proofs[i], kind_)
        rows = sorted(plan)
        if rows:
            pts[rows] = g_times([k for i in rows for k in proofs[i].pts]).reshape(len(rows), NPTS[kind], 12)
        return proofs, pts


def tamper(S, kind, i, p, what):
    bump = lambda lst, k: lst.__setitem__(k, (lst[k] + 1) % R)
    if what.startswith("forged"):
        p = S.prove(kind, i, forged=True)
    if what == "zero_d":
        return S.prove(kind, i, d=0)
    if what == "c":
        p.c = (p.c + 1) % R
    elif what in ("A_identity", "C_identity"):
        p.pts[0] = 0
    elif what == "J_identity":
        p.pts[2] = 0
    elif what == "both_identities":
        p.pts[0] = p.pts[2] = 0
    elif what in ("Abar", "Cbar"):
        bump(p.pts, 1)
    elif what in ("T", "forged_and_T"):
        bump(p.pts, 2)
    elif what in ("T1", "T2"):
        bump(p.pts, 3 if what == "T1" else 4)
    elif what in ("z1", "z2"):
        bump(p.resp, int(what[1]) - 1)
    elif what in ("s_r", "s_y", "s_d"):
        bump(p.resp, ("s_r", "s_y", "s_d").index(what))
    return p


def pack(proofs, f=limbs):
    n = len(proofs)
    if n == 0:
        return np.zeros((0, 1, 4), np.uint64), np.zeros((0, 4), np.uint64)
    return f([z for p in proofs for z in p.resp]).reshape(n, len(proofs[0].resp), 4), f([p.c for p in proofs])


def heads(S, kind, key, **wrong):
    V, P, Q = S.shared(**wrong)
    return (key, V) if kind == MEM else (key, V, P, Q)


def each(S, kind, key, proofs, pts, montgomery=False, **wrong):
    resp, c = pack(proofs, mont if montgomery else limbs)
    fn = ACC.membership_proofs_verify_each if kind == MEM else ACC.non_membership_proofs_verify_each
    return fn(*heads(S, kind, key, **wrong), pts, resp, c, montgomery=montgomery).tolist()


def each_both_forms(S, kind, key, proofs, pts, **wrong):
    st = each(S, kind, key, proofs, pts, **wrong)
    assert st == each(S, kind, key, proofs, pts, montgomery=True, **wrong)
    return st


def batch(S, kind, key, proofs, pts, rho, montgomery=False, **wrong):
    f = mont if montgomery else limbs
    resp, c = pack(proofs, f)
    fn = ACC.membership_proofs_verify_batch if kind == MEM else ACC.non_membership_proofs_verify_batch
    return fn(*heads(S, kind, key, **wrong), pts, resp, c, f([rho])[0], montgomery=montgomery)


_S = []


def scenario():
    if not _S:
        _S.append(Scenario())
    return _S[0]


def neg_point(pt):
    """-P on affine Montgomery words: y -> p - y"""
    out = pt.copy()
    if pt.any():
        y = P_MOD - sum(int(w) << (64 * k) for k, w in enumerate(pt[6:]))
        out[6:] = [(y >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]
    return out


def test_the_oracle_confirms_the_proofs_before_any_gpu_verdict():
    """a dozen proofs per kind: the Schnorr equations by the oracle's MSM over the points, the pairing by its Miller loop and final exponentiation; a wrong
    response breaks its equation, a forged witness the pairing"""
    S = scenario()
    one = O.fp12_one()
    lim = lambda v: O.int_to_limbs(v % R, 4)

    def msm_is_identity(bases, scalars):
        live = [(b, s) for b, s in zip(bases, scalars) if b.any() and s % R]
        return not live or bool(G.to_affine(G.msm(np.stack([b for b, _ in live]), np.stack([lim(s) for _, s in live])))[1])

    def pairing(x1, x2):
        gt = O.final_exponentiation(O.multi_miller_loop(np.stack([x1, neg_point(x2)]), np.stack([S.pk, S.p_tilde])))
        return gt is not None and bool((gt == one).all())

    for i in (0, 1, 2, 3, 4, 5, 9, 10, 63, 64, 65, 256):
        for kind in (MEM, NM):
            p, pts = S.proofs(kind)[i], S.points(kind)[i]
            assert p.status(S.key) == 0
            own = p.own()
            bases = [S.V, pts[0], pts[1], pts[2]] if kind == MEM else [S.Q, pts[2], pts[4], S.V, pts[0], S.P, pts[1], pts[3]]
            for lo, hi in ((0, 4),) if kind == MEM else ((0, 3), (3, 8)):
                assert msm_is_identity(bases[lo:hi], own[lo:hi]), (kind, i)
                assert not msm_is_identity(bases[lo:hi], [own[lo] + 1] + own[lo + 1:hi]), (kind, i)
            if i < 4:
                assert pairing(pts[0], pts[1]), (kind, i)
    assert not S.points(MEM)[3][2].any() and not S.points(NM)[3][3:].any()           # the zero blindings: T, T1, T2 are the identity
    for kind in (MEM, NM):
        f = S.prove(kind, 0, forged=True)
        assert f.status(S.key) == (3 if kind == MEM else 5)
        fp = g_times(f.pts[:2])
        assert not pairing(fp[0], fp[1])


@pytest.mark.parametrize("kind", [MEM, NM])
def test_valid_proofs_every_shape_and_both_forms(kind):
    """status 0 for every row — zero blindings, y = 0, y = r - 1, c = 0, c = r - 1 among them — and one verdict True; Montgomery inputs give the same bytes"""
    S = scenario()
    key, proofs, pts = S.vkey(), S.proofs(kind), S.points(kind)
    for n in NS:
        assert each_both_forms(S, kind, key, proofs[:n], pts[:n]) == [0] * n, n
        assert batch(S, kind, key, proofs[:n], pts[:n], RHO) and batch(S, kind, key, proofs[:n], pts[:n], RHO, montgomery=True), n
    assert batch(S, kind, key, proofs[:65], pts[:65], 1) and batch(S, kind, key, proofs[:65], pts[:65], R - 1)
    assert batch(S, kind, key, proofs[:0], pts[:0], RHO) and each(S, kind, key, proofs[:1], pts[:1]) == [0]


@pytest.mark.parametrize("kind", [MEM, NM])
def test_every_tamper_kind_in_one_call(kind):
    """257 proofs, every kind at the first row, the last row or a row between: the status is the reference's first error, the neighbours verify; a wrong V, P or
    Q handed to the verifier fails every row at its check"""
    S = scenario()
    key, kinds = S.vkey(), KINDS[kind]
    rows = [0, N - 1] + [11 + 17 * k for k in range(len(kinds) - 2)]
    plan = dict(zip(rows, kinds))
    proofs, pts = S.tampered(kind, N, plan)
    want = [p.status(S.key) for p in proofs]
    for i, what in plan.items():
        assert want[i] == kinds[what], (i, what)
    assert sum(1 for v in want if v) == len(plan)
    assert each_both_forms(S, kind, key, proofs, pts) == want
    assert not batch(S, kind, key, proofs, pts, RHO)
    n = 65
    good, gpts = S.proofs(kind)[:n], S.points(kind)[:n]
    for name, status in WRONG[kind].items():
        assert [p.status(S.key, **{name: getattr(S.key, name) + 1}) for p in good] == [status] * n
        assert each_both_forms(S, kind, key, good, gpts, **{name: 1}) == [status] * n, name
        assert not batch(S, kind, key, good, gpts, RHO, **{name: 1}), name


@pytest.mark.parametrize("kind", [MEM, NM])
def test_forced_chunk_borders(twin, kind):
    """65 rows per chunk through the development surface at n = 64, 65, 66, 131: valid rows verify; one tamper kind per call at the first row, on both sides of a
    border and at the last row; the batch call, cut the same way, refuses each"""
    S = scenario()
    key, kinds = S.vkey(), list(KINDS[kind])
    try:
        assert twin.dgpu_set_many_chunk_rows(65) == 0
        for k, n in enumerate((64, 65, 66, 131)):
            good, gpts = S.proofs(kind)[:n], S.points(kind)[:n]
            assert each_both_forms(S, kind, key, good, gpts) == [0] * n, n
            assert batch(S, kind, key, good, gpts, RHO), n
            for what in kinds[k::4]:
                plan = {i: what for i in sorted({0, min(64, n - 1), min(65, n - 1), n - 1})}
                proofs, pts = S.tampered(kind, n, plan)
                want = [p.status(S.key) for p in proofs]
                assert all(want[i] == KINDS[kind][what] for i in plan) and sum(1 for v in want if v) == len(plan), what
                assert each(S, kind, key, proofs, pts) == want, (n, what)
                assert not batch(S, kind, key, proofs, pts, RHO), (n, what)
    finally:
        twin.dgpu_set_many_chunk_rows(0)


@pytest.mark.parametrize("kind", [MEM, NM])
def test_batch_single_tampers_and_a_cancelling_pair(twin, kind):
    """every tamper kind alone at the first row, the last row and a chunk-border row refuses the batch; two rows whose Schnorr errors cancel unweighted pass under
    the scalar that weighs them alike (rho = 1 for membership, rho = r - 1 for non-membership, whose u_i = rho^(2i)), as the model says, and fail under rho = 2"""
    S = scenario()
    key, n = S.vkey(), 131
    try:
        assert twin.dgpu_set_many_chunk_rows(65) == 0
        for what in KINDS[kind]:
            for i in (0, 65, n - 1):
                proofs, pts = S.tampered(kind, n, {i: what})
                assert not AM.batch_verdict(S.key, proofs, RHO)
                assert not batch(S, kind, key, proofs, pts, RHO), (what, i)
    finally:
        twin.dgpu_set_many_chunk_rows(0)
    n = 65
    i, j, X, t = 7, 41, 0x123456789, (2 if kind == MEM else 3)
    even = 1 if kind == MEM else R - 1
    proofs, pts = [p.copy() for p in S.proofs(kind)[:n]], S.points(kind)[:n].copy()
    proofs[i].pts[t], proofs[j].pts[t] = (proofs[i].pts[t] + X) % R, (proofs[j].pts[t] - X) % R
    pts[[i, j]] = g_times(proofs[i].pts + proofs[j].pts).reshape(2, NPTS[kind], 12)
    assert AM.batch_verdict(S.key, proofs, even) and not AM.batch_verdict(S.key, proofs, 2)
    assert batch(S, kind, key, proofs, pts, even) and batch(S, kind, key, proofs, pts, even, montgomery=True)
    assert not batch(S, kind, key, proofs, pts, 2) and not batch(S, kind, key, proofs, pts, 2, montgomery=True)
    bad = 2 if kind == MEM else 4
    assert each(S, kind, key, proofs, pts) == [bad if k in (i, j) else 0 for k in range(n)]
    # one proof: the batch is the proof's own verdict
    assert batch(S, kind, key, proofs[:1], pts[:1], RHO) and not batch(S, kind, key, proofs[7:8], pts[7:8], RHO) and each(S, kind, key, proofs[7:8], pts[7:8]) == [bad]


@pytest.mark.parametrize("n", [4095, 4096, 4097])
@pytest.mark.parametrize("kind", [MEM, NM])
def test_at_the_chunk_size(kind, n):
    """one row below, at and above the 4096 rows of a chunk of the each calls — and of one column block of the batch calls: every row verifies, and tampers at the
    ends and on both sides of the border are the only other statuses; the batch call sees them too"""
    S = scenario()
    key = S.vkey()
    proofs, pts = S.big(kind)
    assert each(S, kind, key, proofs[:n], pts[:n]) == [0] * n
    assert batch(S, kind, key, proofs[:n], pts[:n], RHO)
    kinds = [k for k in KINDS[kind]]
    plan = {i: kinds[(i + n) % len(kinds)] for i in sorted({0, n - 1, 4094, min(4095, n - 1)})}
    bad, bpts = S.tampered(kind, n, plan, big=True)
    want = [p.status(S.key) for p in bad]
    assert all(want[i] == KINDS[kind][what] for i, what in plan.items()) and sum(1 for v in want if v) == len(plan)
    assert each(S, kind, key, bad, bpts) == want
    assert not batch(S, kind, key, bad, bpts, RHO)


def test_a_second_call_of_a_shape_allocates_nothing():
    """eight proofs: after one warming call of each of the four calls a second identical call leaves dgpu_device_alloc_count where it was"""
    S = scenario()
    key, n = S.vkey(), 8
    for kind in (MEM, NM):
        proofs, pts = S.proofs(kind)[:n], S.points(kind)[:n]
        for name, call, want in (("each", lambda: each(S, kind, key, proofs, pts), [0] * n), ("batch", lambda: batch(S, kind, key, proofs, pts, RHO), True)):
            assert call() == want, (kind, name)
            before = lib().dgpu_device_alloc_count()
            got = call()
            assert lib().dgpu_device_alloc_count() == before, (kind, name)
            assert got == want, (kind, name)


def test_four_threads_at_once_give_the_same_bytes():
    S = scenario()
    key = S.vkey()
    jobs = []
    for k in range(4):
        kind, n = k % 2, 62 + k
        kinds = list(KINDS[kind])
        proofs, pts = S.tampered(kind, n, {k: kinds[k], 30 + k: kinds[4 + k], n - 1: "forged"})
        jobs.append((kind, proofs, pts, [p.status(S.key) for p in proofs]))

    def work(k):
        kind, proofs, pts, want = jobs[k % 4]
        n = len(proofs)
        good, gpts = S.proofs(kind)[:n], S.points(kind)[:n]
        return each(S, kind, key, proofs, pts) == want and not batch(S, kind, key, proofs, pts, 77 + k) and batch(S, kind, key, good, gpts, 77 + k) and \
            each(S, kind, key, good, gpts) == [0] * n
    with ThreadPoolExecutor(4) as ex:
        assert all(ex.map(work, range(8)))


@pytest.mark.parametrize("kind", [MEM, NM])
def test_the_composed_chain_of_public_calls_gives_the_same_statuses(kind):
    """n = 40: the segment sums from dgpu_msm_g1_segments over the staged bases with the model's own scalars, the pairings from dgpu_multi_pairing_segments — the
    caller's chain, with its host scalar work — equal the each call on rows with planted tampers"""
    S = scenario()
    key, n = S.vkey(), 40
    one = O.fp12_one()
    proofs, pts = S.tampered(kind, n, dict(zip(range(2, 2 + 3 * len(KINDS[kind]), 3), KINDS[kind])))
    got = each(S, kind, key, proofs, pts)
    if kind == MEM:
        bases = np.stack([q for i in range(n) for q in (S.V, pts[i][0], pts[i][1], pts[i][2])])
        ends = [4 * (i + 1) for i in range(n)]
    else:
        bases = np.stack([q for i in range(n) for q in (S.Q, pts[i][2], pts[i][4], S.V, pts[i][0], S.P, pts[i][1], pts[i][3])])
        ends = [v for i in range(n) for v in (8 * i + 3, 8 * i + 8)]
    _, sinf = msm_segments(CG1, bases, limbs([v for p in proofs for v in p.own()]), ends, flags=True)
    gts = multi_pairings([(np.stack([pts[i][0], neg_point(pts[i][1])]), np.stack([S.pk, S.p_tilde])) for i in range(n)])
    chain = []
    for i in range(n):
        pair = bool((gts[i] == one).all())
        if kind == MEM:
            chain.append(1 if not pts[i][0].any() else 2 if not sinf[i] else 3 if not pair else 0)
        else:
            chain.append(1 if not pts[i][0].any() else 2 if not pts[i][2].any() else 3 if not sinf[2 * i] else 4 if not sinf[2 * i + 1] else 5 if not pair else 0)
    assert chain == got == [p.status(S.key) for p in proofs]
    assert len(set(got)) == (4 if kind == MEM else 6)
