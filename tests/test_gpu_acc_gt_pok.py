"""GPU (-m gpu): the four accumulator proof calls with a GT commitment (crypto_amd/csrc/dock_acc_gt.hip, acc_gt_kernels.hip.h) through crypto_amd.accumulator_gt.
The key, the witnesses and the proofs come from known discrete logs (tests/acc_gt_model.py) through the oracle's scalar multiplication and GT power, so every
point is k G and every R_E is e(G, P~)^k for a k the model computes, and every expected status is decided in the exponent (the model itself is confirmed over
real points in tests/test_acc_gt_model.py).  Every comparison is exact.  One scenario of 257 distinct proofs per kind is built once; smaller shapes are a prefix
of it, larger ones take its rows in turn."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import acc_gt_model as GM
from acc_gt_model import MEM, NM, TAMPERS
import crypto_amd as ca
from crypto_amd import accumulator_gt as AGT
from crypto_amd import G1 as CG1
from crypto_amd.accumulator import VerifierKey
from crypto_amd.msm import msm_segments
from crypto_amd.pairing import multi_pairings
from crypto_amd._native import acc_gt_lib, twin
from bbs_model import R

pytestmark = pytest.mark.gpu
R2 = pow(2, 256, R)
G = O.G1
N = 257
NS = [1, 2, 63, 64, 65, 257]
RHO = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
NPTS = GM.NPTS
# the valid edge rows of the scenario
ROW_Y0, ROW_YMAX, ROW_C0, ROW_CMAX, ROW_IDENTITIES, ROW_Q_IDENTITY, ROW_PQ_IDENTITY = 1, 2, 3, 4, 5, 6, 7
# what the verifier can be handed wrongly for the whole call, and the check every row then fails
WRONG = {MEM: {"x": 1, "yk": 2, "z": 5, "v": 5}, NM: {"pi": 1, "k": 1, "x": 3, "yk": 4, "z": 7, "v": 7}}


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


_E_GEN, _GT = [], {}


def gt_of(log):
    """e(G, P~)^log by the oracle (P~ the generator of G2), kept per log"""
    log %= R
    if log not in _GT:
        if not _E_GEN:
            _E_GEN.append(O.final_exponentiation(O.multi_miller_loop(G.generator().reshape(1, 12), O.G2.generator().reshape(1, 24))))
        _GT[log] = np.asarray(O.fp12_pow(_E_GEN[0], log), np.uint64) if log else np.asarray(O.fp12_one(), np.uint64)
    return _GT[log]


class Scenario:
    def __init__(self):
        rng = np.random.default_rng(31415)
        self.key = GM.Key(*rand(rng, 7))
        self.rows = [dict(y=rand(rng, 1)[0], d=rand(rng, 1)[0] or 1, rnd=rand(rng, 12), c=rand(rng, 1)[0]) for _ in range(N)]
        rows = self.rows
        rows[ROW_Y0]["y"], rows[ROW_YMAX]["y"], rows[ROW_C0]["c"], rows[ROW_CMAX]["c"] = 0, R - 1, 0, R - 1
        rows[ROW_IDENTITIES]["rnd"] = [0] * 12              # no randomisation, zero blindings: every commitment is the identity, R_E = 1; E_C is the witness itself
        # c = 0 and r_rho = -r_sigma: q = -(s_sigma + s_rho) Z + c E_C is the identity; with r_y = 0, r_delta_rho = -r_delta_sigma and r_v = 0 so is p, and R_E = 1
        for i in (ROW_Q_IDENTITY, ROW_PQ_IDENTITY):
            rows[i]["c"] = 0
            rows[i]["rnd"][4] = R - rows[i]["rnd"][3]
        rnd = rows[ROW_PQ_IDENTITY]["rnd"]
        rnd[2], rnd[6], rnd[10] = 0, R - rnd[5], 0
        g2 = O.G2.generator()
        self.p_tilde, self.pk = g2, O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(self.key.alpha, 4)))[0]
        self._proofs, self._pts, self._re, self._shared, self._vkey = {}, {}, {}, {}, None

    def vkey(self):
        if self._vkey is None:
            self._vkey = VerifierKey(self.pk, self.p_tilde)
        return self._vkey

    def prove(self, kind, i, forged=False):
        r = self.rows[i]
        return GM.prove_row(self.key, kind, r["y"], r["d"], r["rnd"], r["c"], forged=forged)

    def proofs(self, kind):
        if kind not in self._proofs:
            self._proofs[kind] = [self.prove(kind, i) for i in range(N)]
            self._pts[kind] = g_times([k for p in self._proofs[kind] for k in p.pts]).reshape(N, NPTS[kind], 12)
            self._re[kind] = np.stack([gt_of(p.re) for p in self._proofs[kind]])
        return self._proofs[kind]

    def points(self, kind):
        self.proofs(kind)
        return self._pts[kind], self._re[kind]

    def take(self, kind, n):
        """(proofs, points, R_E) of n rows: the scenario's rows in turn"""
        proofs = self.proofs(kind)
        idx = np.arange(n) % N
        return [proofs[i] for i in idx], self._pts[kind][idx], self._re[kind][idx]

    def shared(self, **wrong):
        """the logs -> points of V, P, X, Y, Z, K, one of them replaced by (its log + 1) G where named"""
        k = tuple(sorted(wrong))
        if k not in self._shared:
            names = ("v", "pi", "x", "yk", "z", "k")
            self._shared[k] = dict(zip(names, g_times([getattr(self.key, n) + (1 if n in wrong else 0) for n in names])))
        return self._shared[k]

    def tampered(self, kind, n, plan):
        """(proofs, points, R_E) of n rows with the tamper plan[i] applied to row i; the changed points are k G again for the changed k, the changed R_E
        e(G, P~)^k"""
        proofs, pts, re = self.take(kind, n)
        proofs, pts, re = list(proofs), pts.copy(), re.copy()
        for i, what in plan.items():
            proofs[i] = self.prove(kind, i % N, forged=True) if what == "forged" else GM.tamper(proofs[i], what)
        rows = sorted(plan)
        if rows:
            pts[rows] = g_times([k for i in rows for k in proofs[i].pts]).reshape(len(rows), NPTS[kind], 12)
            re[rows] = np.stack([gt_of(proofs[i].re) for i in rows])
        return proofs, pts, re


_S = []


def scenario():
    if not _S:
        _S.append(Scenario())
    return _S[0]


def pack(proofs, f=limbs):
    n = len(proofs)
    if n == 0:
        return np.zeros((0, 1, 4), np.uint64), np.zeros((0, 4), np.uint64)
    return f([z for p in proofs for z in p.resp]).reshape(n, len(proofs[0].resp), 4), f([p.c for p in proofs])


def heads(S, kind, **wrong):
    sh = S.shared(**wrong)
    prk = np.stack([sh["x"], sh["yk"], sh["z"]] + ([sh["k"]] if kind == NM else []))
    return (S.vkey(), sh["v"], prk) if kind == MEM else (S.vkey(), sh["v"], sh["pi"], prk)


def each(S, kind, proofs, pts, re, montgomery=False, **wrong):
    resp, c = pack(proofs, mont if montgomery else limbs)
    fn = AGT.membership_proofs_verify_each if kind == MEM else AGT.non_membership_proofs_verify_each
    return fn(*heads(S, kind, **wrong), pts, re, resp, c, montgomery=montgomery).tolist()


def each_both_forms(S, kind, proofs, pts, re, **wrong):
    st = each(S, kind, proofs, pts, re, **wrong)
    assert st == each(S, kind, proofs, pts, re, montgomery=True, **wrong)
    return st


def batch(S, kind, proofs, pts, re, rho, montgomery=False, **wrong):
    f = mont if montgomery else limbs
    resp, c = pack(proofs, f)
    fn = AGT.membership_proofs_verify_batch if kind == MEM else AGT.non_membership_proofs_verify_batch
    return fn(*heads(S, kind, **wrong), pts, re, resp, c, f([rho])[0], montgomery=montgomery)


def tamper_plan(kind, n):
    """every tamper kind once: the first row, the last row, rows between that are none of the valid edge rows"""
    kinds = list(TAMPERS[kind])
    rows = [0, n - 1] + [11 + 9 * k for k in range(len(kinds) - 2)]
    assert rows[-2] < n - 1
    return dict(zip(rows, kinds))


@pytest.mark.parametrize("kind", [MEM, NM])
def test_valid_proofs_every_shape_and_both_forms(kind):
    """status 0 for every row — y = 0, y = r - 1, c = 0, c = r - 1, identity commitments, an identity q, identities p and q with R_E = 1 among them — and one
    verdict True; Montgomery inputs give the same bytes"""
    S = scenario()
    proofs = S.proofs(kind)
    assert all(p.status(S.key) == 0 for p in proofs)
    pts, re = S.points(kind)
    one = np.asarray(O.fp12_one(), np.uint64)
    assert not pts[ROW_IDENTITIES][1:7].any() and pts[ROW_IDENTITIES][0].any() and (re[ROW_IDENTITIES] == one).all()
    sums = lambda i: proofs[i].segment_sums(S.key)[-2:]
    assert sums(ROW_Q_IDENTITY)[1] == 0 and sums(ROW_Q_IDENTITY)[0] != 0 and sums(ROW_PQ_IDENTITY) == [0, 0] and (re[ROW_PQ_IDENTITY] == one).all()
    for n in NS:
        assert each_both_forms(S, kind, proofs[:n], pts[:n], re[:n]) == [0] * n, n
        assert batch(S, kind, proofs[:n], pts[:n], re[:n], RHO) and batch(S, kind, proofs[:n], pts[:n], re[:n], RHO, montgomery=True), n
    assert batch(S, kind, proofs[:65], pts[:65], re[:65], 1) and batch(S, kind, proofs[:65], pts[:65], re[:65], R - 1)
    assert batch(S, kind, proofs[:0], pts[:0], re[:0], RHO)
    # the edge rows alone, and a GT factor on the row whose pairing has no pair left
    for i in (ROW_IDENTITIES, ROW_Q_IDENTITY, ROW_PQ_IDENTITY):
        assert each(S, kind, proofs[i:i + 1], pts[i:i + 1], re[i:i + 1]) == [0] and batch(S, kind, proofs[i:i + 1], pts[i:i + 1], re[i:i + 1], RHO), i
    i = ROW_PQ_IDENTITY
    moved = gt_of(1).reshape(1, 72)
    assert each(S, kind, proofs[i:i + 1], pts[i:i + 1], moved) == [GM.CHECKS[kind] + 1] and not batch(S, kind, proofs[i:i + 1], pts[i:i + 1], moved, RHO)


@pytest.mark.parametrize("kind", [MEM, NM])
def test_every_tamper_kind_in_one_call(kind):
    """257 proofs, every kind — R_E moved by a GT factor among them — at the first row, the last row or a row between: the status is the reference's first error,
    the neighbours verify; a wrong V, P, X, Y, Z or K handed to the verifier fails every row at its check"""
    S = scenario()
    plan = tamper_plan(kind, N)
    proofs, pts, re = S.tampered(kind, N, plan)
    want = [p.status(S.key) for p in proofs]
    for i, what in plan.items():
        assert want[i] == TAMPERS[kind][what], (i, what)
    assert sum(1 for v in want if v) == len(plan)
    assert each_both_forms(S, kind, proofs, pts, re) == want
    assert not batch(S, kind, proofs, pts, re, RHO)
    n = 9
    good, gpts, gre = S.take(kind, n)
    for name, status in WRONG[kind].items():
        want = [p.status(S.key, **{name: getattr(S.key, name) + 1}) for p in good]
        assert want[0] == status and want[ROW_CMAX] == status
        assert each(S, kind, good, gpts, gre, **{name: 1}) == want, name
        assert not batch(S, kind, good, gpts, gre, RHO, **{name: 1}), name


@pytest.mark.parametrize("kind", [MEM, NM])
def test_a_partial_proof_and_two_tampers(kind):
    """a partial proof carries no s_y: the caller writes resp_for_element where s_y goes — the right one verifies, another fails the first check that reads it;
    two tampers in a row give the lower number"""
    S = scenario()
    n = 20
    proofs, pts, re = S.take(kind, n)
    resp_for_element = [p.resp[GM.S_Y] for p in proofs]
    partial = [p.copy() for p in proofs]
    for p in partial:
        p.resp[GM.S_Y] = 0
    assert any(st for st in each(S, kind, partial, pts, re))
    for p, s in zip(partial, resp_for_element):
        p.resp[GM.S_Y] = s
    assert each(S, kind, partial, pts, re) == [0] * n
    partial[12].resp[GM.S_Y] = resp_for_element[13]
    assert each(S, kind, partial, pts, re) == [TAMPERS[kind]["s_y"] if i == 12 else 0 for i in range(n)]
    plan = {0: ("R_rho", "R_E"), 9: ("s_delta_rho", "R_sigma"), 19: ("E_C", "R_delta_sigma")}
    bad, bpts, bre = S.tampered(kind, n, {i: a for i, (a, b) in plan.items()})
    for i, (a, b) in plan.items():
        bad[i] = GM.tamper(bad[i], b)
    rows = sorted(plan)
    bpts[rows] = g_times([k for i in rows for k in bad[i].pts]).reshape(len(rows), NPTS[kind], 12)
    bre[rows] = np.stack([gt_of(bad[i].re) for i in rows])
    want = [p.status(S.key) for p in bad]
    assert [want[i] for i in rows] == [min(TAMPERS[kind][a], TAMPERS[kind][b]) for a, b in (plan[i] for i in rows)]
    assert each_both_forms(S, kind, bad, bpts, bre) == want and not batch(S, kind, bad, bpts, bre, RHO)


@pytest.mark.parametrize("kind", [MEM, NM])
def test_forced_chunk_borders(kind):
    """65 rows per chunk through the development build at n = 64, 65, 66, 131: valid rows verify; tampers at the first row, on both sides of a border and at
    the last row; the batch call, cut the same way, refuses each"""
    S = scenario()
    kinds = list(TAMPERS[kind])
    with twin(acc_gt=True) as T:
        try:
            assert T.dgpu_set_many_chunk_rows(65) == 0
            for k, n in enumerate((64, 65, 66, 131)):
                good, gpts, gre = S.take(kind, n)
                assert each(S, kind, good, gpts, gre) == [0] * n, n
                assert batch(S, kind, good, gpts, gre, RHO), n
                rows = sorted({0, min(64, n - 1), min(65, n - 1), n - 1})
                plan = {i: kinds[(5 * k + j) % len(kinds)] for j, i in enumerate(rows)}
                proofs, pts, re = S.tampered(kind, n, plan)
                want = [p.status(S.key) for p in proofs]
                assert all(want[i] == TAMPERS[kind][what] for i, what in plan.items()) and sum(1 for v in want if v) == len(plan)
                assert each(S, kind, proofs, pts, re, montgomery=bool(k & 1)) == want, n
                assert not batch(S, kind, proofs, pts, re, RHO), n
                for i in rows[1:3]:
                    one, opts, ore = S.tampered(kind, n, {i: plan[i]})
                    assert not batch(S, kind, one, opts, ore, RHO, montgomery=bool(k & 1)), (n, i)
        finally:
            T.dgpu_set_many_chunk_rows(0)


@pytest.mark.parametrize("n", [4096, 4097])
@pytest.mark.parametrize("kind", [MEM, NM])
def test_at_the_chunk_size(kind, n):
    """at and above the 4096 rows of a chunk of the each calls — and of one column block of the batch calls: every row verifies, and tampers at the ends and on
    both sides of the border are the only other statuses; the batch call sees them too"""
    S = scenario()
    proofs, pts, re = S.take(kind, n)
    assert each(S, kind, proofs, pts, re) == [0] * n
    assert batch(S, kind, proofs, pts, re, RHO)
    kinds = list(TAMPERS[kind])
    plan = {i: kinds[(i + n) % len(kinds)] for i in sorted({0, n - 1, 4094, min(4095, n - 1)})}
    bad, bpts, bre = S.tampered(kind, n, plan)
    want = [p.status(S.key) for p in bad]
    assert all(want[i] == TAMPERS[kind][what] for i, what in plan.items()) and sum(1 for v in want if v) == len(plan)
    assert each(S, kind, bad, bpts, bre) == want
    assert not batch(S, kind, bad, bpts, bre, RHO)


@pytest.mark.parametrize("kind", [MEM, NM])
def test_batch_single_tampers_a_cancelling_pair_and_mixed_statuses(kind):
    """every tamper kind alone refuses the batch, at the first row, a chunk-border row or the last row of forced chunks; two rows whose errors cancel unweighted
    — in a commitment of the G1 equation, and in R_E — pass under rho = 1, as the model says, and fail under rho = 2; rows of mixed statuses refuse"""
    S = scenario()
    n = 131
    with twin(acc_gt=True) as T:
        try:
            assert T.dgpu_set_many_chunk_rows(65) == 0
            for k, what in enumerate(TAMPERS[kind]):
                i = (0, 65, n - 1)[k % 3]
                proofs, pts, re = S.tampered(kind, n, {i: what})
                assert not GM.batch_verdict(S.key, proofs, RHO)
                assert not batch(S, kind, proofs, pts, re, RHO), (what, i)
        finally:
            T.dgpu_set_many_chunk_rows(0)
    n = 65
    i, j, X = 9, 41, 0x123456789
    for field in ("R_delta_rho", "R_E"):
        proofs, pts, re = S.take(kind, n)
        proofs, pts, re = [p.copy() for p in proofs], pts.copy(), re.copy()
        for row, dx in ((i, X), (j, -X)):
            if field == "R_E":
                proofs[row].re = (proofs[row].re + dx) % R
            else:
                proofs[row].pts[GM.R_DRHO] = (proofs[row].pts[GM.R_DRHO] + dx) % R
        pts[[i, j]] = g_times(proofs[i].pts + proofs[j].pts).reshape(2, NPTS[kind], 12)
        re[[i, j]] = np.stack([gt_of(proofs[i].re), gt_of(proofs[j].re)])
        assert GM.batch_verdict(S.key, proofs, 1) and not GM.batch_verdict(S.key, proofs, 2)
        assert batch(S, kind, proofs, pts, re, 1) and batch(S, kind, proofs, pts, re, 1, montgomery=True), field
        assert not batch(S, kind, proofs, pts, re, 2) and not batch(S, kind, proofs, pts, re, 2, montgomery=True), field
        bad = TAMPERS[kind][field]
        assert each(S, kind, proofs, pts, re) == [bad if k in (i, j) else 0 for k in range(n)]
        # one proof: the batch is the proof's own verdict
        assert batch(S, kind, proofs[:1], pts[:1], re[:1], RHO) and not batch(S, kind, proofs[i:i + 1], pts[i:i + 1], re[i:i + 1], RHO)
    proofs, pts, re = S.tampered(kind, n, {0: "R_E", 20: "s_y", 64: "forged"})
    assert len({p.status(S.key) for p in proofs}) == 3 and not batch(S, kind, proofs, pts, re, RHO)


def test_a_second_call_of_a_shape_allocates_nothing():
    """eight proofs: after one warming call of each of the four calls a second identical call leaves dgpu_device_alloc_count where it was"""
    S = scenario()
    n = 8
    for kind in (MEM, NM):
        proofs, pts, re = S.take(kind, n)
        for name, call, want in (("each", lambda: each(S, kind, proofs, pts, re), [0] * n), ("batch", lambda: batch(S, kind, proofs, pts, re, RHO), True)):
            assert call() == want, (kind, name)
            before = acc_gt_lib().dgpu_device_alloc_count()
            got = call()
            assert acc_gt_lib().dgpu_device_alloc_count() == before, (kind, name)
            assert got == want, (kind, name)


def test_four_threads_at_once_give_the_same_bytes():
    S = scenario()
    jobs = []
    for k in range(4):
        kind, n = k % 2, 62 + k
        kinds = list(TAMPERS[kind])
        proofs, pts, re = S.tampered(kind, n, {k: kinds[k], 30 + k: kinds[6 + k], n - 1: "forged"})
        jobs.append((kind, proofs, pts, re, [p.status(S.key) for p in proofs]))

    def work(k):
        kind, proofs, pts, re, want = jobs[k % 4]
        n = len(proofs)
        good, gpts, gre = S.take(kind, n)
        return each(S, kind, proofs, pts, re) == want and not batch(S, kind, proofs, pts, re, 77 + k) and batch(S, kind, good, gpts, gre, 77 + k) and \
            each(S, kind, good, gpts, gre) == [0] * n
    S.vkey(), S.shared()
    with ThreadPoolExecutor(4) as ex:
        assert all(ex.map(work, range(8)))


@pytest.mark.parametrize("kind", [MEM, NM])
def test_the_composed_chain_of_public_calls_gives_the_same_statuses(kind):
    """n = 30: the segment sums from dgpu_msm_g1_segments over the staged bases with the model's own scalars, the pairings' values from
    dgpu_multi_pairing_segments over the last two sums of every row, compared with R_E on the host — the caller's chain, with its host scalar work — equal the
    each call on rows with planted tampers"""
    S = scenario()
    n = 30
    J = GM.CHECKS[kind]
    kinds = list(TAMPERS[kind])
    proofs, pts, re = S.tampered(kind, n, {8 + k: what for k, what in enumerate(kinds[::2])})
    got = each(S, kind, proofs, pts, re)
    sh = S.shared()
    tags = {"v": 1000, "pi": 1001, "x": 1002, "yk": 1003, "z": 1004, "k": 1005}
    by_tag = {t: sh[name] for name, t in tags.items()}
    layout = GM.Proof(kind, list(range(NPTS[kind])), 0, [0] * GM.NRESP[kind], 0).bases(GM.Key(0, 0, 0, 0, 0, 0, 0), **tags)
    bases = np.stack([by_tag[t] if t >= 1000 else pts[i][t] for i in range(n) for t in layout])
    no = len(layout)
    ends = [no * i + e for i in range(n) for e in GM.SEG_ENDS[kind]]
    sums, sinf = msm_segments(CG1, bases, limbs([v for p in proofs for v in p.own()]), ends, flags=True)
    segs = J + 2
    one = np.asarray(O.fp12_one(), np.uint64)
    jobs, rows_with_pairs = [], []
    for i in range(n):
        live = [(sums[i * segs + J + s], q2) for s, q2 in ((0, S.p_tilde), (1, S.pk)) if not sinf[i * segs + J + s]]
        if live:
            jobs.append((np.stack([G.to_affine(jac)[0] for jac, _ in live]), np.stack([q2 for _, q2 in live])))
            rows_with_pairs.append(i)
    gts = dict(zip(rows_with_pairs, multi_pairings(jobs)))
    chain = []
    for i in range(n):
        bad = [j for j in range(J) if not sinf[i * segs + j]]
        value = gts.get(i, one)
        chain.append(bad[0] + 1 if bad else 0 if (np.asarray(value, np.uint64) == re[i]).all() else J + 1)
    assert chain == got == [p.status(S.key) for p in proofs]
    assert len(set(got)) == J + 2
