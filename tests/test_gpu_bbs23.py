"""GPU (-m gpu): the seven dgpu_bbs23_* calls (crypto_amd/csrc/dock_bbs.hip, bbs_kernels.hip.h with one fixed column, bbs23_kernels.hip.h) through
crypto_amd.bbs_23.  The key, the signatures and the proofs come from known discrete logs (tests/bbs23_model.py) through the oracle's scalar multiplication, so every
point is k G for a k the model computes and every expected byte is decided in the exponent (tests/test_bbs23_model.py pins the model against the oracle's own MSM
and pairing).  Every comparison is exact.  One scenario of 257 rows of up to 32 messages is built once; every shape is a prefix of it.  Edge rows: e = 0 (3),
messages 0 and r - 1 (4, 5, 6), c = 0 (9), c = r - 1 (10), all-hidden (i = 1 mod 6) and all-revealed (2 mod 6) masks, and the last CDL row has r1 = 0: its Abar
is the identity and its status 1."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import bbs23_model as M
import crypto_amd as ca
from crypto_amd import bbs_23 as B23
from crypto_amd import G1 as CG1
from crypto_amd.msm import DeviceBases, msm_segments
from crypto_amd.pairing import multi_pairings
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu
R, CDL, IETF = M.R, M.CDL, M.IETF
R2 = pow(2, 256, R)
P_MOD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
G = O.G1
N = 257
NBIG = 4097
NS = [1, 2, 9, 10, 11, 63, 64, 65, 257]
LS = [1, 2, 30, 31, 32]
RHO = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
NPTS = {CDL: 5, IETF: 3}
# tamper kinds and the status the reference's order of errors gives each
KINDS = {CDL: {"T1": 2, "d": 2, "Bbar": 2, "z1": 2, "z2": 2, "c": 2, "T2": 3, "z3": 3, "hidden": 3, "revealed": 3, "mask": 3, "A_identity": 1, "forged": 4, "forged_and_T1": 2},
         IETF: {"T": 3, "Bbar": 3, "z_a": 3, "z_b": 3, "c": 3, "hidden": 3, "revealed": 3, "mask": 3, "A_identity": 1, "forged": 4, "forged_and_T": 3}}
IDENTITIES = {CDL: {"T1_identity": 2, "T2_identity": 3, "Bbar_identity": 2}, IETF: {"T_identity": 3, "Bbar_identity": 3}}
POINT_OF = {CDL: {"Bbar": 1, "d": 2, "T1": 3, "T2": 4}, IETF: {"Bbar": 1, "T": 2}}
RESP_OF = {CDL: {"z1": 0, "z2": 1, "z3": 2}, IETF: {"z_a": 0, "z_b": 1}}
BOTH = [CDL, IETF]


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


def mask_of(i, L):
    kind = i % 6
    if kind == 0:
        return [1 if (i * 7 + j * j + j // 3) % 3 == 0 else 0 for j in range(L)]
    return {1: [0] * L, 2: [1] * L, 3: [1] + [0] * (L - 1), 4: [0] * (L - 1) + [1], 5: [j & 1 for j in range(L)]}[kind]


class Scenario:
    def __init__(self):
        rng = np.random.default_rng(2023)
        x, gamma = rand(rng, 2)
        self.key = M.Key(x, gamma, rand(rng, 32))
        self.e, self.r1, self.r2, self.r, self.c = (rand(rng, N) for _ in range(5))
        self.msgs = [rand(rng, 32) for _ in range(N)]
        self.blind = [rand(rng, 3 + 32) for _ in range(N)]
        self.e[3] = 0
        self.msgs[4][0], self.msgs[5][0], self.msgs[6] = 0, R - 1, [R - 1] * 32
        self.c[9], self.c[10], self.r1[N - 1] = 0, R - 1, 0
        self.g2 = O.G2.generator()
        self.w = O.G2.to_affine(O.G2.mul(self.g2, O.int_to_limbs(x, 4)))[0]
        self._proofs, self._pts, self._params, self._sigs, self._big = {}, {}, {}, {}, {}

    def prove(self, kind, L, i, a=None, r1=None):
        e, m = self.e[i], self.msgs[i][:L]
        a = self.key.a(e, m) if a is None else a
        assert a is not None
        mask = mask_of(i, L)
        rev = {j for j in range(L) if mask[j]}
        if kind == CDL:
            return M.prove_cdl(self.key, a, e, m, rev, self.r1[i] if r1 is None else r1, self.r2[i], self.blind[i], self.c[i])
        return M.prove_ietf(self.key, a, e, m, rev, self.r[i], self.blind[i], self.c[i])

    def proofs(self, kind, L):
        if (kind, L) not in self._proofs:
            self._proofs[kind, L] = [self.prove(kind, L, i) for i in range(N)]
        return self._proofs[kind, L]

    def points(self, kind, L):
        """the points of the scenario's proofs for L messages per row, (257, 5 | 3, 12) ABI words"""
        if (kind, L) not in self._pts:
            self._pts[kind, L] = g_times([k for p in self.proofs(kind, L) for k in p.pts]).reshape(N, NPTS[kind], 12)
        return self._pts[kind, L]

    def want(self, kind, L, n):
        return [p.status(self.key) for p in self.proofs(kind, L)[:n]]

    def sig_logs(self, L):
        return [self.key.a(self.e[i], self.msgs[i][:L]) for i in range(N)]

    def sigs(self, L):
        if L not in self._sigs:
            self._sigs[L] = g_times(self.sig_logs(L))
        return self._sigs[L]

    def param_points(self, L):
        if L not in self._params:
            self._params[L] = g_times(self.key.params_scalars(L))
        return self._params[L]

    def params(self, L):
        p = self.param_points(L)
        return B23.Params23(p[0], p[1:], self.g2, self.w)

    def big(self, kind):
        """4097 valid proofs of one message: the scenario's rows over and over with a blinding factor of their own (so no two rows hold the same points)"""
        if kind not in self._big:
            proofs = []
            for i in range(NBIG):
                k = i % N
                e, m = self.e[k], self.msgs[k][:1]
                rev = {0} if mask_of(k, 1)[0] else set()
                if kind == CDL:
                    proofs.append(M.prove_cdl(self.key, self.key.a(e, m), e, m, rev, (self.r1[k] + i) % R or 1, self.r2[k], self.blind[k], self.c[k]))
                else:
                    proofs.append(M.prove_ietf(self.key, self.key.a(e, m), e, m, rev, (self.r[k] + i) % R or 1, self.blind[k], self.c[k]))
            self._big[kind] = (proofs, g_times([q for p in proofs for q in p.pts]).reshape(NBIG, NPTS[kind], 12))
        return self._big[kind]

    def tampered(self, kind, L, n, plan):
        """(proofs, points) of the first n rows with the tamper plan[i] applied to row i; the changed points are k G again for the changed k"""
        proofs, pts = [p.copy() for p in self.proofs(kind, L)[:n]], self.points(kind, L)[:n].copy()
        for i, t in plan.items():
            proofs[i] = tamper(self, kind, L, i, proofs[i], t)
        rows = sorted(plan)
        if rows:
            pts[rows] = g_times([k for i in rows for k in proofs[i].pts]).reshape(len(rows), NPTS[kind], 12)
        return proofs, pts


def tamper(S, kind, L, i, p, t):
    if t.startswith("forged"):
        p = S.prove(kind, L, i, a=(S.key.a(S.e[i], S.msgs[i][:L]) + 1) % R)
        t = t[len("forged_and_"):]
    bump = lambda lst, k: lst.__setitem__(k, (lst[k] + 1) % R)
    if t in POINT_OF[kind]:
        bump(p.pts, POINT_OF[kind][t])
    elif t in RESP_OF[kind]:
        bump(p.fixed, RESP_OF[kind][t])
    elif t == "c":
        p.c = (p.c + 1) % R
    elif t == "hidden":
        bump(p.values, p.mask.index(0))
    elif t == "revealed":
        bump(p.values, p.mask.index(1))
    elif t == "mask":
        p.mask[0] ^= 1
    elif t == "A_identity":
        p.pts[0] = 0
    elif t.endswith("_identity"):
        p.pts[POINT_OF[kind][t[:-len("_identity")]]] = 0
    else:
        assert t == "", t
    return p


def mixed_rows(S, kind, L, n):
    """the rows whose masks hide some messages and reveal others (a tamper of either kind finds its entry) and whose challenge is not zero (c m hides a change of
    a revealed m where c = 0)"""
    return [i for i, p in enumerate(S.proofs(kind, L)[:n]) if 0 < sum(p.mask) < L and p.c != 0 and p.pts[0] != 0]


def pack(proofs, f=limbs):
    n, L, nresp = len(proofs), len(proofs[0].values), len(proofs[0].fixed)
    return (f([z for p in proofs for z in p.fixed]).reshape(n, nresp, 4), f([v for p in proofs for v in p.values]).reshape(n, L, 4),
            np.array([p.mask for p in proofs], np.uint8).reshape(n, L), f([p.c for p in proofs]))


EACH = {CDL: B23.pok_verify_each, IETF: B23.pok_ietf_verify_each}
BATCH = {CDL: B23.pok_verify_batch, IETF: B23.pok_ietf_verify_batch}


def each(P, proofs, pts, montgomery=False):
    fixed, values, mask, c = pack(proofs, mont if montgomery else limbs)
    return EACH[proofs[0].kind](P, pts, fixed, values, mask, c, montgomery=montgomery).tolist()


def each_both_forms(P, proofs, pts):
    st = each(P, proofs, pts)
    assert st == each(P, proofs, pts, montgomery=True)
    return st


def batch(P, proofs, pts, rho, montgomery=False):
    f = mont if montgomery else limbs
    fixed, values, mask, c = pack(proofs, f)
    return BATCH[proofs[0].kind](P, pts, fixed, values, mask, c, f([rho])[0], montgomery=montgomery)


def batch_both_forms(P, proofs, pts, rho):
    ok = batch(P, proofs, pts, rho)
    assert ok == batch(P, proofs, pts, rho, montgomery=True)
    return ok


_S = []


def scenario():
    if not _S:
        _S.append(Scenario())
    return _S[0]


# ---- signatures --------------------------------------------------------------------------------------------------------------------------------------------
def msgs_of(S, L, n, f=limbs):
    return f([v for i in range(n) for v in S.msgs[i][:L]]).reshape(n, L, 4)


@pytest.mark.parametrize("L", LS)
def test_sign_many_against_the_model(L):
    """A_i = a_i G limb for limb for every shape and both input forms; then every signature verifies, one by one and as a batch"""
    S = scenario()
    want = S.sigs(L)
    with S.params(L) as P:
        for n in NS:
            for f, mg in ((limbs, False), (mont, True)):
                A, bad = B23.sign_many(P, f([S.key.x])[0], msgs_of(S, L, n, f), f(S.e[:n]), montgomery=mg)
                assert not bad.any() and (A == want[:n]).all(), (n, mg)
                assert B23.verify_each(P, A, f(S.e[:n]), msgs_of(S, L, n, f), montgomery=mg).tolist() == [1] * n, (n, mg)
                assert B23.verify_batch(P, A, f(S.e[:n]), msgs_of(S, L, n, f), f([RHO])[0], montgomery=mg), (n, mg)
        assert B23.verify_batch(P, want[:65], S.e[:65], [m[:L] for m in S.msgs[:65]], 1) and B23.verify_batch(P, want[:65], limbs(S.e[:65]), msgs_of(S, L, 65), R - 1)


@pytest.mark.parametrize("L", [1, 30])
def test_rows_without_a_signature_are_flagged_and_their_neighbours_intact(L):
    """x + e = 0 at rows 1 and 63, b = O at row 32 (the first message solves g1 + sum m_j h_j = O): bad = 1 and zero words there, every other row as the model"""
    S = scenario()
    n = 65
    es, msgs = list(S.e[:n]), [list(m[:L]) for m in S.msgs[:n]]
    es[1] = es[63] = (R - S.key.x) % R
    H = S.key.params_scalars(L)
    msgs[32][0] = (-(H[0] + sum(m * h for m, h in zip(msgs[32][1:], H[2:]))) * M.inv(H[1])) % R
    assert S.key.b(msgs[32]) == 0
    logs = [S.key.a(e, m) for e, m in zip(es, msgs)]
    assert [i for i, a in enumerate(logs) if a is None] == [1, 32, 63]
    want = g_times([a or 0 for a in logs])
    with S.params(L) as P:
        for f, mg in ((limbs, False), (mont, True)):
            A, bad = B23.sign_many(P, f([S.key.x])[0], f([v for m in msgs for v in m]).reshape(n, L, 4), f(es), montgomery=mg)
            assert bad.tolist() == [1 if a is None else 0 for a in logs] and (A == want).all()
            ok = B23.verify_each(P, A, f(es), f([v for m in msgs for v in m]).reshape(n, L, 4), montgomery=mg).tolist()
            assert ok == [0 if a is None else 1 for a in logs]                      # an identity A is ZeroSignature
            assert not B23.verify_batch(P, A, f(es), f([v for m in msgs for v in m]).reshape(n, L, 4), f([RHO])[0], montgomery=mg)


@pytest.mark.parametrize("L", [2, 31])
def test_verify_each_is_the_complement_of_planted_faults_and_a_compensating_pair(L):
    S = scenario()
    n = 65
    logs, es, msgs = S.sig_logs(L)[:n], list(S.e[:n]), [list(m[:L]) for m in S.msgs[:n]]
    logs[0] += 1; es[15] = (es[15] + 1) % R; msgs[16][0] = (msgs[16][0] + 1) % R; msgs[33][L - 1] = (msgs[33][L - 1] + 1) % R; logs[64] = 0; logs[40] = R - logs[40]
    faults = {0, 15, 16, 33, 40, 64}
    want = [1 if S.key.verifies(a, e, m) else 0 for a, e, m in zip(logs, es, msgs)]
    assert want == [0 if i in faults else 1 for i in range(n)]
    A = S.sigs(L)[:n].copy()
    A[sorted(faults)] = g_times([logs[i] for i in sorted(faults)])
    with S.params(L) as P:
        for f, mg in ((limbs, False), (mont, True)):
            m_ = f([v for m in msgs for v in m]).reshape(n, L, 4)
            assert B23.verify_each(P, A, f(es), m_, montgomery=mg).tolist() == want
            assert not B23.verify_batch(P, A, f(es), m_, f([RHO])[0], montgomery=mg)
        # one fault alone, at either end: the batch refuses
        for i in (0, n - 1):
            B = S.sigs(L)[:n].copy()
            B[i] = g_times([S.sig_logs(L)[i] + 1])[0]
            assert not B23.verify_batch(P, B, S.e[:n], [m[:L] for m in S.msgs[:n]], RHO)
        # m_i0 += X, m_j0 -= X: with rho = 1 the column sum is unchanged and the two errors cancel; rho = 2 weighs them apart; the per-row verdicts see both
        i, j, X = 7, 41, 0x123456789
        msgs = [list(m[:L]) for m in S.msgs[:n]]
        msgs[i][0], msgs[j][0] = (msgs[i][0] + X) % R, (msgs[j][0] - X) % R
        sigs = S.sig_logs(L)[:n]
        assert S.key.batch_verifies(sigs, S.e[:n], msgs, 1) and not S.key.batch_verifies(sigs, S.e[:n], msgs, 2)
        A = S.sigs(L)[:n]
        for f, mg in ((limbs, False), (mont, True)):
            m_ = f([v for m in msgs for v in m]).reshape(n, L, 4)
            assert B23.verify_batch(P, A, f(S.e[:n]), m_, f([1])[0], montgomery=mg) and not B23.verify_batch(P, A, f(S.e[:n]), m_, f([2])[0], montgomery=mg)
            assert B23.verify_each(P, A, f(S.e[:n]), m_, montgomery=mg).tolist() == [0 if k in (i, j) else 1 for k in range(n)]


# ---- proofs of knowledge -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("kind", BOTH)
def test_the_scenarios_proofs_every_shape_and_both_forms(kind, L):
    """the model's status for every row — 0 but for the CDL row with r1 = 0 — and one verdict; all-hidden and all-revealed rows, c = 0, c = r - 1, e = 0 and
    messages 0 and r - 1 among them"""
    S = scenario()
    proofs, pts = S.proofs(kind, L), S.points(kind, L)
    assert {tuple(p.mask) for p in proofs[:9]} >= {tuple([0] * L), tuple([1] * L)}
    want = S.want(kind, L, N)
    assert want == [0] * (N - 1) + [1 if kind == CDL else 0] and (kind == IETF or not pts[N - 1][0].any())
    with S.params(L) as P:
        for n in NS:
            assert each_both_forms(P, proofs[:n], pts[:n]) == want[:n], n
            assert batch_both_forms(P, proofs[:n], pts[:n], RHO) == (not any(want[:n])), n
        assert batch(P, proofs[:65], pts[:65], 1) and batch(P, proofs[:65], pts[:65], R - 1)


@pytest.mark.parametrize("kind", BOTH)
def test_a_strided_view_of_the_values_reads_nothing_between_the_rows(kind):
    S = scenario()
    L, n = 30, 65
    proofs, pts = S.proofs(kind, L)[:n], S.points(kind, L)[:n]
    fixed, values, mask, c = pack(proofs)
    wide = np.full((n, L + 3, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    wide[:, :L] = values
    with S.params(L) as P:
        assert EACH[kind](P, pts, fixed, wide[:, :L], mask, c).tolist() == [0] * n
        assert BATCH[kind](P, pts, fixed, wide[:, :L], mask, c, RHO)
        if kind == CDL:
            msgs = np.full((n, L + 3, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
            msgs[:, :L] = msgs_of(S, L, n)
            A, bad = B23.sign_many(P, S.key.x, msgs[:, :L], S.e[:n])
            assert not bad.any() and (A == S.sigs(L)[:n]).all()
            assert B23.verify_each(P, A, S.e[:n], msgs[:, :L]).all() and B23.verify_batch(P, A, S.e[:n], msgs[:, :L], RHO)


@pytest.mark.parametrize("kind", BOTH)
def test_every_tamper_kind_in_one_call(kind):
    """257 proofs of 31 messages, every kind at the first row or a row between: the status is the reference's first error, the neighbours verify"""
    S = scenario()
    L, n = 31, N
    both = mixed_rows(S, kind, L, n)
    assert both[0] == 0
    plan = dict(zip(both, KINDS[kind]))
    free = [i for i in (19, 25, 37, 43) if i not in plan]
    plan.update({7: "hidden", 8: "revealed"})                                        # (7: everything hidden; 8: everything revealed)
    plan.update(dict(zip(free, IDENTITIES[kind])))
    proofs, pts = S.tampered(kind, L, n, plan)
    want = [p.status(S.key) for p in proofs]
    for i, t in plan.items():
        assert want[i] == {**KINDS[kind], **IDENTITIES[kind]}[t], (i, t)
    assert sum(1 for v in want[:N - 1] if v) == len(plan) and (kind == CDL or 2 not in want)
    with S.params(L) as P:
        assert each_both_forms(P, proofs, pts) == want
        assert not batch(P, proofs[:N - 1], pts[:N - 1], RHO)


@pytest.mark.parametrize("kind", BOTH)
def test_tampers_around_forced_chunk_borders(twin, kind):
    """sixteen rows per chunk through the development surface, 65 rows of 30 messages: one kind per call at the first row, on both sides of a border and at the
    last row; the batch call, cut the same way, refuses each.  The signature calls are cut by the same knob"""
    S = scenario()
    L, n = 30, 65
    with S.params(L) as P:
        try:
            assert twin.dgpu_set_many_chunk_rows(16) == 0
            assert each_both_forms(P, S.proofs(kind, L)[:n], S.points(kind, L)[:n]) == [0] * n
            assert batch(P, S.proofs(kind, L)[:n], S.points(kind, L)[:n], RHO)
            for k, t in enumerate(list(KINDS[kind]) + list(IDENTITIES[kind])):
                b = 16 if k % 2 == 0 else 48                                # (rows 0, 15, 16, 47, 48, 64 hide some messages and reveal others)
                plan = {i: t for i in (0, b - 1, b, 64)}
                proofs, pts = S.tampered(kind, L, n, plan)
                want = [p.status(S.key) for p in proofs]
                assert all(want[i] == {**KINDS[kind], **IDENTITIES[kind]}[t] for i in plan), t
                assert each(P, proofs, pts) == want, t
                assert not batch(P, proofs, pts, RHO), t
            if kind == CDL:
                A, bad = B23.sign_many(P, S.key.x, msgs_of(S, L, n), S.e[:n])
                assert not bad.any() and (A == S.sigs(L)[:n]).all()
                for i in (0, 15, 16, 64):
                    B = A.copy()
                    B[i] = S.sigs(L)[(i + 1) % n]
                    assert B23.verify_each(P, B, S.e[:n], msgs_of(S, L, n)).tolist() == [0 if k == i else 1 for k in range(n)]
                    assert not B23.verify_batch(P, B, S.e[:n], msgs_of(S, L, n), RHO)
                assert B23.verify_batch(P, A, S.e[:n], msgs_of(S, L, n), RHO)
        finally:
            twin.dgpu_set_many_chunk_rows(0)


@pytest.mark.parametrize("L", [2, 30])
@pytest.mark.parametrize("kind", BOTH)
def test_batch_single_tampers_and_a_cancelling_pair(kind, L):
    S = scenario()
    n = 65
    t_idx = 3 if kind == CDL else 2                                               # T1, respectively T: weighed by u_i alone
    with S.params(L) as P:
        for t in list(KINDS[kind]) + list(IDENTITIES[kind]):
            for i in (0, 34, n - 1):                                       # (34 = 4 mod 6: only the last message revealed)
                p = S.proofs(kind, L)[i]
                if (t == "hidden" and 0 not in p.mask) or (t == "revealed" and (1 not in p.mask or p.c == 0)):
                    continue
                proofs, pts = S.tampered(kind, L, n, {i: t})
                assert not M.batch_verdict(S.key, proofs, RHO)
                assert not batch(P, proofs, pts, RHO), (t, i)
        # T_i += X, T_j -= X: with every u_i one (CDL: rho = r - 1; IETF: rho = 1) the two errors cancel; rho = 2 weighs them apart; the per-proof verdicts see both
        i, j, X = 7, 41, 0x123456789
        unit = R - 1 if kind == CDL else 1
        proofs = [p.copy() for p in S.proofs(kind, L)[:n]]
        pts = S.points(kind, L)[:n].copy()
        proofs[i].pts[t_idx], proofs[j].pts[t_idx] = (proofs[i].pts[t_idx] + X) % R, (proofs[j].pts[t_idx] - X) % R
        pts[[i, j]] = g_times(proofs[i].pts + proofs[j].pts).reshape(2, NPTS[kind], 12)
        assert M.batch_verdict(S.key, proofs, unit) and not M.batch_verdict(S.key, proofs, 2)
        assert batch_both_forms(P, proofs, pts, unit) and not batch_both_forms(P, proofs, pts, 2)
        assert each(P, proofs, pts) == [(2 if kind == CDL else 3) if k in (i, j) else 0 for k in range(n)]
        # one proof: the batch is the proof's own verdict
        for k in (0, 5):
            assert batch(P, proofs[k:k + 1], pts[k:k + 1], RHO) and each(P, proofs[k:k + 1], pts[k:k + 1]) == [0]
        assert not batch(P, proofs[7:8], pts[7:8], RHO) and each(P, proofs[7:8], pts[7:8]) == [2 if kind == CDL else 3]


@pytest.mark.parametrize("n", [4095, 4096, 4097])
@pytest.mark.parametrize("kind", BOTH)
def test_proofs_at_the_chunk_size(kind, n):
    """L = 1, one row below, at and above the 4096 rows of a chunk: every row verifies, and tampers at the ends and on both sides of the border are the only
    other statuses; the batch call sees them too"""
    S = scenario()
    proofs, pts = S.big(kind)
    with S.params(1) as P:
        assert each(P, proofs[:n], pts[:n]) == [0] * n
        assert batch(P, proofs[:n], pts[:n], RHO)
        kinds = ["T1", "z3", "forged", "A_identity", "c", "T2"] if kind == CDL else ["T", "z_a", "forged", "A_identity", "c", "Bbar"]
        plan = {i: kinds[(i + n) % 6] for i in sorted({0, n - 1, 4094, min(4095, n - 1)})}
        bad, bpts = [p.copy() for p in proofs[:n]], pts[:n].copy()
        for i, t in plan.items():
            if t == "forged":
                k = i % N
                e, m = S.e[k], S.msgs[k][:1]
                rev = {0} if mask_of(k, 1)[0] else set()
                a = (S.key.a(e, m) + 1) % R
                bad[i] = M.prove_cdl(S.key, a, e, m, rev, (S.r1[k] + i) % R or 1, S.r2[k], S.blind[k], S.c[k]) if kind == CDL else \
                    M.prove_ietf(S.key, a, e, m, rev, (S.r[k] + i) % R or 1, S.blind[k], S.c[k])
            else:
                bad[i] = tamper(S, kind, 1, i % N, bad[i], t)
        bpts[sorted(plan)] = g_times([k for i in sorted(plan) for k in bad[i].pts]).reshape(len(plan), NPTS[kind], 12)
        want = [p.status(S.key) for p in bad]
        assert all(want[i] == KINDS[kind][t] for i, t in plan.items()) and sum(1 for v in want if v) == len(plan)
        assert each(P, bad, bpts) == want
        assert not batch(P, bad, bpts, RHO)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_signatures_at_the_chunk_size(n):
    """L = 1: sign n rows against the model at the ends and on both sides of the border, verify them all, then plant faults at those rows"""
    S = scenario()
    es = [(S.e[i % N] + i) % R for i in range(n)]
    msgs = [[(S.msgs[i % N][0] + 3 * i) % R] for i in range(n)]
    rows = sorted({0, n - 1, 4094, min(4095, n - 1)})
    with S.params(1) as P:
        A, bad = B23.sign_many(P, S.key.x, msgs, es)
        assert not bad.any() and (A[rows] == g_times([S.key.a(es[i], msgs[i]) for i in rows])).all()
        assert B23.verify_each(P, A, es, msgs).tolist() == [1] * n and B23.verify_batch(P, A, es, msgs, RHO)
        B = A.copy()
        B[rows] = g_times([S.key.a(es[i], msgs[i]) + 1 for i in rows])
        assert B23.verify_each(P, B, es, msgs).tolist() == [0 if i in rows else 1 for i in range(n)] and not B23.verify_batch(P, B, es, msgs, RHO)


def test_rows_longer_than_the_many_row_kernels_accept():
    """L + 1 = 31 above a lowered dgpu_set_small_msm_max: the single-row driver inside the calls gives the same bytes"""
    S = scenario()
    L, n = 30, 9
    with S.params(L) as P:
        try:
            assert lib().dgpu_set_small_msm_max(8) == 0
            for kind in BOTH:
                proofs, pts = S.tampered(kind, L, n, {4: "T2" if kind == CDL else "T", 6: "forged"})
                assert each(P, proofs, pts) == [0, 0, 0, 0, 3, 0, 4, 0, 0]
                assert not batch(P, proofs, pts, RHO) and batch(P, S.proofs(kind, L)[:n], S.points(kind, L)[:n], RHO)
            A, bad = B23.sign_many(P, S.key.x, msgs_of(S, L, n), S.e[:n])
            assert not bad.any() and (A == S.sigs(L)[:n]).all()
            A[5] = S.sigs(L)[6]
            assert B23.verify_each(P, A, S.e[:n], msgs_of(S, L, n)).tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 1] and not B23.verify_batch(P, A, S.e[:n], msgs_of(S, L, n), RHO)
            assert B23.verify_batch(P, S.sigs(L)[:n], S.e[:n], msgs_of(S, L, n), RHO)
        finally:
            lib().dgpu_set_small_msm_max(8192)


def test_a_second_call_of_a_shape_allocates_nothing():
    """eight rows of two messages: after one warming call of each of the seven calls (it readies the context's idle slots too) a second identical call leaves
    dgpu_device_alloc_count where it was"""
    S = scenario()
    L, n = 2, 8
    A, e, m = S.sigs(L)[:n], limbs(S.e[:n]), msgs_of(S, L, n)
    with S.params(L) as P:
        calls = [("sign_many", lambda: B23.sign_many(P, S.key.x, m, e)[0].tolist(), A.tolist()),
                 ("verify_each", lambda: B23.verify_each(P, A, e, m).tolist(), [1] * n), ("verify_batch", lambda: B23.verify_batch(P, A, e, m, RHO), True)]
        for kind in BOTH:
            proofs, pts = S.proofs(kind, L)[:n], S.points(kind, L)[:n]
            calls += [("each %d" % kind, lambda proofs=proofs, pts=pts: each(P, proofs, pts), [0] * n),
                      ("batch %d" % kind, lambda proofs=proofs, pts=pts: batch(P, proofs, pts, RHO), True)]
        for name, call, want in calls:
            assert call() == want, name
            before = lib().dgpu_device_alloc_count()
            got = call()
            assert lib().dgpu_device_alloc_count() == before, name
            assert got == want, name


def test_four_threads_at_once_give_the_same_bytes():
    S = scenario()
    L = 30
    jobs = []
    for k in range(4):
        n, kind = 62 + k, BOTH[k & 1]
        t = "T1" if kind == CDL else "T"
        proofs, pts = S.tampered(kind, L, n, {k: t, 30 + k: "z2" if kind == CDL else "z_b", n - 1: "forged"})
        jobs.append((kind, proofs, pts, [p.status(S.key) for p in proofs]))
    with S.params(L) as P:
        def work(k):
            kind, proofs, pts, want = jobs[k % 4]
            n = len(proofs)
            A, bad = B23.sign_many(P, S.key.x, msgs_of(S, L, n), S.e[:n])
            return each(P, proofs, pts) == want and not batch(P, proofs, pts, 77 + k) and batch(P, S.proofs(kind, L)[:n], S.points(kind, L)[:n], 77 + k) and \
                each(P, S.proofs(kind, L)[:n], S.points(kind, L)[:n]) == [0] * n and not bad.any() and (A == S.sigs(L)[:n]).all() and \
                B23.verify_each(P, A, S.e[:n], msgs_of(S, L, n)).all() and B23.verify_batch(P, A, S.e[:n], msgs_of(S, L, n), 77 + k)
        with ThreadPoolExecutor(4) as ex:
            assert all(ex.map(work, range(8)))


def test_handles_the_calls_refuse():
    """a handle of another length (MessageCountIncompatibleWithSigParams), a precomputed one, no handle at all: DGPU_E_BADARG from all seven calls"""
    S = scenario()
    with S.params(2) as P:
        pre = DeviceBases(CG1, S.param_points(2)); pre.precompute(16)
        for handle, L in ((P.handle, 1), (P.handle, 3), (pre.handle, 2), (0xDEADBEEF, 2)):
            class Q:
                pass
            q = Q(); q.handle, q.L, q.pk_pc, q.g2_pc = handle, L, P.pk_pc, P.g2_pc
            e, m, A = S.e[:3], msgs_of(S, L, 3), S.sigs(L)[:3]
            calls = [lambda: B23.sign_many(q, S.key.x, m, e), lambda: B23.verify_each(q, A, e, m), lambda: B23.verify_batch(q, A, e, m, 5)]
            for kind in BOTH:
                proofs, pts = S.proofs(kind, L)[:3], S.points(kind, L)[:3]
                calls += [lambda proofs=proofs, pts=pts: each(q, proofs, pts), lambda proofs=proofs, pts=pts: batch(q, proofs, pts, 5)]
            assert len(calls) == 7
            for call in calls:
                with pytest.raises(ca.DockGpuError) as err:
                    call()
                assert err.value.code == -3, (handle, L)
        pre.free()


def neg_point(pt):
    """-P on affine Montgomery words: y -> p - y"""
    out = pt.copy()
    if pt.any():
        y = P_MOD - sum(int(w) << (64 * k) for k, w in enumerate(pt[6:]))
        out[6:] = [(y >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]
    return out


@pytest.mark.parametrize("kind", BOTH)
def test_the_composed_chain_of_public_calls_gives_the_same_statuses(kind):
    """n = 65, L = 30: P_i from dgpu_msm_g1_handle_many on the model's rows, the segment sums from dgpu_msm_g1_segments over the proofs' own points, the pairings
    from dgpu_multi_pairing_segments — the caller's chain, with its host scalar work — equal the fused call on rows with planted tampers"""
    S = scenario()
    L, n = 30, 65
    one = O.fp12_one()
    tampers = list(KINDS[kind]) + list(IDENTITIES[kind])
    proofs, pts = S.tampered(kind, L, n, dict(zip(mixed_rows(S, kind, L, n), tampers)))
    segs, own = (2, 6) if kind == CDL else (1, 3)
    order = [0, 2, 1, 3, 2, 4] if kind == CDL else [0, 1, 2]
    with S.params(L) as P:
        got = each(P, proofs, pts)
        rows = limbs([v for p in proofs for v in p.row()]).reshape(n, L + 1, 4)
        pj, pinf = P.bases.msm_many(rows, flags=True)
        bases = np.stack([pts[i][q] for i in range(n) for q in order])
        ends = [v for i in range(n) for v in ((own * i + 4, own * i + 6) if kind == CDL else (own * i + 3,))]
        sj, sinf = msm_segments(CG1, bases, limbs([v for p in proofs for v in p.own()]), ends, flags=True)
        gts = multi_pairings([(np.stack([pts[i][0], neg_point(pts[i][1])]), np.stack([S.w, S.g2])) for i in range(n)])
        chain = []
        for i in range(n):
            q = segs * i + segs - 1
            second = bool(pinf[i]) and bool(sinf[q]) if pinf[i] or sinf[q] else (neg_point(G.to_affine(pj[i])[0]) == G.to_affine(sj[q])[0]).all()
            first = bool(sinf[2 * i]) if kind == CDL else True
            chain.append(1 if not pts[i][0].any() else 2 if not first else 3 if not second else 4 if not (gts[i] == one).all() else 0)
        assert chain == got == [p.status(S.key) for p in proofs]
        assert sorted(set(got)) == ([0, 1, 2, 3, 4] if kind == CDL else [0, 1, 3, 4])
