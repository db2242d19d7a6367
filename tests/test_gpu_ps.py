"""GPU (-m gpu): the four dgpu_ps_* calls (crypto_amd/csrc/dock_ps.hip, ps_kernels.hip.h, and the G2 form of msm_many.hip.h's RowMsm and pair_check.hip.h's
affine-first-side check) through crypto_amd.ps.  The key, the signatures and the proofs come from known discrete logs (tests/ps_model.py) through the oracle's G1 /
G2 scalar multiplication, so every point is k G or k G2 for a k the model computes and every expected byte is decided in the exponent (tests/test_ps_model.py pins
the model against the oracle's own MSM and pairing).  Every comparison is exact.  One scenario of 257 rows of up to 32 messages is built once; every shape is a
prefix of it.  The G2 points of the proofs (a millisecond each on the oracle) exist for all 257 rows at L = 2, 30, 32 and for 11 rows at the other L.  Edge rows:
messages 0 and r - 1 (4, 5, 6), c = 0 (9), c = r - 1 (10), all-hidden (i = 1 mod 6) and all-revealed (2 mod 6) masks."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import ps_model as M
import crypto_amd as ca
from crypto_amd import ps as PS
from crypto_amd import G1 as CG1, G2 as CG2
from crypto_amd.msm import DeviceBases
from crypto_amd.pairing import multi_pairings
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu
R = M.R
R2 = pow(2, 256, R)
P_MOD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
N = 257
NS = [1, 2, 9, 63, 64, 65, 257]
LS = [1, 2, 3, 15, 30, 31, 32]           # rows of L + 1 and L + 2 terms on both sides of every segment size of many_geometry (2, 4, 8, 16, 32 per group; 33 and 34: three leaves)
FULL = (2, 30, 32)                       # the L whose proofs have G2 points for all 257 rows
FEW = 11
LMAX = 32
RHO = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
# tamper kinds and the status the reference's order of errors (3 over 1 over 4) gives each; "mask" is decided by the model (3 or 4)
KINDS = {"t": 3, "k": 3, "hidden": 3, "z_r": 3, "c": 3, "revealed": 4, "mask": None, "s1_identity": 1, "s2_identity": 1, "forged": 4, "forged_and_t": 3, "s1_identity_and_t": 3,
         "t_identity": 3, "k_identity": 3}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)
    yield


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def mont(vals):
    return limbs([v * R2 % R for v in vals])


FORMS = ((limbs, False), (mont, True))


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def g1_times(scalars):
    """k G as affine ABI words (k = 0: zero words), on the oracle's host threads"""
    scalars = [k % R for k in scalars]
    out, inf = O.g1_scale_batch(np.tile(O.G1.generator(), (len(scalars), 1)), limbs(scalars), threads=16)
    out[inf.astype(bool)] = 0
    return out


def g2_times(scalars):
    """k G2 as affine ABI words (k = 0: zero words) by the oracle's scalar multiplication"""
    g = O.G2.generator()
    return np.stack([np.zeros(24, np.uint64) if k % R == 0 else O.G2.to_affine(O.G2.mul(g, O.int_to_limbs(k % R, 4)))[0] for k in scalars])


def mask_of(i, L):
    kind = i % 6
    if kind == 0:
        return [1 if (i * 7 + j * j + j // 3) % 3 == 0 else 0 for j in range(L)]
    return {1: [0] * L, 2: [1] * L, 3: [1] + [0] * (L - 1), 4: [0] * (L - 1) + [1], 5: [j & 1 for j in range(L)]}[kind]


class Scenario:
    def __init__(self, lmax=LMAX, rows=N, seed=2024):
        rng = np.random.default_rng(seed)
        x, gamma, gamma_t = rand(rng, 3)
        self.lmax, self.rows = lmax, rows
        self.key = M.Key(x, rand(rng, lmax), gamma, gamma_t)
        self.rs, self.rp, self.rbar, self.c = (rand(rng, rows) for _ in range(4))
        self.msgs = [rand(rng, lmax) for _ in range(rows)]
        self.blind = [rand(rng, lmax + 1) for _ in range(rows)]
        if rows > 10:
            self.msgs[4][0], self.msgs[5][0], self.msgs[6] = 0, R - 1, [R - 1] * lmax
            self.c[9], self.c[10] = 0, R - 1
        self.g = g1_times([gamma])[0]
        self.pk = g2_times(self.key.pk_scalars(lmax))                         # alpha_tilde, beta_tilde_1 .. beta_tilde_lmax, g_tilde
        self._sigs, self._proofs, self._pts = {}, {}, {}

    def params(self, L):
        return PS.PsParams(self.g, self.pk[self.lmax + 1], self.pk[0], self.pk[1:L + 1])

    def sig_logs(self, L):
        return [self.key.sign(self.rs[i], self.msgs[i][:L]) for i in range(self.rows)]

    def sigs(self, L):
        if L not in self._sigs:
            self._sigs[L] = g1_times([v for s in self.sig_logs(L) for v in s]).reshape(self.rows, 2, 12)
        return self._sigs[L]

    def prove(self, L, i, forge=0):
        s1, s2 = self.key.sign(self.rs[i], self.msgs[i][:L])
        mask = mask_of(i, L)
        return M.prove(self.key, (s1, s2 + forge), self.msgs[i][:L], {j for j in range(L) if mask[j]}, self.rp[i], self.rbar[i], self.blind[i][:L] + [self.blind[i][self.lmax]],
                       self.c[i])

    def count(self, L):
        return self.rows if L in FULL or self.rows < FEW else FEW

    def proofs(self, L):
        if L not in self._proofs:
            self._proofs[L] = [self.prove(L, i) for i in range(self.count(L))]
        return self._proofs[L]

    def points(self, L):
        """(sigs (n, 2, 12), g2_points (n, 2, 24)) of the scenario's proofs for L messages per row"""
        if L not in self._pts:
            self._pts[L] = points_of(self.proofs(L))
        return self._pts[L]

    def tampered(self, L, n, plan):
        """(proofs, sigs, g2_points) of the first n rows with the tamper plan[i] applied to row i; the changed points are multiples of the generators again"""
        proofs = [p.copy() for p in self.proofs(L)[:n]]
        sg, pts = (a[:n].copy() for a in self.points(L))
        for i, t in plan.items():
            proofs[i] = tamper(self, L, i, proofs[i], t)
        rows = sorted(plan)
        if rows:
            sg[rows], pts[rows] = points_of([proofs[i] for i in rows])
        return proofs, sg, pts


def points_of(proofs):
    n = len(proofs)
    return g1_times([v for p in proofs for v in p.sig]).reshape(n, 2, 12), g2_times([v for p in proofs for v in (p.k, p.t)]).reshape(n, 2, 24)


def tamper(S, L, i, p, t):
    if t.startswith("forged"):
        p = S.prove(L, i, forge=1)
        t = t[len("forged_and_"):]
    if t.startswith("s1_identity"):
        p.sig[0] = 0
        t = t[len("s1_identity_and_"):]
    if t in ("t", "k", "z_r", "c"):
        setattr(p, t, (getattr(p, t) + 1) % R)
    elif t == "hidden":
        k = p.mask.index(0); p.values[k] = (p.values[k] + 1) % R
    elif t == "revealed":
        k = p.mask.index(1); p.values[k] = (p.values[k] + 1) % R
    elif t == "mask":
        p.mask[0] ^= 1
    elif t == "s2_identity":
        p.sig[1] = 0
    elif t == "t_identity":
        p.t = 0
    elif t == "k_identity":
        p.k = 0
    else:
        assert t == "", t
    return p


def mixed_rows(S, L, n):
    """the rows whose masks hide some messages and reveal others (a tamper of either kind finds its entry) and whose challenge is not zero"""
    return [i for i, p in enumerate(S.proofs(L)[:n]) if 0 < sum(p.mask) < L and p.c != 0]


def pack(proofs, f=limbs):
    n, L = len(proofs), len(proofs[0].values)
    return f([p.z_r for p in proofs]), f([v for p in proofs for v in p.values]).reshape(n, L, 4), np.array([p.mask for p in proofs], np.uint8).reshape(n, L), f([p.c for p in proofs])


def each(P, proofs, sg, pts, montgomery=False):
    z, values, mask, c = pack(proofs, mont if montgomery else limbs)
    return PS.pok_verify_each(P, sg, pts, z, values, mask, c, montgomery=montgomery).tolist()


def each_both_forms(P, proofs, sg, pts):
    st = each(P, proofs, sg, pts)
    assert st == each(P, proofs, sg, pts, montgomery=True)
    return st


_S = {}


def scenario(lmax=LMAX, rows=N):
    if (lmax, rows) not in _S:
        _S[lmax, rows] = Scenario(lmax, rows)
    return _S[lmax, rows]


def msgs_of(S, L, n, f=limbs):
    return f([v for i in range(n) for v in S.msgs[i][:L]]).reshape(n, L, 4)


def solve_first(key, m):
    """m with its first entry replaced so that x + sum y_j m_j = 0"""
    m = list(m)
    m[0] = (-(key.x + sum(y * v for y, v in zip(key.ys[1:], m[1:]))) * M.inv(key.ys[0])) % R
    assert key.exponent(m) == 0
    return m


# ---- signatures --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS)
def test_sign_many_against_the_model(L):
    """(sigma_1, sigma_2) = (s1 G, s2 G) limb for limb for every shape and both input forms; then every signature verifies, one by one and as a batch"""
    S = scenario()
    want = S.sigs(L)
    with S.params(L) as P:
        for n in NS:
            for f, mg in FORMS:
                A, bad = PS.sign_many(P, f(S.key.sk(L)), msgs_of(S, L, n, f), f(S.rs[:n]), montgomery=mg)
                assert not bad.any() and (A == want[:n]).all(), (n, mg)
                assert PS.verify_each(P, A, msgs_of(S, L, n, f), montgomery=mg).tolist() == [1] * n, (n, mg)
                assert PS.verify_batch(P, A, msgs_of(S, L, n, f), f([RHO])[0], montgomery=mg), (n, mg)
        assert PS.verify_batch(P, want[:65], [m[:L] for m in S.msgs[:65]], 1) and PS.verify_batch(P, want[:65], msgs_of(S, L, 65), R - 1)


@pytest.mark.parametrize("L", [1, 30])
def test_identity_elements_are_flagged_and_refused_and_their_neighbours_intact(L):
    """r_i = 0 at rows 1 and 63 (both elements the identity), u_i = 0 at row 32 (the first message solves x + sum y_j m_j = 0: sigma_2 = O): bad = 1 and zero
    words there, every other row as the model; no verifier accepts them.  Row 40 keeps a signature of other messages over a row whose Q_i is the identity"""
    S = scenario()
    n = 65
    rs, msgs = list(S.rs[:n]), [list(m[:L]) for m in S.msgs[:n]]
    rs[1] = rs[63] = 0
    msgs[32] = solve_first(S.key, msgs[32])
    logs = [S.key.sign(r, m) for r, m in zip(rs, msgs)]
    assert [i for i, s in enumerate(logs) if 0 in s] == [1, 32, 63] and logs[32][0] != 0 and logs[1] == (0, 0)
    want = g1_times([v for s in logs for v in s]).reshape(n, 2, 12)
    with S.params(L) as P:
        for f, mg in FORMS:
            m_ = f([v for m in msgs for v in m]).reshape(n, L, 4)
            A, bad = PS.sign_many(P, f(S.key.sk(L)), m_, f(rs), montgomery=mg)
            assert bad.tolist() == [1 if 0 in s else 0 for s in logs] and (A == want).all()
            assert not A[1].any() and not A[32][1].any() and A[32][0].any()
            assert PS.verify_each(P, A, m_, montgomery=mg).tolist() == [0 if 0 in s else 1 for s in logs]      # ZeroSignature
            assert not PS.verify_batch(P, A, m_, f([RHO])[0], montgomery=mg)
        # Q_40 = O under a signature with no identity element: the first pair is skipped, the second decides
        msgs[40] = solve_first(S.key, msgs[40])
        assert S.key.q(msgs[40]) == 0 and not S.key.verifies(logs[40], msgs[40])
        ok = [1 if S.key.verifies(s, m) else 0 for s, m in zip(logs, msgs)]
        assert ok[40] == 0 and sum(ok) == n - 4
        assert PS.verify_each(P, want, [m for m in msgs]).tolist() == ok


def neg_point(pt):
    """-P on affine Montgomery words: y -> p - y"""
    out = pt.copy()
    if pt.any():
        y = P_MOD - sum(int(w) << (64 * k) for k, w in enumerate(pt[6:]))
        out[6:] = [(y >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]
    return out


@pytest.mark.parametrize("L", [2, 31])
def test_verify_each_follows_planted_faults_and_equals_the_composed_chain(L):
    """faults in sigma_1, sigma_2, a first and a last message, an identity and a negated element; then Q_i from dgpu_msm_g2_handle_many on the model's rows and the
    pairings from dgpu_multi_pairing_segments — the caller's chain — row by row"""
    S = scenario()
    n = 65
    logs, msgs = [list(s) for s in S.sig_logs(L)[:n]], [list(m[:L]) for m in S.msgs[:n]]
    logs[0][0] += 1; logs[15][1] += 1; msgs[16][0] = (msgs[16][0] + 1) % R; msgs[33][L - 1] = (msgs[33][L - 1] + 1) % R; logs[64][1] = 0; logs[40][1] = R - logs[40][1]
    faults = {0, 15, 16, 33, 40, 64}
    want = [1 if S.key.verifies(s, m) else 0 for s, m in zip(logs, msgs)]
    assert want == [0 if i in faults else 1 for i in range(n)]
    A = S.sigs(L)[:n].copy()
    A[sorted(faults)] = g1_times([v for i in sorted(faults) for v in logs[i]]).reshape(len(faults), 2, 12)
    one = O.fp12_one()
    with S.params(L) as P:
        for f, mg in FORMS:
            m_ = f([v for m in msgs for v in m]).reshape(n, L, 4)
            assert PS.verify_each(P, A, m_, montgomery=mg).tolist() == want
            assert not PS.verify_batch(P, A, m_, f([RHO])[0], montgomery=mg)
        rows = limbs([v for m in msgs for v in M.verify_row(m)]).reshape(n, L + 1, 4)
        qj, qinf = P.bases.msm_many(rows, flags=True)
        Q = np.stack([np.zeros(24, np.uint64) if qinf[i] else O.G2.to_affine(qj[i])[0] for i in range(n)])
        assert (Q[:8] == g2_times([S.key.q(m) for m in msgs[:8]])).all()
        gts = multi_pairings([(np.stack([A[i][0], neg_point(A[i][1])]), np.stack([Q[i], P.points[L + 1]])) for i in range(n)])
        chain = [1 if A[i][0].any() and A[i][1].any() and (gts[i] == one).all() else 0 for i in range(n)]
        assert chain == want


@pytest.mark.parametrize("L", [2, 30])
def test_verify_batch_single_tampers_and_a_cancelling_pair(L):
    S = scenario()
    with S.params(L) as P:
        for n in (1, 65, N):
            m_ = msgs_of(S, L, n)
            for i in sorted({0, n // 2, n - 1}):
                B = S.sigs(L)[:n].copy()
                B[i][1] = g1_times([S.sig_logs(L)[i][1] + 1])[0]
                assert not PS.verify_batch(P, B, m_, 2), (n, i)
                B = S.sigs(L)[:n].copy()
                B[i][0] = g1_times([S.sig_logs(L)[i][0] + 1])[0]
                assert not PS.verify_batch(P, B, m_, 2), (n, i)
            msgs = [list(m[:L]) for m in S.msgs[:n]]
            msgs[n - 1][L - 1] = (msgs[n - 1][L - 1] + 1) % R
            assert not PS.verify_batch(P, S.sigs(L)[:n], msgs, 2) and PS.verify_batch(P, S.sigs(L)[:n], m_, 2)
        # sigma_2 shifted by +X and -X in two rows: with rho = 1 the two errors cancel; rho = 2 weighs them apart; the per-row verdicts see both
        n, i, j, X = 65, 7, 41, 0x123456789
        logs = [list(s) for s in S.sig_logs(L)[:n]]
        logs[i][1], logs[j][1] = (logs[i][1] + X) % R, (logs[j][1] - X) % R
        msgs = [m[:L] for m in S.msgs[:n]]
        assert S.key.batch_verifies(logs, msgs, 1) and not S.key.batch_verifies(logs, msgs, 2)
        A = S.sigs(L)[:n].copy()
        A[[i, j]] = g1_times(logs[i] + logs[j]).reshape(2, 2, 12)
        for f, mg in FORMS:
            m_ = msgs_of(S, L, n, f)
            assert PS.verify_batch(P, A, m_, f([1])[0], montgomery=mg) and not PS.verify_batch(P, A, m_, f([2])[0], montgomery=mg)
            assert PS.verify_each(P, A, m_, montgomery=mg).tolist() == [0 if k in (i, j) else 1 for k in range(n)]


# ---- proofs of knowledge -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS)
def test_the_scenarios_proofs_every_shape_and_both_forms(L):
    """the model's status for every row: all-hidden and all-revealed rows, c = 0, c = r - 1 and messages 0 and r - 1 among them"""
    S = scenario()
    proofs = S.proofs(L)
    sg, pts = S.points(L)
    assert {tuple(p.mask) for p in proofs[:9]} >= {tuple([0] * L), tuple([1] * L)}
    assert [p.status(S.key) for p in proofs] == [0] * len(proofs) and proofs[9].c == 0 and proofs[10].c == R - 1
    with S.params(L) as P:
        for n in [n for n in NS if n <= len(proofs)] + ([FEW] if len(proofs) == FEW else []):
            assert each_both_forms(P, proofs[:n], sg[:n], pts[:n]) == [0] * n, n


def test_every_tamper_kind_in_one_call():
    """257 proofs of 30 messages, every kind at the first row or a row between: the status is the reference's first error, 3 over 1 over 4; the neighbours verify"""
    S = scenario()
    L, n = 30, N
    both = mixed_rows(S, L, n)
    assert both[0] == 0
    plan = dict(zip(both, KINDS))
    plan.update({7: "hidden", 8: "revealed", 256: "forged"})                         # (7: everything hidden; 8: everything revealed; the last row)
    proofs, sg, pts = S.tampered(L, n, plan)
    want = [p.status(S.key) for p in proofs]
    for i, t in plan.items():
        assert want[i] == KINDS[t] or (t == "mask" and want[i] in (3, 4)), (i, t)
    assert sum(1 for v in want if v) == len(plan) and sorted(set(want)) == [0, 1, 3, 4]
    with S.params(L) as P:
        assert each_both_forms(P, proofs, sg, pts) == want


@pytest.mark.parametrize("L", [2, 32])
def test_tampers_at_every_other_full_size(L):
    """65 rows: a mask bit on the hidden and on the revealed side, a revealed message, the signature's elements — beside valid neighbours"""
    S = scenario()
    n = 65
    both = mixed_rows(S, L, n)
    plan = dict(zip(both, ["t", "revealed", "mask", "s1_identity", "forged", "forged_and_t", "s1_identity_and_t", "k", "z_r", "hidden", "c", "s2_identity"]))
    flip = [i for i in both if i not in plan and S.proofs(L)[i].mask[0] == 1][0]
    plan[flip] = "mask"                                                             # a revealed entry declared hidden
    proofs, sg, pts = S.tampered(L, n, plan)
    want = [p.status(S.key) for p in proofs]
    assert all(want[i] == KINDS[t] or t == "mask" for i, t in plan.items()) and want[flip] in (3, 4) and sum(1 for v in want if v) == len(plan)
    with S.params(L) as P:
        assert each_both_forms(P, proofs, sg, pts) == want


def test_every_call_across_forced_chunk_borders(twin):
    """sixteen MSM rows per chunk through the development surface — sixteen signatures, eight proofs — 65 rows of 30 messages: every call valid, then faults at the
    first row, on both sides of a border and at the last row"""
    S = scenario()
    L, n = 30, 65
    with S.params(L) as P:
        try:
            assert twin.dgpu_set_many_chunk_rows(16) == 0
            proofs, (sg, pts) = S.proofs(L)[:n], [a[:n] for a in S.points(L)]
            assert each_both_forms(P, proofs, sg, pts) == [0] * n
            for k, t in enumerate(KINDS):
                b = 8 if k % 2 == 0 else 48                                 # proofs are cut every eight rows
                rows = [i for i in (0, b - 1, b, 64) if (t != "hidden" or 0 in proofs[i].mask) and (t not in ("revealed",) or (1 in proofs[i].mask))]
                tp, tsg, tpts = S.tampered(L, n, {i: t for i in rows})
                want = [p.status(S.key) for p in tp]
                assert all(want[i] != 0 for i in rows) or t in ("c",), t
                assert each(P, tp, tsg, tpts) == want, t
            for f, mg in FORMS:
                A, bad = PS.sign_many(P, f(S.key.sk(L)), msgs_of(S, L, n, f), f(S.rs[:n]), montgomery=mg)
                assert not bad.any() and (A == S.sigs(L)[:n]).all()
                assert PS.verify_each(P, A, msgs_of(S, L, n, f), montgomery=mg).tolist() == [1] * n
                assert PS.verify_batch(P, A, msgs_of(S, L, n, f), f([RHO])[0], montgomery=mg)
            for i in (0, 15, 16, 64):
                B = A.copy()
                B[i] = S.sigs(L)[(i + 1) % n]
                assert PS.verify_each(P, B, msgs_of(S, L, n, mont), montgomery=True).tolist() == [0 if k == i else 1 for k in range(n)]
                assert not PS.verify_batch(P, B, msgs_of(S, L, n), RHO)
        finally:
            twin.dgpu_set_many_chunk_rows(0)


def test_three_rows_of_128_messages_take_two_blocks_per_row():
    S = scenario(128, 3)
    L, n = 128, 3
    sigs = g1_times([v for i in range(n) for v in S.key.sign(S.rs[i], S.msgs[i])]).reshape(n, 2, 12)
    proofs = [S.prove(L, i) for i in range(n)]
    proofs[1] = tamper(S, L, 1, proofs[1], "hidden")
    proofs[2] = tamper(S, L, 2, proofs[2], "forged")
    sg, pts = points_of(proofs)
    want = [p.status(S.key) for p in proofs]
    assert want == [0, 3, 4]
    with S.params(L) as P:
        for f, mg in FORMS:
            A, bad = PS.sign_many(P, f(S.key.sk(L)), msgs_of(S, L, n, f), f(S.rs), montgomery=mg)
            assert not bad.any() and (A == sigs).all()
            assert PS.verify_each(P, A, msgs_of(S, L, n, f), montgomery=mg).tolist() == [1, 1, 1] and PS.verify_batch(P, A, msgs_of(S, L, n, f), f([RHO])[0], montgomery=mg)
        B = sigs.copy(); B[1] = sigs[2]
        assert PS.verify_each(P, B, msgs_of(S, L, n)).tolist() == [1, 0, 1] and not PS.verify_batch(P, B, msgs_of(S, L, n), RHO)
        assert each_both_forms(P, proofs, sg, pts) == want


def test_rows_longer_than_the_many_row_kernels_accept():
    """L + 1 = 31 and L + 2 = 32 above a lowered dgpu_set_small_msm_max: the single-row driver inside the calls, normalised over Fq2 on the host, gives the same bytes"""
    S = scenario()
    L, n = 30, 9
    with S.params(L) as P:
        try:
            assert lib().dgpu_set_small_msm_max(8) == 0
            proofs, sg, pts = S.tampered(L, n, {4: "t", 6: "forged", 3: "s1_identity"})
            assert each(P, proofs, sg, pts) == [0, 0, 0, 1, 3, 0, 4, 0, 0]
            A = S.sigs(L)[:n].copy()
            assert PS.verify_each(P, A, msgs_of(S, L, n)).tolist() == [1] * n and PS.verify_batch(P, A, msgs_of(S, L, n), RHO)
            A[5] = S.sigs(L)[6]
            assert PS.verify_each(P, A, msgs_of(S, L, n)).tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 1] and not PS.verify_batch(P, A, msgs_of(S, L, n), RHO)
        finally:
            lib().dgpu_set_small_msm_max(8192)


def test_a_second_call_of_a_shape_allocates_nothing():
    S = scenario()
    L, n = 2, 8
    A, m = S.sigs(L)[:n], msgs_of(S, L, n)
    proofs, (sg, pts) = S.proofs(L)[:n], [a[:n] for a in S.points(L)]
    with S.params(L) as P:
        calls = [("sign_many", lambda: PS.sign_many(P, S.key.sk(L), m, S.rs[:n])[0].tolist(), A.tolist()), ("verify_each", lambda: PS.verify_each(P, A, m).tolist(), [1] * n),
                 ("verify_batch", lambda: PS.verify_batch(P, A, m, RHO), True), ("pok", lambda: each(P, proofs, sg, pts), [0] * n)]
        for name, call, want in calls:
            assert call() == want, name
            before = lib().dgpu_device_alloc_count()
            got = call()
            assert lib().dgpu_device_alloc_count() == before, name
            assert got == want, name


def test_two_threads_at_once_give_the_same_bytes():
    S = scenario()
    L = 30
    jobs = []
    for k in range(2):
        n = 63 + k
        proofs, sg, pts = S.tampered(L, n, {k: "t", 30 + k: "z_r", n - 1: "forged"})
        jobs.append((n, proofs, sg, pts, [p.status(S.key) for p in proofs]))
    with S.params(L) as P:
        P.g_table                                                            # (the lazy table: built before the threads start)
        def work(k):
            n, proofs, sg, pts, want = jobs[k % 2]
            A, bad = PS.sign_many(P, S.key.sk(L), msgs_of(S, L, n), S.rs[:n])
            return each(P, proofs, sg, pts) == want and not bad.any() and (A == S.sigs(L)[:n]).all() and PS.verify_each(P, A, msgs_of(S, L, n)).all() and \
                PS.verify_batch(P, A, msgs_of(S, L, n), 77 + k) and each(P, S.proofs(L)[:n], *[a[:n] for a in S.points(L)]) == [0] * n
        with ThreadPoolExecutor(2) as ex:
            assert all(ex.map(work, range(4)))


def test_handles_the_calls_refuse():
    """a handle of another length, a precomputed one, a G1 handle, no handle at all; a G2 table or a bases handle for g: DGPU_E_BADARG"""
    S = scenario()
    with S.params(2) as P:
        pre = DeviceBases(CG2, P.points); pre.precompute(16)
        g1h = DeviceBases(CG1, g1_times([1, 2, 3, 4]))
        sg, pts = (a[:3] for a in S.points(2))
        for handle, L in ((P.handle, 1), (P.handle, 3), (pre.handle, 2), (g1h.handle, 2), (0xDEADBEEF, 2)):
            class Q:
                pass
            q = Q(); q.handle, q.L, q.g_tilde_pc, q.all_pc = handle, L, P.g_tilde_pc, np.ascontiguousarray(np.tile(P.g_tilde_pc, (L + 2, 1)))
            m, A = msgs_of(S, L, 3), S.sigs(L)[:3]
            z, values, mask, c = pack([M.Proof([1, 1], 1, 1, [5] * L, [0] * L, 7, 9)] * 3)
            for call in (lambda: PS.verify_each(q, A, m), lambda: PS.verify_batch(q, A, m, 5), lambda: PS.pok_verify_each(q, sg, pts, z, values, mask, c)):
                with pytest.raises(ca.DockGpuError) as err:
                    call()
                assert err.value.code == -3, (handle, L)
        for table in (P.handle, g1h.handle, 0xDEADBEEF):
            class Q:
                pass
            q = Q(); q.L, q.g_table = 2, table
            with pytest.raises(ca.DockGpuError) as err:
                PS.sign_many(q, S.key.sk(2), msgs_of(S, 2, 3), S.rs[:3])
            assert err.value.code == -3
        pre.free(); g1h.free()
