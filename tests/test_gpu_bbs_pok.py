"""GPU (-m gpu): dgpu_bbs_plus_pok_verify_each_g1 and dgpu_bbs_plus_pok_verify_batch_g1 (crypto_amd/csrc/dock_bbs.hip, bbs_pok_kernels.hip.h) through
crypto_amd.bbs_plus.  The key, the signatures and the proofs come from known discrete logs (tests/bbs_model.py, tests/bbs_pok_model.py) through the oracle's scalar
multiplication, so every point is k G for a k the model computes and every expected status is decided in the exponent; a dozen proofs are confirmed by the oracle's own
MSMs and pairing on the reference's four equations before any GPU verdict is trusted.  Every comparison is exact.  One scenario (257 proofs of up to 31 messages, the
masks mixed: per-row patterns, all hidden, all revealed, only first, only last, alternating) is built once; every shape is a prefix of it."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import bbs_model as BM
import bbs_pok_model as PM
import crypto_amd as ca
from crypto_amd import bbs_plus as BBS
from crypto_amd import G1 as CG1
from crypto_amd.msm import DeviceBases, msm_segments
from crypto_amd.pairing import multi_pairings
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu
R = BM.R
R2 = pow(2, 256, R)
P_MOD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
G = O.G1
N = 257
NBIG = 4097
NS = [1, 2, 9, 10, 11, 63, 64, 65, 257]
LS = [1, 2, 29, 30, 31]
RHO = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
# tamper kinds and the status the reference's order of errors gives each
KINDS = {"T1": 2, "d": 2, "z1": 2, "z2": 2, "c": 2, "T2": 3, "z3": 3, "z4": 3, "hidden": 3, "revealed": 3, "mask": 3, "A_identity": 1, "forged": 4, "forged_and_T1": 2}


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
        rng = np.random.default_rng(31415)
        x, gamma = rand(rng, 2)
        self.key = BM.Key(x, gamma, rand(rng, 32))
        self.e, self.s, self.r1, self.r2, self.c = (rand(rng, N) for _ in range(5))
        self.msgs = [rand(rng, 31) for _ in range(N)]
        self.blind = [rand(rng, 4 + 31) for _ in range(N)]
        self.s[3] = 0
        self.msgs[4][0], self.msgs[5][0], self.msgs[6] = 0, R - 1, [R - 1] * 31
        self.c[9], self.c[10], self.r2[11] = 0, R - 1, 0
        self.g2 = O.G2.generator()
        self.w = O.G2.to_affine(O.G2.mul(self.g2, O.int_to_limbs(x, 4)))[0]
        self._proofs, self._pts, self._params, self._big = {}, {}, {}, None

    def prove(self, L, i, a=None):
        e, s, m = self.e[i], self.s[i], self.msgs[i][:L]
        a = self.key.a(e, s, m) if a is None else a
        assert a is not None
        mask = mask_of(i, L)
        return PM.prove(self.key, a, e, s, m, {j for j in range(L) if mask[j]}, self.r1[i], self.r2[i], self.blind[i], self.c[i])

    def proofs(self, L):
        if L not in self._proofs:
            self._proofs[L] = [self.prove(L, i) for i in range(N)]
        return self._proofs[L]

    def points(self, L):
        """the points of the valid proofs for L messages per row, (257, 5, 12) ABI words"""
        if L not in self._pts:
            self._pts[L] = g_times([k for p in self.proofs(L) for k in p.pts]).reshape(N, 5, 12)
        return self._pts[L]

    def param_points(self, L):
        if L not in self._params:
            self._params[L] = g_times(self.key.params_scalars(L))
        return self._params[L]

    def params(self, L):
        p = self.param_points(L)
        return BBS.Params(p[0], p[1], p[2:], self.g2, self.w)

    def big(self):
        """4097 valid proofs of one message: the 257 of the scenario over and over with a blinding factor r1 of their own (so no two rows hold the same points)"""
        if self._big is None:
            proofs = []
            for i in range(NBIG):
                k = i % N
                e, s, m = self.e[k], self.s[k], self.msgs[k][:1]
                mask = mask_of(k, 1)
                proofs.append(PM.prove(self.key, self.key.a(e, s, m), e, s, m, {0} if mask[0] else set(), (self.r1[k] + i) % R or 1, self.r2[k], self.blind[k], self.c[k]))
            self._big = (proofs, g_times([q for p in proofs for q in p.pts]).reshape(NBIG, 5, 12))
        return self._big

    def tampered(self, L, n, plan):
        """(proofs, points) of the first n rows with the tamper plan[i] applied to row i; the changed points are k G again for the changed k"""
        proofs, pts = [p.copy() for p in self.proofs(L)[:n]], self.points(L)[:n].copy()
        for i, kind in plan.items():
            proofs[i] = tamper(self, L, i, proofs[i], kind)
        rows = sorted(plan)
        if rows:
            pts[rows] = g_times([k for i in rows for k in proofs[i].pts]).reshape(len(rows), 5, 12)
        return proofs, pts


def tamper(S, L, i, p, kind):
    if kind in ("forged", "forged_and_T1"):
        p = S.prove(L, i, a=(S.key.a(S.e[i], S.s[i], S.msgs[i][:L]) + 1) % R)
    bump = lambda lst, k: lst.__setitem__(k, (lst[k] + 1) % R)
    if kind in ("T1", "forged_and_T1"):
        bump(p.pts, 3)
    elif kind == "d":
        bump(p.pts, 2)
    elif kind == "T2":
        bump(p.pts, 4)
    elif kind in ("z1", "z2", "z3", "z4"):
        bump(p.fixed, int(kind[1]) - 1)
    elif kind == "c":
        p.c = (p.c + 1) % R
    elif kind == "hidden":
        bump(p.values, p.mask.index(0))
    elif kind == "revealed":
        bump(p.values, p.mask.index(1))
    elif kind == "mask":
        p.mask[0] ^= 1
    elif kind == "A_identity":
        p.pts[0] = 0
    elif kind == "T1_identity":
        p.pts[3] = 0
    elif kind == "T2_identity":
        p.pts[4] = 0
    return p


def mixed_rows(S, L, n):
    """the rows whose masks hide some messages and reveal others (a tamper of either kind finds its entry) and whose challenge is not zero"""
    return [i for i, p in enumerate(S.proofs(L)[:n]) if 0 < sum(p.mask) < L and p.c != 0]


def pack(proofs, f=limbs):
    n, L = len(proofs), len(proofs[0].values)
    return (f([z for p in proofs for z in p.fixed]).reshape(n, 4, 4), f([v for p in proofs for v in p.values]).reshape(n, L, 4),
            np.array([p.mask for p in proofs], np.uint8).reshape(n, L), f([p.c for p in proofs]))


def each(P, proofs, pts, montgomery=False):
    fixed, values, mask, c = pack(proofs, mont if montgomery else limbs)
    return BBS.pok_verify_each(P, pts, fixed, values, mask, c, montgomery=montgomery).tolist()


def each_both_forms(P, proofs, pts):
    st = each(P, proofs, pts)
    assert st == each(P, proofs, pts, montgomery=True)
    return st


def batch(P, proofs, pts, rho, montgomery=False):
    f = mont if montgomery else limbs
    fixed, values, mask, c = pack(proofs, f)
    return BBS.pok_verify_batch(P, pts, fixed, values, mask, c, f([rho])[0], montgomery=montgomery)


_S = []


def scenario():
    if not _S:
        _S.append(Scenario())
    return _S[0]


def test_the_oracle_confirms_the_proofs_before_any_gpu_verdict():
    """a dozen proofs: the two Schnorr equations by the oracle's MSM over the points, e(A', w) e(-Abar, g2) = 1 by its Miller loop and final exponentiation; a
    wrong response breaks the second equation, a forged signature the pairing"""
    S = scenario()
    one = O.fp12_one()
    lim = lambda v: O.int_to_limbs(v % R, 4)
    aff = lambda jac: G.to_affine(jac)[0]
    for L, i in [(1, 0), (1, 1), (1, 2), (2, 3), (2, 4), (29, 5), (29, 6), (30, 0), (30, 9), (30, 64), (31, 10), (31, 256)]:
        p = S.proofs(L)[i]
        assert p.status(S.key) == 0
        H, (Ap, Abar, d, T1, T2) = S.param_points(L), S.points(L)[i]
        z1, z2, z3, z4 = p.fixed
        assert (aff(G.msm(np.stack([Ap, H[1], Abar, d]), np.stack([lim(z1), lim(z2), lim(R - p.c), lim(p.c)]))) == T1).all(), (L, i)
        bases = [H[2 + j] for j in range(L)] + [d, H[1], H[0]]
        sc = [p.c * v if m else v for v, m in zip(p.values, p.mask)] + [z3, z4, p.c]
        assert (aff(G.msm(np.stack(bases), np.stack([lim(v) for v in sc]))) == T2).all(), (L, i)
        sc[0] += 1
        assert not (aff(G.msm(np.stack(bases), np.stack([lim(v) for v in sc]))) == T2).all()
        gt = O.final_exponentiation(O.multi_miller_loop(np.stack([Ap, g_times([R - p.pts[1]])[0]]), np.stack([S.w, S.g2])))
        assert gt is not None and (gt == one).all(), (L, i)
    f = tamper(S, 30, 0, None, "forged")
    assert f.status(S.key) == 4
    fp = g_times([f.pts[0], R - f.pts[1]])
    assert not (O.final_exponentiation(O.multi_miller_loop(fp, np.stack([S.w, S.g2]))) == one).all()


@pytest.mark.parametrize("L", LS)
def test_valid_proofs_every_shape_and_both_forms(L):
    """status 0 for every row — all-hidden and all-revealed rows, c = 0, c = r - 1, r2 = 0, s = 0 and messages 0 and r - 1 among them — and one verdict True"""
    S = scenario()
    proofs, pts = S.proofs(L), S.points(L)
    assert {tuple(p.mask) for p in proofs[:9]} >= {tuple([0] * L), tuple([1] * L)}
    with S.params(L) as P:
        for n in NS:
            assert each_both_forms(P, proofs[:n], pts[:n]) == [0] * n, n
            assert batch(P, proofs[:n], pts[:n], RHO) and batch(P, proofs[:n], pts[:n], RHO, montgomery=True), n
        assert batch(P, proofs[:65], pts[:65], 1) and batch(P, proofs[:65], pts[:65], R - 1)


def test_a_strided_view_of_the_values_reads_nothing_between_the_rows():
    S = scenario()
    L, n = 29, 65
    proofs, pts = S.proofs(L)[:n], S.points(L)[:n]
    fixed, values, mask, c = pack(proofs)
    wide = np.full((n, L + 3, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    wide[:, :L] = values
    with S.params(L) as P:
        assert BBS.pok_verify_each(P, pts, fixed, wide[:, :L], mask, c).tolist() == [0] * n
        assert BBS.pok_verify_batch(P, pts, fixed, wide[:, :L], mask, c, RHO)


def test_every_tamper_kind_in_one_call():
    """257 proofs of 31 messages, every kind at the first row, the last row or a row between: the status is the reference's first error, the neighbours verify"""
    S = scenario()
    L, n = 31, N
    both = mixed_rows(S, L, n)
    assert both[0] == 0 and both[-1] == n - 1
    plan = dict(zip([0, n - 1] + both[1:len(KINDS) - 1], KINDS))
    plan.update({7: "hidden", 8: "revealed", 19: "T1_identity", 25: "T2_identity"})      # (7, 19, 25: everything hidden; 8: everything revealed)
    proofs, pts = S.tampered(L, n, plan)
    want = [p.status(S.key) for p in proofs]
    for i, kind in plan.items():
        if kind in KINDS:
            assert want[i] == KINDS[kind], (i, kind)
    assert want[19] == 2 and want[25] == 3 and sum(1 for v in want if v) == len(plan)
    with S.params(L) as P:
        assert each_both_forms(P, proofs, pts) == want
        assert not batch(P, proofs, pts, RHO)


def test_tampers_around_forced_chunk_borders(twin):
    """sixteen rows per chunk through the development surface, 65 proofs of 30 messages: one kind per call at the first row, on both sides of a border and at the
    last row; the batch call, cut the same way, refuses each"""
    S = scenario()
    L, n = 30, 65
    with S.params(L) as P:
        try:
            assert twin.dgpu_set_many_chunk_rows(16) == 0
            assert each_both_forms(P, S.proofs(L)[:n], S.points(L)[:n]) == [0] * n
            assert batch(P, S.proofs(L)[:n], S.points(L)[:n], RHO)
            for k, kind in enumerate(list(KINDS) + ["T1_identity", "T2_identity"]):
                b = 16 if k % 2 == 0 else 48                                # (rows 0, 15, 16, 47, 48, 64 hide some messages and reveal others)
                plan = {i: kind for i in (0, b - 1, b, 64)}
                proofs, pts = S.tampered(L, n, plan)
                want = [p.status(S.key) for p in proofs]
                assert all(want[i] == KINDS.get(kind, want[i]) and want[i] for i in plan), kind
                assert each(P, proofs, pts) == want, kind
                assert not batch(P, proofs, pts, RHO), kind
        finally:
            twin.dgpu_set_many_chunk_rows(0)


@pytest.mark.parametrize("L", [2, 30])
def test_batch_single_tampers_and_a_cancelling_pair(L):
    S = scenario()
    n = 65
    with S.params(L) as P:
        for kind in list(KINDS) + ["T1_identity", "T2_identity"]:
            for i in (0, 34, n - 1):                                       # (34 = 4 mod 6: only the last message revealed)
                if (kind == "hidden" and 0 not in S.proofs(L)[i].mask) or (kind == "revealed" and 1 not in S.proofs(L)[i].mask):
                    continue
                proofs, pts = S.tampered(L, n, {i: kind})
                assert not PM.batch_verdict(S.key, proofs, RHO)
                assert not batch(P, proofs, pts, RHO), (kind, i)
        # T1_i += X, T1_j -= X: with rho = r - 1 every u_i is one and the two errors cancel; rho = 2 weighs them apart; the per-proof verdicts see both
        i, j, X = 7, 41, 0x123456789
        proofs = [p.copy() for p in S.proofs(L)[:n]]
        pts = S.points(L)[:n].copy()
        proofs[i].pts[3], proofs[j].pts[3] = (proofs[i].pts[3] + X) % R, (proofs[j].pts[3] - X) % R
        pts[[i, j]] = g_times(proofs[i].pts + proofs[j].pts).reshape(2, 5, 12)
        assert PM.batch_verdict(S.key, proofs, R - 1) and not PM.batch_verdict(S.key, proofs, 2)
        assert batch(P, proofs, pts, R - 1) and batch(P, proofs, pts, R - 1, montgomery=True)
        assert not batch(P, proofs, pts, 2) and not batch(P, proofs, pts, 2, montgomery=True)
        assert each(P, proofs, pts) == [2 if k in (i, j) else 0 for k in range(n)]
        # one proof: the batch is the proof's own verdict
        for k in (0, 5):
            assert batch(P, proofs[k:k + 1], pts[k:k + 1], RHO) and each(P, proofs[k:k + 1], pts[k:k + 1]) == [0]
        assert not batch(P, proofs[7:8], pts[7:8], RHO) and each(P, proofs[7:8], pts[7:8]) == [2]


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_at_the_chunk_size(n):
    """L = 1, one row below, at and above the 4096 rows of a chunk (8192 segments of the segmented small MSM in one launch): every row verifies, and tampers at
    the ends and on both sides of the border are the only other statuses; the batch call sees them too"""
    S = scenario()
    proofs, pts = S.big()
    with S.params(1) as P:
        assert each(P, proofs[:n], pts[:n]) == [0] * n
        assert batch(P, proofs[:n], pts[:n], RHO)
        kinds = ["T1", "z3", "forged", "A_identity", "c", "T2"]
        plan = {i: kinds[(i + n) % 6] for i in sorted({0, n - 1, 4094, min(4095, n - 1)})}
        bad, bpts = [p.copy() for p in proofs[:n]], pts[:n].copy()
        for i, kind in plan.items():
            bad[i] = tamper(S, 1, i % N, bad[i], kind)
        bpts[sorted(plan)] = g_times([k for i in sorted(plan) for k in bad[i].pts]).reshape(len(plan), 5, 12)
        want = [p.status(S.key) for p in bad]
        assert all(want[i] == KINDS[kind] for i, kind in plan.items()) and sum(1 for v in want if v) == len(plan)
        assert each(P, bad, bpts) == want
        assert not batch(P, bad, bpts, RHO)


def test_rows_longer_than_the_many_row_kernels_accept():
    """L + 2 = 32 above a lowered dgpu_set_small_msm_max: the single-row driver inside the call gives the same statuses"""
    S = scenario()
    L, n = 30, 9
    proofs, pts = S.tampered(L, n, {4: "T2", 6: "forged"})
    with S.params(L) as P:
        try:
            assert lib().dgpu_set_small_msm_max(8) == 0
            assert each(P, proofs, pts) == [0, 0, 0, 0, 3, 0, 4, 0, 0]
            assert not batch(P, proofs, pts, RHO) and batch(P, S.proofs(L)[:n], S.points(L)[:n], RHO)
        finally:
            lib().dgpu_set_small_msm_max(8192)


def test_a_second_call_of_a_shape_allocates_nothing():
    """eight proofs of two messages: after one warming call of each of the two calls (it readies the context's idle slots too) a second identical call leaves
    dgpu_device_alloc_count where it was"""
    S = scenario()
    L, n = 2, 8
    proofs, pts = S.proofs(L)[:n], S.points(L)[:n]
    with S.params(L) as P:
        for name, call, want in (("pok_verify_each", lambda: each(P, proofs, pts), [0] * n), ("pok_verify_batch", lambda: batch(P, proofs, pts, RHO), True)):
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
        n = 62 + k
        proofs, pts = S.tampered(L, n, {k: "T1", 30 + k: "z4", n - 1: "forged"})
        jobs.append((proofs, pts, [p.status(S.key) for p in proofs]))
    with S.params(L) as P:
        def work(k):
            proofs, pts, want = jobs[k % 4]
            n = len(proofs)
            return each(P, proofs, pts) == want and not batch(P, proofs, pts, 77 + k) and batch(P, S.proofs(L)[:n], S.points(L)[:n], 77 + k) and \
                each(P, S.proofs(L)[:n], S.points(L)[:n]) == [0] * n
        with ThreadPoolExecutor(4) as ex:
            assert all(ex.map(work, range(8)))


def test_handles_the_calls_refuse():
    """a handle of another length (MessageCountIncompatibleWithSigParams), a precomputed one, no handle at all: DGPU_E_BADARG from both calls"""
    S = scenario()
    with S.params(2) as P:
        pre = DeviceBases(CG1, S.param_points(2)); pre.precompute(16)
        for handle, L in ((P.handle, 1), (P.handle, 3), (pre.handle, 2), (0xDEADBEEF, 2)):
            class Q:
                pass
            q = Q(); q.handle, q.L, q.h_0, q.pk_pc, q.g2_pc = handle, L, P.h_0, P.pk_pc, P.g2_pc
            proofs, pts = S.proofs(L)[:3], S.points(L)[:3]
            for call in (lambda: each(q, proofs, pts), lambda: batch(q, proofs, pts, 5)):
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


def test_the_composed_chain_of_public_calls_gives_the_same_statuses():
    """n = 65, L = 30: P_i from dgpu_msm_g1_handle_many on the model's rows, the five-term and the two-term sums from dgpu_msm_g1_segments over the proofs' own
    points, the pairings from dgpu_multi_pairing_segments — the caller's chain, with its host scalar work — equal pok_verify_each on rows with planted tampers"""
    S = scenario()
    L, n = 30, 65
    one = O.fp12_one()
    kinds = list(KINDS) + ["T1_identity", "T2_identity"]
    proofs, pts = S.tampered(L, n, dict(zip(mixed_rows(S, L, n), kinds)))
    h0 = S.param_points(L)[1]
    with S.params(L) as P:
        got = each(P, proofs, pts)
        rows = limbs([v for p in proofs for v in p.row()]).reshape(n, L + 2, 4)
        pj, pinf = P.bases.msm_many(rows, flags=True)
        bases = np.stack([q for i in range(n) for q in (pts[i][0], h0, pts[i][1], pts[i][2], pts[i][3], pts[i][2], pts[i][4])])
        ends = [v for i in range(n) for v in (7 * i + 5, 7 * i + 7)]
        sj, sinf = msm_segments(CG1, bases, limbs([v for p in proofs for v in p.own()]), ends, flags=True)
        gts = multi_pairings([(np.stack([pts[i][0], neg_point(pts[i][1])]), np.stack([S.w, S.g2])) for i in range(n)])
        chain = []
        for i in range(n):
            second = bool(pinf[i]) and bool(sinf[2 * i + 1]) if pinf[i] or sinf[2 * i + 1] else (neg_point(G.to_affine(pj[i])[0]) == G.to_affine(sj[2 * i + 1])[0]).all()
            chain.append(1 if not pts[i][0].any() else 2 if not sinf[2 * i] else 3 if not second else 4 if not (gts[i] == one).all() else 0)
        assert chain == got == [p.status(S.key) for p in proofs]
