"""GPU (-m gpu): the two range-proof calls (crypto_amd/csrc/dock_smc.hip, smc_kernels.hip.h) through crypto_amd.smc_range_proof.  The parameters, the commitment
key, the signatures and the proofs come from known discrete logs (tests/smc_model.py) through the oracle's scalar multiplication, so every point is k G for a k the
model computes and every expected (status, detail) and verdict is decided in the exponent; two proofs are confirmed by the oracle's own MSM and pairing on the
reference's equations before any GPU verdict is trusted.  Every comparison is exact.  Points are computed once per discrete log and shared by every test."""
from concurrent.futures import ThreadPoolExecutor
import os
import re
import numpy as np
import pytest
import torch
import oracle_c as O
import smc_model as SM
from smc_model import CLS, CCS
import crypto_amd as ca
from crypto_amd import smc_range_proof as SRP
from crypto_amd._native import twin
from bbs_model import R

pytestmark = pytest.mark.gpu
R2 = pow(2, 256, R)
P_MOD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
G = O.G1
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "crypto_amd", "csrc")
RHO = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
# (kind, base, min, max): the statements of the issue — l = 64, rm = 2, rm = 1, l = 0, base 16; CCS with l = 5 and l = 64
STATEMENTS = [(CLS, 2, 0, 2 ** 64 - 1), (CLS, 3, 5, 13), (CLS, 3, 5, 12), (CLS, 4, 10, 11), (CLS, 16, 0, 65536), (CCS, 4, 10, 1000), (CCS, 2, 0, 2 ** 63)]
IDS = ["cls-2-l64", "cls-3-rm2", "cls-3-rm1", "cls-4-l0", "cls-16", "ccs-4", "ccs-2-l64"]


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


class World:
    """the key, the parameters as points, and every point ever asked for by its discrete log"""

    def __init__(self):
        rng = np.random.default_rng(31415)
        self.key = SM.Key(*rand(rng, 4))
        self.cache = {0: np.zeros(12, np.uint64)}
        self.g2 = O.G2.generator()
        self.pk = O.G2.to_affine(O.G2.mul(self.g2, O.int_to_limbs(self.key.alpha, 4)))[0]
        g1, g, h = self.points([self.key.gamma, self.key.kg, self.key.kh])
        self.params = SRP.Params(g1, self.g2, self.pk, g, h)
        self.cases = {}

    def points(self, logs):
        """k G as affine ABI words (k = 0: zero words) for every log, on the oracle's host threads; each log once"""
        new = sorted({k % R for k in logs} - set(self.cache))
        if new:
            out, inf = O.g1_scale_batch(np.tile(G.generator(), (len(new), 1)), limbs(new), threads=16)
            out[inf.astype(bool)] = 0
            self.cache.update(zip(new, out))
        return np.stack([self.cache[k % R] for k in logs]) if len(logs) else np.zeros((0, 12), np.uint64)

    def case(self, k):
        """(statement, n honest proofs, the same proofs made with signatures under another key)"""
        if k not in self.cases:
            kind, base, lo, hi = STATEMENTS[k]
            st = SM.Statement(kind, lo, hi, base)
            rng = np.random.default_rng(100 + k)
            n = 2 if st.l == 64 else 4
            values = [lo, hi - 1] + [lo + int(rng.integers(0, 2 ** 62)) % (hi - lo) for _ in range(n - 2)]
            honest, forged = [], []
            for v in values:
                b = rand(rng, 1 + st.sides * (1 + 3 * st.l) + 2)
                honest.append(SM.prove(self.key, st, v, b[-1], b[-2], lambda j: b[j]))
                forged.append(SM.prove(self.key, st, v, b[-1], b[-2], lambda j: b[j], other_key=True))
            assert all(p.status(self.key, st) == (0, 0) for p in honest)
            self.cases[k] = (st, honest, forged)
        return self.cases[k]

    def sixty_five(self):
        """(statement 1, 65 honest proofs of it, its tampers, 65 scalars for the merged form): made once, shared by the tests that need them"""
        if "65" not in self.cases:
            st, honest, forged = self.case(1)
            var = [p for _, p in variants(st, honest, forged)]
            rng = np.random.default_rng(65)
            good = []
            for i in range(65):
                b = rand(rng, 1 + st.sides * (1 + 3 * st.l) + 2)
                good.append(SM.prove(self.key, st, st.min + i % (st.max - st.min), b[-1], b[-2], lambda j: b[j]))
            self.cases["65"] = (st, good, var, rand(rng, 65))
        return self.cases["65"]

    def pack(self, st, proofs, f=limbs):
        pts = self.points([p.C for p in proofs] + [v for p in proofs for v in p.D] + [v for p in proofs for d in p.digits for v in (d.ap, d.abar, d.t)])
        n = len(proofs)
        return SRP.Proofs(st.as_tuple(), pts[:n], f([p.c for p in proofs]), pts[n:n + n * st.sides], f([v for p in proofs for v in p.zr]), pts[n + n * st.sides:],
                          f([v for p in proofs for d in p.digits for v in (d.z1, d.z2)]))


_W = []


def world():
    if not _W:
        _W.append(World())
    return _W[0]


def each(W, st, proofs, random=None, montgomery=False):
    f = mont if montgomery else limbs
    status, detail = SRP.verify_each(W.params, st.as_tuple(), W.pack(st, proofs, f), None if random is None else f(random), montgomery=montgomery)
    return list(zip(status.tolist(), detail.tolist()))


def batch(W, st, proofs, rho, montgomery=False):
    f = mont if montgomery else limbs
    return SRP.verify_batch(W.params, st.as_tuple(), W.pack(st, proofs, f), f([rho])[0], montgomery=montgomery)


def variants(st, honest, forged):
    """one tamper per proof, on the first and last proof and the first and last digit: [(name, proof, kind of check)]"""
    out = []
    for i in sorted({0, len(honest) - 1}):
        p, fp = honest[i], forged[i]
        for s in range(st.sides):
            out.append(("D%d" % s, SM.tamper(p, "D", s=s)))
        for d in sorted({0, st.D - 1}) if st.D else []:
            out.append(("A_identity", SM.tamper(p, "A_identity", d)))
            out.append(("z1", SM.tamper(p, "z1", d)))
            out.append(("forged", SM.tamper(p, "forged", d, forged=fp)))
            out.append(("D_and_digit", SM.tamper(SM.tamper(p, "z1", d), "D", s=st.sides - 1)))
        if st.D >= 2:
            a, b = (st.l, 1) if st.sides == 2 else (st.D - 1, 0)          # CCS: max[0] (position 1) and min[1] (position 2); CLS: the last digit and the first
            out.append(("two_digits", SM.tamper(SM.tamper(p, "forged", a, forged=fp), "z1", b)))
    return out


def neg_point(pt):
    out = pt.copy()
    if pt.any():
        y = P_MOD - sum(int(w) << (64 * k) for k, w in enumerate(pt[6:]))
        out[6:] = [(y >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]
    return out


def test_the_oracle_confirms_the_proofs_before_any_gpu_verdict():
    """one CLS (rm = 2) and one CCS proof: every equation by the oracle's MSM over the points with the model's own scalars, two pairings by its Miller loop and
    final exponentiation; a signature under another key breaks the pairing alone"""
    W = world()
    one = O.fp12_one()

    def msm_is_identity(bases, scalars):
        live = [(b, s) for b, s in zip(bases, scalars) if b.any() and s % R]
        return not live or bool(G.to_affine(G.msm(np.stack([b for b, _ in live]), np.stack([O.int_to_limbs(s % R, 4) for _, s in live])))[1])

    def pairing(x1, x2):
        gt = O.final_exponentiation(O.multi_miller_loop(np.stack([x1, neg_point(x2)]), np.stack([W.pk, W.g2])))
        return gt is not None and bool((gt == one).all())

    for k in (1, 5):
        st, honest, forged = W.case(k)
        p = honest[0]
        own, bases = p.own(st), W.points(p.bases(W.key, st))
        for m in range(st.M):
            assert msm_is_identity(bases[4 * m:4 * m + 4], own[4 * m:4 * m + 4]), (k, m)
            assert not msm_is_identity(bases[4 * m:4 * m + 4], [own[4 * m] + 1] + own[4 * m + 1:4 * m + 4]), (k, m)
        d = p.digits[st.D - 1]
        assert pairing(*W.points([d.ap, d.abar]))
        f = forged[0].digits[st.D - 1]
        assert not pairing(*W.points([f.ap, f.abar]))


@pytest.mark.parametrize("k", range(len(STATEMENTS)), ids=IDS)
def test_honest_proofs_and_every_tamper(k):
    """the statement's honest proofs and one tamper per proof in ONE call: the (status, detail) of the reference's first error, in both input forms; the merged
    form agrees (3, 0 where the exact form found the pairing alone); the batch accepts the honest proofs and refuses each tamper"""
    W = world()
    st, honest, forged = W.case(k)
    var = variants(st, honest, forged)
    proofs = honest + [p for _, p in var]
    want = [p.status(W.key, st) for p in proofs]
    assert want[:len(honest)] == [(0, 0)] * len(honest) and all(w != (0, 0) for w in want[len(honest):])
    for (name, _), w in zip(var, want[len(honest):]):
        assert w[0] == (1 if name.startswith("D") else 2), name
    got = each(W, st, proofs)
    assert got == want
    assert each(W, st, proofs, montgomery=True) == want
    rnd = rand(np.random.default_rng(k), len(proofs))
    want_m = [p.status(W.key, st, random=r) for p, r in zip(proofs, rnd)]
    for (name, _), w, m in zip(var, want[len(honest):], want_m[len(honest):]):
        assert (m == (3, 0) and w[1] % 4 == 3) if name == "forged" else (m[0] == 2 if name == "two_digits" else m == w), name
    assert each(W, st, proofs, random=rnd) == want_m and each(W, st, proofs, random=rnd, montgomery=True) == want_m
    assert batch(W, st, honest, RHO) and batch(W, st, honest, RHO, montgomery=True) and batch(W, st, honest[:1], 1) and batch(W, st, honest, R - 1)
    assert batch(W, st, [], RHO) and each(W, st, []) == []
    assert not batch(W, st, proofs, RHO)
    seen = set()
    for name, p in var:
        if name in seen:
            continue
        seen.add(name)
        assert not SM.batch_verdict(W.key, st, honest + [p], RHO)
        assert not batch(W, st, honest + [p], RHO), name
        assert not batch(W, st, [p] + honest, RHO, montgomery=True), name


def test_sixty_five_proofs_in_forced_chunks():
    """n = 65 with the chunks cut to 64 proofs and to 1 proof through the development surface: the statuses, the merged statuses and the batch verdicts are
    those of the uncut call"""
    W = world()
    st, good, var, rnd = W.sixty_five()
    proofs = list(good)
    for i, v in zip((0, 1, 31, 63, 64), (var[0], var[3], var[1], var[2], var[5])):
        proofs[i] = v
    want = [p.status(W.key, st) for p in proofs]
    assert sum(1 for w in want if w != (0, 0)) == 5
    want_m = [p.status(W.key, st, random=r) for p, r in zip(proofs, rnd)]
    assert each(W, st, proofs) == want and each(W, st, proofs, random=rnd) == want_m and batch(W, st, good, RHO) and not batch(W, st, proofs, RHO)
    with twin(smc=True) as T:
        try:
            for rows in (64, 1):
                assert T.dgpu_set_many_chunk_rows(rows) == 0
                assert each(W, st, proofs) == want, rows
                assert each(W, st, proofs, random=rnd) == want_m, rows
                assert batch(W, st, good, RHO) and not batch(W, st, proofs, RHO), rows
                assert not batch(W, st, good[:64] + [proofs[64]], RHO), rows          # the bad proof alone in the last chunk
        finally:
            T.dgpu_set_many_chunk_rows(0)


def tiled_batches(W, st, src, good, n, cases):
    """every case's batch of n proofs — tile i is source i mod `good`, but for the places a case names — in both input forms: the GPU verdict is the model's,
    a batch passing exactly when the model gives status (0, 0) to the source of every tile.  The model's statuses are taken before any GPU verdict is read"""
    status = [p.status(W.key, st) for p in src]
    assert status[:good] == [(0, 0)] * good and all(w != (0, 0) for w in status[good:])
    tiles = np.arange(n) % good
    for montgomery in (False, True):
        f = mont if montgomery else limbs
        P = W.pack(st, src, f)
        rho = f([RHO])[0]
        for name, put in cases:
            idx = tiles.copy()
            for at, which in put.items():
                idx[at] = which
            want = all(status[k] == (0, 0) for k in idx)
            assert want == (not put), name
            T = SRP.Proofs(st.as_tuple(), P.commitments[idx], P.challenge[idx], P.side_points.reshape(len(src), -1)[idx], P.side_responses.reshape(len(src), -1)[idx],
                           P.digit_points.reshape(len(src), -1)[idx], P.digit_responses.reshape(len(src), -1)[idx])
            assert SRP.verify_batch(W.params, st.as_tuple(), T, rho, montgomery=montgomery) == want, (name, montgomery)
    return status


def test_a_batch_across_the_border_of_a_block_of_equations():
    """n proofs in ONE chunk whose n M equations fill more than one block of k_smc_col_sums (256 lanes x 16 equations = 4096): n = 4096 div M + 2, so that
    4096 + M < n M <= SMC_BATCH_EQS: proof j = 4096 div M holds equation 4096 and proof j + 1 lies wholly in the second block.  The proofs are tiled from a few
    sources, so the model's work is theirs alone.
    Statement 1 (the 65 proofs of the forced-chunk test; M = 4): the honest batch verifies; it is refused with one tampered proof in the second block (j + 1),
    with one just before the border (j - 1, equations 4092 .. 4095) and with one at it (j, equations 4096 .. 4099).  M = 4 divides 4096, so no proof of this
    statement has equations on both sides of the border.
    The CCS statement with l = 5 (M = 12; its 4 honest proofs): proof 341 holds equations 4092 .. 4103 and STRADDLES the border — its two side equations and its
    first two digits' in the first block, the digits' from the third on in the second.  The honest batch verifies; it is refused when that proof has a side
    equation wrong (below the border), when it has the third digit's wrong (equation 4096), and when it has both."""
    W = world()
    hdr = open(os.path.join(CSRC, "smc_launch.hip.h")).read()
    eqs = int(re.search(r"SMC_BATCH_EQS = (\d+)\b", hdr).group(1))
    run = int(re.search(r"\bCOL_RUN = (\d+)\b", open(os.path.join(CSRC, "col_launch.hip.h")).read()).group(1))
    border = 256 * run
    assert border == 4096

    st, good, _, _ = W.sixty_five()
    M = st.M
    j = border // M                                                          # the proof that holds equation 4096
    n = j + 2
    assert border + M < n * M <= eqs and st.sides + st.D == M and st.D >= 1
    assert (j - 1) * M + M - 1 < border <= j * M + M - 1 and (j + 1) * M > border       # j - 1 ends below the border, j holds it, j + 1 is behind it
    # sources: 0 .. 64 the honest proofs; 65: a digit's response, 66: a side's point, 67: both (equations 0 and 1 of the proof)
    src = good + [SM.tamper(good[3], "z1", st.D - 1), SM.tamper(good[4], "D", s=0), SM.tamper(SM.tamper(good[5], "z1", 0), "D", s=0)]
    status = tiled_batches(W, st, src, 65, n, [("honest", {}), ("second block", {j + 1: 65}), ("before the border", {j - 1: 66}), ("at the border", {j: 67})])
    assert status[65][0] == 2 and status[66][0] == 1 and status[67][0] == 1

    st, honest, _ = W.case(5)
    M, S = st.M, st.sides
    j = border // M
    n = j + 2
    d = border - j * M - S                                                   # the digit of proof j whose equation is equation 4096
    assert border + M < n * M <= eqs and border % M != 0 and j * M < border == j * M + S + d < (j + 1) * M and 0 <= d < st.D
    # sources: 0 .. 3 the honest proofs; 4: side 0's point (equation j M, below the border), 5: digit d's response (equation 4096), 6: both
    src = honest + [SM.tamper(honest[1], "D", s=0), SM.tamper(honest[2], "z1", d), SM.tamper(SM.tamper(honest[3], "z1", d), "D", s=0)]
    status = tiled_batches(W, st, src, len(honest), n, [("honest", {}), ("straddling, wrong below the border", {j: len(honest)}),
                                                        ("straddling, wrong behind the border", {j: len(honest) + 1}), ("straddling, wrong on both sides", {j: len(honest) + 2})])
    assert [w[0] for w in status[len(honest):]] == [1, 2, 1]


def test_two_threads_at_once_give_the_same_bytes():
    W = world()
    jobs = []
    for k in (1, 5):
        st, honest, forged = W.case(k)
        proofs = honest + [p for _, p in variants(st, honest, forged)]
        jobs.append((st, proofs, honest, [p.status(W.key, st) for p in proofs]))
        W.pack(st, proofs)                                               # (the points, before the threads start)

    def work(t):
        st, proofs, honest, want = jobs[t % 2]
        return each(W, st, proofs) == want and batch(W, st, honest, 77 + t) and not batch(W, st, proofs, 77 + t) and each(W, st, proofs, random=[5 + t] * len(proofs))[0] == (0, 0)
    with ThreadPoolExecutor(2) as ex:
        assert all(ex.map(work, range(4)))


@pytest.mark.parametrize("k", [1, 5], ids=["cls-3-rm2", "ccs-4"])
def test_cancelling_errors_pass_under_one_and_fail_under_two(k):
    """two pairing errors that cancel inside one proof (Abar_a + delta g1, Abar_b - delta g1, the Schnorr checks consistent) pass the merged form under
    random = 1 and fail under 2; two Schnorr errors that cancel between two proofs, and the pairing pair, pass the batch under rho = 1 and fail under 2 — as
    the model says; an identity A' refuses the batch at once"""
    W = world()
    st, honest, _ = W.case(k)
    p = SM.tamper(SM.tamper(honest[0], "shift", 0, delta=5), "shift", st.D - 1, delta=R - 5)
    proofs = [honest[1], p, honest[2]]
    exact = each(W, st, proofs)
    assert exact == [p_.status(W.key, st) for p_ in proofs] and exact[1] == (2, 4 * st.ref_position(0) + 3) and exact[0] == exact[2] == (0, 0)
    assert p.status(W.key, st, random=1) == (0, 0) and p.status(W.key, st, random=2) == (3, 0)
    assert each(W, st, proofs, random=[1, 1, 1]) == [(0, 0)] * 3 and each(W, st, proofs, random=[1, 1, 1], montgomery=True) == [(0, 0)] * 3
    assert each(W, st, proofs, random=[2, 2, 2]) == [(0, 0), (3, 0), (0, 0)] and each(W, st, proofs, random=[2, 2, 2], montgomery=True) == [(0, 0), (3, 0), (0, 0)]
    assert SM.batch_verdict(W.key, st, proofs, 1) and not SM.batch_verdict(W.key, st, proofs, 2)
    assert batch(W, st, proofs, 1) and batch(W, st, proofs, 1, montgomery=True) and not batch(W, st, proofs, 2) and not batch(W, st, proofs, 2, montgomery=True)
    bad = [q.copy() for q in honest]
    bad[0].digits[0].t = (bad[0].digits[0].t + 77) % R
    bad[3].digits[st.D - 1].t = (bad[3].digits[st.D - 1].t - 77) % R
    assert SM.batch_verdict(W.key, st, bad, 1) and not SM.batch_verdict(W.key, st, bad, 2)
    assert batch(W, st, bad, 1) and not batch(W, st, bad, 2)
    assert [s for s, _ in each(W, st, bad)] == [2, 0, 0, 2]
    zero = honest[:3] + [SM.tamper(honest[3], "A_identity", st.D - 1)]
    assert not batch(W, st, zero, 1) and not batch(W, st, zero, RHO)
