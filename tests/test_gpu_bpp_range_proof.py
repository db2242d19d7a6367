"""GPU (-m gpu): the two Bulletproofs++ calls (crypto_amd/csrc/dock_bpp.hip, bpp_kernels.hip.h) through crypto_amd.bpp_range_proof.  The setup and the proofs
come from known discrete logs (tests/bpp_model.py: the reference's prover, ported) through the oracle's scalar multiplication, so every point is k G for a k the
model computes and every expected status and verdict is decided in the exponent; one proof is confirmed by the oracle's own MSM on the reference's equation
before any GPU verdict is trusted.  Every comparison is exact.  Points are computed once per discrete log and shared by every test."""
from concurrent.futures import ThreadPoolExecutor
import os
import re
import numpy as np
import pytest
import torch
import oracle_c as O
import bpp_model as BM
import crypto_amd as ca
from crypto_amd import bpp_range_proof as BRP
from crypto_amd._native import twin, bpp_lib, DockGpuError
from bbs_model import R

pytestmark = pytest.mark.gpu
R2 = pow(2, 256, R)
G = O.G1
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "crypto_amd", "csrc")
RHO = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
# (2, 8, 1): NG = 8, K = 3, the smallest; (2, 8, 2): aggregation, lambda matters; (16, 8, 1): base > digits, pub_k reaches beyond D; (4, 16, 4); (2, 64, 2):
# proof_system's shape, NG = 128, K = 7, rows of 137 terms (the many-row kernels' multi-block path), with 3 honest proofs
SHAPES = [(2, 8, 1), (2, 8, 2), (16, 8, 1), (4, 16, 4), (2, 64, 2)]
IDS = ["%d-%d-%d" % s for s in SHAPES]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)
    yield


def limbs(vals):
    return [int(v) for v in vals]


def mont(vals):
    return [int(v) * R2 % R for v in vals]


class World:
    """every point ever asked for by its discrete log; per shape the model's setup, its honest proofs and the resident setup of each library image"""

    def __init__(self):
        self.cache = {0: np.zeros(12, np.uint64)}
        self.cases, self.setups, self.msetups = {}, {}, {}

    def points(self, logs):
        """k G as affine ABI words (k = 0: zero words) for every log, on the oracle's host threads; each log once"""
        new = sorted({k % R for k in logs} - set(self.cache))
        if new:
            sc = np.array([[(k >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for k in new], dtype=np.uint64)
            out, inf = O.g1_scale_batch(np.tile(G.generator(), (len(new), 1)), sc, threads=16)
            out[inf.astype(bool)] = 0
            self.cache.update(zip(new, out))
        return np.stack([self.cache[k % R] for k in logs]) if len(logs) else np.zeros((0, 12), np.uint64)

    def msetup(self, shape):
        if shape not in self.msetups:
            self.msetups[shape] = BM.Setup(BM.Shape(*shape), BM.make_rnd(99 + 17 * len(self.msetups)))
        return self.msetups[shape]

    def case(self, shape, n=3):
        """(shape, the model's setup, n honest proofs, a proof made for another setup, a proof of a value of 2^num_bits or more)"""
        key = (shape, n)
        if key not in self.cases:
            s = BM.Shape(*shape)
            rnd = BM.make_rnd(4242 + 31 * len(self.cases))
            setup = self.msetup(shape)
            top = (1 << s.num_bits) - 1
            vals = [[0] * s.m, [top] * s.m] + [[rnd() & top for _ in range(s.m)] for _ in range(max(n - 2, 0))]
            honest = [BM.prove(s, setup, v, rnd) for v in vals[:n]]
            foreign = BM.prove(s, BM.Setup(s, rnd), [1] * s.m, rnd)
            big = BM.prove(s, setup, [top + 2] + [1] * (s.m - 1), rnd) if s.num_bits < 64 else None
            assert all(BM.status(s, setup, p) == 0 for p in honest) and BM.status(s, setup, foreign) == 1 and (big is None or BM.status(s, setup, big) == 1)
            self.cases[key] = (s, setup, honest, foreign, big)
        return self.cases[key]

    def setup(self, shape):
        """the resident setup in the library that serves the calls right now (the product's sibling, or its development build inside `with twin(bpp=True)`)"""
        key = (shape, id(bpp_lib()))
        if key not in self.setups:
            pts = self.points(self.msetup(shape).logs())
            self.setups[key] = BRP.Setup(pts[0], pts[9:], pts[1:9])
        return self.setups[key]

    def pack(self, s, proofs, f=limbs):
        n = len(proofs)
        pts = self.points([v for p in proofs for v in p.own_points()]).reshape(n, s.own, 12) if n else np.zeros((0, s.own, 12), np.uint64)
        return BRP.Proofs(s.base, s.num_bits, s.m, pts[:, :s.m], pts[:, s.m:s.m + 4], pts[:, s.m + 4:], f([v for p in proofs for v in (p.l0, p.n0)]),
                          f([c for p in proofs for c in p.chal]))


_W = []


def world():
    if not _W:
        _W.append(World())
    return _W[0]


def each(W, shape, proofs, montgomery=False):
    s = BM.Shape(*shape)
    return BRP.verify_each(W.setup(shape), s.base, s.num_bits, W.pack(s, proofs, mont if montgomery else limbs), montgomery=montgomery).tolist()


def batch(W, shape, proofs, rho, montgomery=False):
    s = BM.Shape(*shape)
    f = mont if montgomery else limbs
    return BRP.verify_batch(W.setup(shape), s.base, s.num_bits, W.pack(s, proofs, f), random=f([rho])[0], montgomery=montgomery)


def variants(W, shape):
    """[(name, proof)]: every tamper kind of the model's tests on the first honest proof, an identity point in each own slot of the second, a value that does not
    fit, a foreign setup, and the status-2 challenges"""
    s, setup, honest, foreign, big = W.case(shape)
    out = [(k, BM.tamper(honest[0], k)) for k in BM.tamper_kinds(s)]
    for slot, k in enumerate(BM.own_slots(s)):
        out.append(("identity_" + k, BM.tamper(honest[1], k, -honest[1].own_points()[slot])))
    out.append(("foreign", foreign))
    if big is not None:
        out.append(("too_big", big))
    for name, pos, v in [("t=0", 6, 0), ("r=0", 3, 0), ("e=0", 0, 0), ("e=-(base-1)", 0, R - s.base + 1)]:
        q = honest[2 % len(honest)].copy()
        q.chal[pos] = v
        out.append((name, q))
    return out


def test_the_oracle_confirms_a_proof_before_any_gpu_verdict():
    """the reference's ONE equation over real points, by the oracle's MSM with the closed form's scalars: the identity for an honest proof, not for a tampered one"""
    W = world()
    s, setup, honest, foreign, _ = W.case((2, 8, 2))
    for p, want in ((honest[0], True), (BM.tamper(honest[0], "R1"), False), (foreign, False)):
        shared, own = BM.verify_closed(s, p)
        assert BM.verify_literal(s, s.NG, p) == (shared, own)
        pts = np.concatenate([W.points(setup.logs()), W.points(p.own_points())])
        live = [(b, v) for b, v in zip(pts, shared + own) if b.any() and v % R]
        inf = G.to_affine(G.msm(np.stack([b for b, _ in live]), np.stack([O.int_to_limbs(v % R, 4) for _, v in live])))[1]
        assert bool(inf) == want


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_honest_proofs_and_every_tamper(shape):
    """the shape's honest proofs and one variant per row in ONE call: the exact status vector, in both input forms; the batch accepts the honest proofs and refuses
    each kind of tamper and each status-2 proof"""
    W = world()
    s, setup, honest, _, _ = W.case(shape)
    var = variants(W, shape)
    proofs = honest + [p for _, p in var]
    want = [BM.status(s, setup, p) for p in proofs]
    assert want[:len(honest)] == [0] * len(honest)
    for (name, _), w in zip(var, want[len(honest):]):
        assert w == (2 if "=" in name else 0 if (name == "lambda" and s.m == 1) else 1), name
    assert each(W, shape, proofs) == want
    assert each(W, shape, proofs, montgomery=True) == want
    assert batch(W, shape, honest, RHO) and batch(W, shape, honest, RHO, montgomery=True) and batch(W, shape, honest[:1], 1) and batch(W, shape, honest, R - 1)
    assert batch(W, shape, [], RHO) and each(W, shape, []) == []
    assert not batch(W, shape, proofs, RHO)
    keep = {"V0", "V%d" % (s.m - 1), "D", "M", "R", "S", "X0", "R%d" % (s.K - 1), "l0", "n0", "gamma0", "gamma%d" % (s.K - 1), "identity_S", "identity_X%d" % (s.K - 1), "identity_V0",
            "foreign", "too_big"} | set(BM.CHAL) | {n for n, _ in var if "=" in n}
    for (name, p), w in zip(var, want[len(honest):]):
        if name not in keep or w == 0:
            continue
        assert not BM.batch_ok(s, setup, honest + [p], RHO), name
        assert not batch(W, shape, honest + [p], RHO), name
        assert not batch(W, shape, [p] + honest, RHO, montgomery=True), name


def test_row_counts_across_forced_chunks():
    """n = 1, 16, 17 and 65 proofs of (2, 8, 2) with the chunks cut to 16 through the development surface, tampers at the borders: the statuses and the batch
    verdicts are those of the model and of the uncut call"""
    W = world()
    shape = (2, 8, 2)
    s, setup, good, _, _ = W.case(shape, n=65)
    proofs = list(good)
    for i, k in zip((0, 15, 16, 31, 63, 64), ("M", "n0", "X1", "gamma2", "V1", "t")):
        proofs[i] = BM.tamper(good[i], k)
    proofs[32] = good[32].copy()
    proofs[32].chal[3] = 0                                                   # r = 0: status 2 in the middle of a chunk
    want = [BM.status(s, setup, p) for p in proofs]
    assert sorted(set(want)) == [0, 1, 2] and sum(1 for w in want if w) == 7
    assert each(W, shape, proofs) == want and batch(W, shape, good, RHO) and not batch(W, shape, proofs, RHO)
    with twin(bpp=True) as T:
        try:
            assert T.dgpu_set_many_chunk_rows(16) == 0
            for n in (1, 16, 17, 65):
                assert each(W, shape, proofs[:n]) == want[:n], n
                assert each(W, shape, good[:n], montgomery=True) == [0] * n, n
                assert batch(W, shape, good[:n], RHO) and not batch(W, shape, proofs[:n], RHO), n
            assert not batch(W, shape, good[:64] + [proofs[64]], RHO)          # the bad proof alone in the last chunk
            assert not batch(W, shape, good[:16] + [proofs[16]] + good[17:], RHO, montgomery=True)
            assert not batch(W, shape, good[:32] + [proofs[32]] + good[33:], RHO)      # status 2 in the third chunk
            assert T.dgpu_set_many_chunk_rows(1) == 0
            assert each(W, shape, proofs[:5]) == want[:5] and batch(W, shape, good[:5], RHO) and not batch(W, shape, good[:4] + [proofs[15]], RHO)
        finally:
            T.dgpu_set_many_chunk_rows(0)


def test_4097_proofs_in_one_chunk_two_blocks_a_column():
    """4097 proofs of (2, 8, 2) in ONE batch call: own = 14, so BPP_BATCH_POINTS / own = 4681 > 4096 and one chunk holds them all, which k_bpp_col_sums runs
    with two blocks a column (256 lanes x 16 proofs = 4096 a block) and k_col_finish adds.  The proofs are the 65 of the forced-chunk test, tiled, so the
    model's work is that of 65 proofs; a batch is expected to pass exactly when the model gives status 0 to the source of every tile, and the model's statuses
    are checked before any GPU verdict is read.  The honest batch verifies in both input forms; it is refused with one tampered proof in the second block
    (proof 4096) and with one just before the border (proof 4095) — a scalar of the shared columns and an own point, at either place."""
    W = world()
    shape = (2, 8, 2)
    s, setup, good, _, _ = W.case(shape, n=65)
    points = int(re.search(r"BPP_BATCH_POINTS = \(size_t\)1 << (\d+)", open(os.path.join(CSRC, "bpp_launch.hip.h")).read()).group(1))
    run = int(re.search(r"\bCOL_RUN = (\d+)\b", open(os.path.join(CSRC, "col_launch.hip.h")).read()).group(1))
    n, border = 4097, 256 * run
    assert border == 4096 and (1 << points) // s.own > border
    src = list(good) + [BM.tamper(good[7], "n0"), BM.tamper(good[40], "M")]  # sources 65 and 66
    status = [BM.status(s, setup, p) for p in src]
    assert status[:65] == [0] * 65 and status[65] == 1 and status[66] == 1
    tiles = np.arange(n) % 65
    cases = [("honest", {})] + [("%s at %d" % (("n0", "M")[which - 65], at), {at: which}) for at in (border, border - 1) for which in (65, 66)]
    for montgomery in (False, True):
        P = W.pack(s, src, mont if montgomery else limbs)
        rho = (mont if montgomery else limbs)([RHO])[0]
        rows = lambda a, per: a.reshape(len(src), per, -1)
        for name, put in cases:
            idx = tiles.copy()
            for at, which in put.items():
                idx[at] = which
            want = all(status[k] == 0 for k in idx)
            assert want == (name == "honest")
            T = BRP.Proofs(s.base, s.num_bits, s.m, rows(P.values, s.m)[idx], rows(P.round_points, 4)[idx], rows(P.wnla_points, 2 * s.K)[idx], rows(P.l_n, 2)[idx],
                           rows(P.challenges, 7 + s.K)[idx])
            assert BRP.verify_batch(W.setup(shape), s.base, s.num_bits, T, random=rho, montgomery=montgomery) == want, (name, montgomery)


def test_two_threads_at_once_give_the_same_bytes():
    W = world()
    jobs = []
    for shape in ((2, 8, 2), (16, 8, 1)):
        s, setup, honest, _, _ = W.case(shape)
        proofs = honest + [p for _, p in variants(W, shape)]
        jobs.append((shape, proofs, honest, [BM.status(s, setup, p) for p in proofs]))
        W.pack(s, proofs); W.setup(shape)                                    # (the points and the handle, before the threads start)

    def work(t):
        shape, proofs, honest, want = jobs[t % 2]
        return each(W, shape, proofs) == want and batch(W, shape, honest, 77 + t) and not batch(W, shape, proofs, 77 + t)
    with ThreadPoolExecutor(2) as ex:
        assert all(ex.map(work, range(4)))


@pytest.mark.parametrize("shape", [(2, 8, 2), (2, 64, 2)], ids=["2-8-2", "2-64-2"])
def test_cancelling_errors_pass_under_one_and_fail_under_two(shape):
    """S moved by +E in one proof and by the matching multiple of -E in another (S weighs -1/t): each proof fails alone, the batch passes under rho = 1 and fails
    under 2 — as the model says; a status-2 proof refuses the batch under any rho"""
    W = world()
    s, setup, honest, _, _ = W.case(shape)
    a, b = honest[0], honest[1]
    qa = BM.tamper(a, "S", 1)
    qb = BM.tamper(b, "S", -BM.inv(a.chal[6]) * b.chal[6] % R)
    proofs = [qa, honest[2], qb]
    assert [BM.status(s, setup, p) for p in proofs] == [1, 0, 1] and each(W, shape, proofs) == [1, 0, 1]
    assert BM.batch_ok(s, setup, proofs, 1) and not BM.batch_ok(s, setup, proofs, 2)
    assert batch(W, shape, proofs, 1) and batch(W, shape, proofs, 1, montgomery=True) and not batch(W, shape, proofs, 2) and not batch(W, shape, proofs, 2, montgomery=True)
    two = honest[0].copy()
    two.chal[6] = 0
    for rho in (1, 2, RHO):
        assert not batch(W, shape, [honest[1], two], rho) and not batch(W, shape, [two, honest[1]], rho, montgomery=True)


def test_a_setup_of_another_length_is_refused():
    W = world()
    s = BM.Shape(2, 8, 1)
    honest = W.case((2, 8, 1))[2]
    wrong = W.setup((2, 8, 2))                                                # 9 + 16 points for a shape that wants 9 + 8
    pr = W.pack(s, honest)
    with pytest.raises(DockGpuError):
        BRP.verify_each(wrong, s.base, s.num_bits, pr)
    with pytest.raises(DockGpuError):
        BRP.verify_batch(wrong, s.base, s.num_bits, pr, random=5)
