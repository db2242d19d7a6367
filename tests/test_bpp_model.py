"""CPU: the integer model of the Bulletproofs++ calls (tests/bpp_model.py) against itself and the curve.  The prover is the reference's, ported line by line; the
verifier exists twice — the reference's vector pipeline transcribed literally and the closed form the kernels compute — and the two must give the same scalar for
every base and the same verdict, on the ten shapes of the issue.  Honest proofs sum to zero; every tamper does not: each own point, l0, n0, each challenge, a
value of 2^num_bits or more committed with truncated digits, a proof made for another setup.  The model runs over a discrete-log group (a point is its
logarithm); for (2, 8, 1) and (16, 8, 1) the same scalars are also laid over real BLS12-381 points by the C oracle, whose MSM must be the identity exactly where
the model says so."""
import numpy as np
import pytest
import bpp_model as BM
from bbs_model import R

IDS = ["%d-%d-%d" % s for s in BM.SHAPES]
_CASES = {}


def case(shape):
    """(shape, setup, honest proofs: random values, all zero, all 2^num_bits - 1)"""
    if shape not in _CASES:
        s = BM.Shape(*shape)
        rnd = BM.make_rnd(1000 + 7 * BM.SHAPES.index(shape))
        setup = BM.Setup(s, rnd)
        top = (1 << s.num_bits) - 1
        vals = [[rnd() & top for _ in range(s.m)], [0] * s.m, [top] * s.m]
        _CASES[shape] = (s, setup, [BM.prove(s, setup, v, rnd) for v in vals], rnd)
    return _CASES[shape]


@pytest.mark.parametrize("shape", BM.SHAPES, ids=IDS)
def test_shape_constants(shape):
    s = BM.Shape(*shape)
    assert s.NG & (s.NG - 1) == 0 and s.K == max(3, s.lg) and s.shared == 9 + s.NG
    _, _, proofs, _ = case(shape)
    for p in proofs:
        assert len(p.X) == len(p.Rr) == s.K and len(p.l) == len(p.n) == 1 and len(p.chal) == 7 + s.K and len(p.own_points()) == s.own
    assert (BM.Shape(2, 64, 2).NG, BM.Shape(2, 64, 2).K, BM.Shape(2, 64, 2).own) == (128, 7, 20)          # proof_system's shape: 137 + 20 = 157 terms


@pytest.mark.parametrize("shape", BM.SHAPES, ids=IDS)
def test_the_two_verifiers_agree_and_accept_honest_proofs(shape):
    s, setup, proofs, _ = case(shape)
    for p in proofs:
        lit, closed = BM.verify_literal(s, s.NG, p), BM.verify_closed(s, p)
        assert lit[0] == closed[0], [k for k in range(s.shared) if lit[0][k] != closed[0][k]][:5]
        assert lit[1] == closed[1]
        assert BM.equation(setup, p, *lit) == 0 and BM.status(s, setup, p) == 0
    assert BM.batch_ok(s, setup, proofs, 12345) and BM.batch_ok(s, setup, proofs, 1)


@pytest.mark.parametrize("shape", BM.SHAPES, ids=IDS)
def test_every_tamper_is_refused_by_both(shape):
    s, setup, proofs, _ = case(shape)
    p = proofs[0]
    for what in BM.tamper_kinds(s):
        q = BM.tamper(p, what)
        lit, closed = BM.verify_literal(s, s.NG, q), BM.verify_closed(s, q)
        assert lit == closed, what
        if what == "lambda" and s.m == 1:                                     # one value: lambda^0 alone enters the equation, in the reference too
            assert BM.equation(setup, q, *lit) == 0 and BM.status(s, setup, q) == 0
            continue
        assert BM.equation(setup, q, *lit) != 0 and BM.status(s, setup, q) == 1, what
        assert not BM.batch_ok(s, setup, [proofs[1], q, proofs[2]], 98765), what
    # two tampers that cancel in the plain sum: +1 on S in one proof, the matching shift in the other.  S weighs -1/t: proof a gains -1/t_a, proof b must lose it
    a, b = proofs[0], proofs[1]
    qa = BM.tamper(a, "S", 1)
    qb = BM.tamper(b, "S", -BM.inv(a.chal[6]) * b.chal[6] % R)
    assert BM.status(s, setup, qa) == BM.status(s, setup, qb) == 1
    assert BM.batch_ok(s, setup, [qa, qb, proofs[2]], 1) and not BM.batch_ok(s, setup, [qa, qb, proofs[2]], 2)


@pytest.mark.parametrize("shape", BM.SHAPES, ids=IDS)
def test_out_of_range_values_and_foreign_setups(shape):
    s, setup, proofs, rnd = case(shape)
    if s.num_bits < 64:
        for v in (1 << s.num_bits, (1 << s.num_bits) + 5, (1 << 63) + 1):
            p = BM.prove(s, setup, [v] + [1] * (s.m - 1), rnd)                  # V commits to v, the digits to v mod 2^num_bits
            assert BM.verify_literal(s, s.NG, p) == BM.verify_closed(s, p) and BM.status(s, setup, p) == 1, v
        p = BM.prove(s, setup, [1] * (s.m - 1) + [(1 << s.num_bits) - 1], rnd)  # ... and the largest value that fits passes
        assert BM.status(s, setup, p) == 0
    other = BM.Setup(s, rnd)
    p = BM.prove(s, other, [3] * s.m, rnd)
    assert BM.status(s, other, p) == 0 and BM.status(s, setup, p) == 1
    assert BM.verify_literal(s, s.NG, p) == BM.verify_closed(s, p)


@pytest.mark.parametrize("shape", BM.SHAPES, ids=IDS)
def test_status_two(shape):
    s, setup, proofs, _ = case(shape)
    p = proofs[0]
    zero = [("t", 6, 0), ("r", 3, 0)] + [("e", 0, (R - k) % R) for k in range(s.base)]
    for name, pos, v in zero:
        q = p.copy()
        q.chal[pos] = v
        assert BM.verify_closed(s, q) is None and BM.status(s, setup, q) == 2, (name, v)
        assert not BM.batch_ok(s, setup, [proofs[1], q], 5)
        with pytest.raises(AssertionError):                                   # where the reference unwrap()s
            BM.verify_literal(s, s.NG, q)
    q = p.copy()
    q.chal[0] = R - s.base                                                     # e = -base is an ordinary wrong challenge
    assert BM.status(s, setup, q) == 1


@pytest.mark.parametrize("shape", [(2, 8, 1), (16, 8, 1)], ids=["2-8-1", "16-8-1"])
def test_over_the_real_curve(shape):
    """every generator and every point of a proof as a real point (its log times the oracle's generator): the oracle's MSM over the closed form's scalars is the
    identity for honest proofs and is not for tampered ones"""
    import oracle_c as O
    G = O.G1
    s, setup, proofs, _ = case(shape)
    limbs = lambda vals: np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)

    def points(logs):
        out, inf = O.g1_scale_batch(np.tile(G.generator(), (len(logs), 1)), limbs([v % R for v in logs]), threads=4)
        assert not inf.any()
        return out
    base_pts = points(setup.logs())
    for p, want in [(proofs[0], True), (proofs[1], True), (BM.tamper(proofs[0], "M"), False), (BM.tamper(proofs[0], "n0"), False), (BM.tamper(proofs[2], "gamma1"), False)]:
        shared, own = BM.verify_closed(s, p)
        assert BM.verify_literal(s, s.NG, p) == (shared, own)
        pts = np.concatenate([base_pts, points(p.own_points())])
        _, inf = G.to_affine(G.msm(pts, limbs(shared + own), threads=4))
        assert bool(inf) == want == (BM.equation(setup, p, shared, own) == 0)
