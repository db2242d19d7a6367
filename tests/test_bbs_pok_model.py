"""CPU: the big-integer model of the proof-of-knowledge calls (tests/bbs_pok_model.py) against itself and against the oracle's group arithmetic on the reference's
four equations (bbs_plus/src/proof.rs:529-611).  Nothing of the library runs here: these are checks of the yardstick the other tests measure with."""
import numpy as np
import oracle_c as O
import bbs_model as BM
import bbs_pok_model as PM
from bbs_model import R


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def test_the_batch_of_two_chunks_adds_up():
    """the model's own consistency: the sums of two chunks add up to the whole (what the second pass relies on)"""
    rng = np.random.default_rng(5)
    proofs = [PM.Proof([0] * 5, rand(rng, 4), rand(rng, 2), [i & 1, (i >> 1) & 1], rand(rng, 1)[0]) for i in range(40)]
    c, w, tp, tn = PM.batch(None, proofs, 3)
    c0, w0, tp0, tn0 = PM.batch(None, proofs[:25], 3)
    c1, w1, tp1, tn1 = PM.batch(None, proofs[25:], 3, i0=25)
    assert [(a + b) % R for a, b in zip(c0, c1)] == c and w0 + w1 == w and tp0 + tp1 == tp and tn0 + tn1 == tn


def test_the_model_against_the_oracle():
    """one proof from known discrete logs, three of five messages hidden: the oracle's own MSMs over the points confirm the reference's two Schnorr equations and its
    pairing equation; the model's four verdicts follow every tamper; a proof made from a non-signature fails the pairing alone"""
    G = O.G1
    rng = np.random.default_rng(99)
    x, gamma = rand(rng, 2)
    L = 5
    key = BM.Key(x, gamma, rand(rng, L + 1))
    e, s, msgs = rand(rng, 1)[0], rand(rng, 1)[0], rand(rng, L)
    a = key.a(e, s, msgs)
    r1, r2, c = rand(rng, 3)
    pf = PM.prove(key, a, e, s, msgs, {1, 3}, r1, r2, rand(rng, 4 + L), c)
    assert pf.checks(key) == (True, True, True, True) and pf.status(key) == 0 and pf.mask == [0, 1, 0, 1, 0]
    lim = lambda v: O.int_to_limbs(v % R, 4)
    gen = G.generator()
    mul = lambda k: G.to_affine(G.mul(gen, lim(k)))[0]
    H = np.stack([mul(k) for k in key.params_scalars(L)])
    Ap, Abar, d, T1, T2 = [mul(k) for k in pf.pts]
    z1, z2, z3, z4 = pf.fixed
    # z1 A' + z2 h_0 - c (Abar - d) = T1
    lhs = G.msm(np.stack([Ap, H[1], Abar, d]), np.stack([lim(z1), lim(z2), lim(R - c), lim(c)]))
    assert (G.to_affine(lhs)[0] == T1).all()
    # sum_hidden z_j h_j + z3 d + z4 h_0 + c (g1 + sum_revealed m_j h_j) = T2
    bases = [H[2 + j] for j in range(L)] + [d, H[1], H[0]]
    sc = [pf.values[j] if not pf.mask[j] else c * msgs[j] for j in range(L)] + [z3, z4, c]
    assert (G.to_affine(G.msm(np.stack(bases), np.stack([lim(v) for v in sc])))[0] == T2).all()
    # e(A', w) e(-Abar, g2) = 1
    g2 = O.G2.generator()
    w = O.G2.to_affine(O.G2.mul(g2, lim(x)))[0]
    gt = O.final_exponentiation(O.multi_miller_loop(np.stack([Ap, mul(R - pf.pts[1])]), np.stack([w, g2])))
    assert gt is not None and (gt == O.fp12_one()).all()
    for field, k, want in (("pts", 3, 2), ("pts", 2, 2), ("fixed", 0, 2), ("fixed", 1, 2), ("pts", 4, 3), ("fixed", 2, 3), ("fixed", 3, 3), ("values", 0, 3), ("values", 1, 3)):
        q = pf.copy()
        getattr(q, field)[k] = (getattr(q, field)[k] + 1) % R
        assert q.status(key) == want, (field, k)
    q = pf.copy(); q.c = (q.c + 1) % R
    assert q.status(key) == 2
    q = pf.copy(); q.mask[0] = 1
    assert q.status(key) == 3
    q = pf.copy(); q.pts[0] = 0
    assert q.status(key) == 1
    forged = PM.prove(key, (a + 1) % R, e, s, msgs, {1, 3}, r1, r2, rand(rng, 4 + L), c)
    assert forged.checks(key) == (True, True, True, False) and forged.status(key) == 4
    assert PM.batch_verdict(key, [pf, pf.copy()], 5) and not PM.batch_verdict(key, [pf, forged], 5) and PM.batch_verdict(key, [], 5)
