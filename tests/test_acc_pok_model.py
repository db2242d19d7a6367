"""CPU: the big-integer model of the accumulator proof calls (tests/acc_pok_model.py) against itself and against the oracle's group arithmetic on the reference's
equations (vb_accumulator/src/proofs_cdh.rs:138-149, :365-387, :481-523; short_group_sig/src/weak_bb_sig_pok_cdh.rs:195-217, :270-287).  Nothing of the library
runs here: these are checks of the yardstick the other tests measure with."""
import numpy as np
import oracle_c as O
import acc_pok_model as AM
from bbs_model import R

G = O.G1


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


lim = lambda v: O.int_to_limbs(v % R, 4)


def mul(k):
    if k % R == 0:
        return np.zeros(12, np.uint64)
    return G.to_affine(G.mul(G.generator(), lim(k)))[0]


def msm_is(bases, scalars, want):
    """sum scalars_k bases_k == want over affine words (want all zero: the identity)"""
    live = [(b, s) for b, s in zip(bases, scalars) if b.any() and s % R]
    if not live:
        return not want.any()
    aff, inf = G.to_affine(G.msm(np.stack([b for b, _ in live]), np.stack([lim(s) for _, s in live])))
    return (not want.any()) if inf else bool((aff == want).all())


def pairing_holds(key, x1, x2):
    """e(X1, pk) e(-X2, P~) = 1 with P~ the generator of G2"""
    g2 = O.G2.generator()
    pk = O.G2.to_affine(O.G2.mul(g2, lim(key.alpha)))[0]
    gt = O.final_exponentiation(O.multi_miller_loop(np.stack([mul(x1), mul(R - x2)]), np.stack([pk, g2])))
    return gt is not None and bool((gt == O.fp12_one()).all())


def key_of(rng):
    return AM.Key(*rand(rng, 4))


def test_two_chunks_of_a_batch_add_up():
    """the model's own consistency: the sums of two chunks add up to the whole (what the second pass relies on)"""
    rng = np.random.default_rng(5)
    for kind, npts, nresp in ((0, 3, 2), (1, 5, 3)):
        proofs = [AM.Proof(kind, [0] * npts, rand(rng, nresp), rand(rng, 1)[0]) for _ in range(40)]
        s, w, tp, tn = AM.batch(proofs, 3)
        s0, w0, tp0, tn0 = AM.batch(proofs[:25], 3)
        s1, w1, tp1, tn1 = AM.batch(proofs[25:], 3, i0=25)
        assert [(a + b) % R for a, b in zip(s0, s1)] == s and w0 + w1 == w and tp0 + tp1 == tp and tn0 + tn1 == tn
        assert tp[39] == pow(3, 39, R) and [len(x) for x in w] == [npts] * 40


def test_membership_model_against_the_oracle():
    """a dozen proofs from known discrete logs — y = 0 and r - 1, c = 0 and r - 1, zero blindings among them: the oracle's own MSM confirms
    z1 V - z2 A' - c Abar = T and its pairing e(A', pk) e(-Abar, P~) = 1; the model's statuses follow every tamper; a forged witness fails the pairing alone"""
    rng = np.random.default_rng(2024)
    key = key_of(rng)
    V = mul(key.v)
    cases = [rand(rng, 5) for _ in range(12)]                 # y, r, b_r, b_y, c
    cases[1][0], cases[2][0], cases[3][4], cases[4][4] = 0, R - 1, 0, R - 1
    cases[5][2] = cases[5][3] = 0                             # zero blindings: T is the identity
    for k, (y, r, b_r, b_y, c) in enumerate(cases):
        pf = AM.prove_membership(key, key.membership_witness(y), y, r, b_r, b_y, c)
        assert pf.checks(key) == (True, True, True) and pf.status(key) == 0, k
        Ap, Abar, T = [mul(v) for v in pf.pts]
        z1, z2 = pf.resp
        assert msm_is([V, Ap, Abar], [z1, R - z2, R - c], T), k
        assert not msm_is([V, Ap, Abar], [z1 + 1, R - z2, R - c], T), k
        if k < 4:
            assert pairing_holds(key, pf.pts[0], pf.pts[1]), k
    assert AM.prove_membership(key, key.membership_witness(7), 7, 3, 0, 0, 5).pts[2] == 0
    y, r, b_r, b_y, c = cases[0]
    pf = AM.prove_membership(key, key.membership_witness(y), y, r, b_r, b_y, c)
    for field, k, want in (("pts", 2, 2), ("pts", 1, 2), ("resp", 0, 2), ("resp", 1, 2)):
        q = pf.copy()
        getattr(q, field)[k] = (getattr(q, field)[k] + 1) % R
        assert q.status(key) == want, (field, k)
    q = pf.copy(); q.c = (q.c + 1) % R
    assert q.status(key) == 2 and pf.status(key, v=key.v + 1) == 2
    q = pf.copy(); q.pts[0] = 0
    assert q.status(key) == 1
    forged = AM.prove_membership(key, key.membership_witness(y) + 1, y, r, b_r, b_y, c)
    assert forged.checks(key) == (True, True, False) and forged.status(key) == 3 and not pairing_holds(key, forged.pts[0], forged.pts[1])
    q = forged.copy(); q.pts[2] = (q.pts[2] + 1) % R
    assert q.status(key) == 2
    assert AM.batch_verdict(key, [pf, pf.copy()], 5) and not AM.batch_verdict(key, [pf, forged], 5) and AM.batch_verdict(key, [], 5)
    assert pf.own() == [pf.resp[0], (R - pf.resp[1]) % R, (R - c) % R, R - 1]
    assert sum(s * b for s, b in zip(pf.own(), pf.bases(key))) % R == 0


def test_non_membership_model_against_the_oracle():
    """a dozen proofs: the oracle's MSMs confirm s_d Q - c J = T2 and s_r V - s_y C' - s_d P - c Cbar = T1, its pairing e(C', pk) e(-Cbar, P~) = 1; the
    statuses follow the reference's order; a witness with d = 0 gives J = O"""
    rng = np.random.default_rng(4202)
    key = key_of(rng)
    V, Pp, Q = mul(key.v), mul(key.pi), mul(key.q)
    cases = [rand(rng, 7) for _ in range(12)]                 # y, d, r, b_r, b_y, b_d, c
    cases[1][0], cases[2][0], cases[3][6], cases[4][6] = 0, R - 1, 0, R - 1
    cases[5][3] = cases[5][4] = cases[5][5] = 0               # zero blindings: T1 and T2 are the identity
    for k, (y, d, r, b_r, b_y, b_d, c) in enumerate(cases):
        pf = AM.prove_non_membership(key, key.non_membership_witness(y, d), d, y, r, b_r, b_y, b_d, c)
        assert pf.checks(key) == (True,) * 5 and pf.status(key) == 0, k
        Cp, Cbar, J, T1, T2 = [mul(v) for v in pf.pts]
        sr, sy, sd = pf.resp
        assert msm_is([Q, J], [sd, R - c], T2), k
        assert msm_is([V, Cp, Pp, Cbar], [sr, R - sy, R - sd, R - c], T1), k
        assert not msm_is([V, Cp, Pp, Cbar], [sr, R - sy, R - sd + 1, R - c], T1), k
        if k < 4:
            assert pairing_holds(key, pf.pts[0], pf.pts[1]), k
    assert cases[5] and AM.prove_non_membership(key, 9, 4, 7, 3, 0, 0, 0, 5).pts[3:] == [0, 0]
    y, d, r, b_r, b_y, b_d, c = cases[0]
    pf = AM.prove_non_membership(key, key.non_membership_witness(y, d), d, y, r, b_r, b_y, b_d, c)
    for field, k, want in (("pts", 4, 3), ("resp", 2, 3), ("pts", 3, 4), ("resp", 0, 4), ("resp", 1, 4), ("pts", 1, 4)):
        q = pf.copy()
        getattr(q, field)[k] = (getattr(q, field)[k] + 1) % R
        assert q.status(key) == want, (field, k)
    q = pf.copy(); q.c = (q.c + 1) % R
    assert q.status(key) == 3 and pf.status(key, q=key.q + 1) == 3 and pf.status(key, pi=key.pi + 1) == 4 and pf.status(key, v=key.v + 1) == 4
    q = pf.copy(); q.pts[0] = 0
    assert q.status(key) == 1
    q.pts[2] = 0
    assert q.status(key) == 1
    q = pf.copy(); q.pts[2] = 0
    assert q.status(key) == 2
    zero_d = AM.prove_non_membership(key, key.non_membership_witness(y, 0), 0, y, r, b_r, b_y, b_d, c)
    assert zero_d.pts[2] == 0 and zero_d.status(key) == 2
    forged = AM.prove_non_membership(key, key.non_membership_witness(y, d) + 1, d, y, r, b_r, b_y, b_d, c)
    assert forged.checks(key) == (True, True, True, True, False) and forged.status(key) == 5 and not pairing_holds(key, forged.pts[0], forged.pts[1])
    assert AM.batch_verdict(key, [pf, pf.copy()], 5) and not AM.batch_verdict(key, [pf, forged], 5) and not AM.batch_verdict(key, [pf, zero_d], 5)
    own, bases = pf.own(), pf.bases(key)
    assert sum(s * b for s, b in zip(own[:3], bases[:3])) % R == 0 and sum(s * b for s, b in zip(own[3:], bases[3:])) % R == 0
