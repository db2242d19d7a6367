"""CPU: the big-integer model of the BBS (2023) calls (tests/bbs23_model.py) against itself and against the oracle's own MSM and pairing on the reference's
equations (bbs_plus/src/signature_23.rs:136-160, proof_23_cdl.rs:302-549, proof_23_ietf.rs:244-479): a dozen signatures and a dozen proofs of each kind.  Nothing of
the library runs here: these are checks of the yardstick the other tests measure with."""
import numpy as np
import oracle_c as O
import bbs23_model as M
from bbs23_model import R, CDL, IETF

G = O.G1
lim = lambda v: O.int_to_limbs(v % R, 4)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def mul(k):
    k %= R
    return np.zeros(12, np.uint64) if k == 0 else G.to_affine(G.mul(G.generator(), lim(k)))[0]


def msm_is(bases, scalars, want):
    jac = G.msm(np.stack(bases), np.stack([lim(v) for v in scalars]))
    aff, inf = G.to_affine(jac)
    return (not want.any()) if inf else bool((aff == want).all())


def pairing_is_one(a, b_neg, w, g2):
    gt = O.final_exponentiation(O.multi_miller_loop(np.stack([a, b_neg]), np.stack([w, g2])))
    return gt is not None and bool((gt == O.fp12_one()).all())


class Setup:
    def __init__(self, seed, L):
        rng = np.random.default_rng(seed)
        self.rng, self.L = rng, L
        x, gamma = rand(rng, 2)
        self.key = M.Key(x, gamma, rand(rng, L))
        self.H = [mul(k) for k in self.key.params_scalars(L)]
        self.g2 = O.G2.generator()
        self.w = O.G2.to_affine(O.G2.mul(self.g2, lim(x)))[0]


def test_the_chunks_of_a_batch_add_up():
    """the model's own consistency: the sums of two chunks add up to the whole (what the second pass relies on), for the signature columns and both proof kinds"""
    rng = np.random.default_rng(5)
    es, msgs = rand(rng, 40), [rand(rng, 3) for _ in range(40)]
    c, w, we = M.columns(3, es, msgs)
    c0, w0, we0 = M.columns(3, es[:25], msgs[:25])
    c1, w1, we1 = M.columns(3, es[25:], msgs[25:], i0=25)
    assert [(a + b) % R for a, b in zip(c0, c1)] == c and w0 + w1 == w and we0 + we1 == we and len(c) == 4
    for kind, npts, nresp in ((CDL, 5, 3), (IETF, 3, 2)):
        proofs = [M.Proof(kind, [0] * npts, rand(rng, nresp), rand(rng, 2), [i & 1, (i >> 1) & 1], rand(rng, 1)[0]) for i in range(40)]
        c, w, tp, tn = M.batch(None, proofs, 3)
        c0, w0, tp0, tn0 = M.batch(None, proofs[:25], 3)
        c1, w1, tp1, tn1 = M.batch(None, proofs[25:], 3, i0=25)
        assert [(a + b) % R for a, b in zip(c0, c1)] == c and w0 + w1 == w and tp0 + tp1 == tp and tn0 + tn1 == tn and len(c) == 3
    assert M.weights(CDL, R - 1, 7)[0] == 1 and M.weights(IETF, 1, 7)[0] == 1          # the scalars under which every u_i is one


def test_a_dozen_signatures_against_the_oracle():
    """A = a G verifies by the oracle's pairing exactly where the model says so: e(A, w) e(e A - b, g2) = 1 with b from the oracle's MSM over [g1, h ..]"""
    S = Setup(7, 3)
    rng = S.rng
    es, msgs = rand(rng, 12), [rand(rng, 3) for _ in range(12)]
    es[1], msgs[2], msgs[3] = 0, [0, 0, 0], [R - 1, 0, 1]
    for i in range(12):
        a = S.key.a(es[i], msgs[i])
        forged = i in (5, 9)
        if forged:
            a = (a + 1) % R
        assert S.key.verifies(a, es[i], msgs[i]) == (not forged)
        b = S.key.b(msgs[i])
        assert msm_is(S.H, M.row(msgs[i]), mul(b))
        assert M.sign_rows(S.key.x, [es[i]], [msgs[i]])[0] == [v * M.inv(S.key.x + es[i]) % R for v in M.row(msgs[i])]
        assert pairing_is_one(mul(a), mul(es[i] * a - b), S.w, S.g2) == (not forged), i
    sigs = [S.key.a(e, m) for e, m in zip(es, msgs)]
    assert S.key.batch_verifies(sigs, es, msgs, 5) and not S.key.batch_verifies(sigs[:5] + [sigs[5] + 1] + sigs[6:], es, msgs, 5)
    assert S.key.a(R - S.key.x, msgs[0]) is None and M.inverses(S.key.x, [R - S.key.x]) == [(0, True)]


def confirm(S, pf, want_second=True, want_pairing=True):
    """the reference's equations for one proof by the oracle's MSM and pairing"""
    L, c = S.L, pf.c
    P = [mul(k) for k in pf.pts]
    hidden = [j for j in range(L) if not pf.mask[j]]
    revealed = [j for j in range(L) if pf.mask[j]]
    shared = [S.H[1 + j] for j in hidden] + [S.H[0]] + [S.H[1 + j] for j in revealed]
    sc = [pf.values[j] for j in hidden] + [c] + [c * pf.values[j] for j in revealed]
    if pf.kind == CDL:
        Abar, Bbar, d, T1, T2 = P
        z1, z2, z3 = pf.fixed
        assert msm_is([Abar, d, Bbar], [z1, z2, R - c], T1)                               # z1 Abar + z2 d - c Bbar = T1
        assert msm_is(shared + [d], sc + [z3], T2) == want_second                         # sum_hidden z_j h_j + z3 d + c (g1 + sum_revealed m_j h_j) = T2
    else:
        Abar, Bbar, T = P
        assert msm_is(shared + [Abar, Bbar], sc + list(pf.fixed), T) == want_second       # .. + z_a Abar + z_b Bbar = T
    assert pairing_is_one(Abar, mul(R - pf.pts[1]), S.w, S.g2) == want_pairing           # e(Abar, w) e(-Bbar, g2) = 1


def make(S, kind, i, a=None):
    rng, L = S.rng, S.L
    e, msgs = rand(rng, 1)[0], rand(rng, L)
    if i == 1:
        e = 0
    if i == 2:
        msgs[0], msgs[L - 1] = 0, R - 1
    c = {3: 0, 4: R - 1}.get(i, rand(rng, 1)[0])
    revealed = [set(), set(range(L)), {0}, {L - 1}, {1, 3}, {0, 2, 4}][i % 6]
    good = S.key.a(e, msgs)
    a = good if a is None else (good + a) % R
    if kind == CDL:
        r1, r2 = rand(rng, 2)
        return M.prove_cdl(S.key, a, e, msgs, revealed, r1, r2, rand(rng, 3 + L), c)
    return M.prove_ietf(S.key, a, e, msgs, revealed, rand(rng, 1)[0], rand(rng, 2 + L), c)


def test_a_dozen_proofs_of_each_kind_against_the_oracle():
    """valid proofs (every mask kind, e = 0, messages 0 and r - 1, c = 0 and c = r - 1): the oracle confirms every equation; a wrong response breaks the Schnorr
    equation over the parameters, a forged a + 1 breaks only the pairing"""
    for kind in (CDL, IETF):
        S = Setup(100 + kind, 5)
        for i in range(12):
            pf = make(S, kind, i)
            assert pf.checks(S.key) == (True, True, True, True) and pf.status(S.key) == 0, (kind, i)
            confirm(S, pf)
            if i < 3:
                q = pf.copy()
                q.values[2] = (q.values[2] + 1) % R
                if not (q.mask[2] and q.c == 0):
                    assert q.status(S.key) == 3
                    confirm(S, q, want_second=False)
                forged = make(S, kind, i, a=1)
                assert forged.checks(S.key) == (True, True, True, False) and forged.status(S.key) == 4
                confirm(S, forged, want_pairing=False)


def test_the_models_statuses_follow_every_tamper():
    for kind, tampers in ((CDL, (("pts", 3, 2), ("pts", 2, 2), ("pts", 1, 2), ("fixed", 0, 2), ("fixed", 1, 2), ("pts", 4, 3), ("fixed", 2, 3), ("values", 0, 3), ("values", 1, 3))),
                          (IETF, (("pts", 2, 3), ("pts", 1, 3), ("fixed", 0, 3), ("fixed", 1, 3), ("values", 0, 3), ("values", 1, 3)))):
        S = Setup(200 + kind, 5)
        pf = make(S, kind, 4)                                                         # (mask {1, 3}: entry 0 hidden, entry 1 revealed; c = r - 1)
        assert pf.mask == [0, 1, 0, 1, 0] and pf.status(S.key) == 0
        for field, k, want in tampers:
            q = pf.copy()
            getattr(q, field)[k] = (getattr(q, field)[k] + 1) % R
            assert q.status(S.key) == want, (kind, field, k)
        q = pf.copy(); q.c = (q.c + 1) % R
        assert q.status(S.key) == (2 if kind == CDL else 3)
        q = pf.copy(); q.mask[0] = 1
        assert q.status(S.key) == 3
        q = pf.copy(); q.pts[0] = 0
        assert q.status(S.key) == 1
        forged = make(S, kind, 5, a=1)
        assert M.batch_verdict(S.key, [pf, pf.copy()], 5) and not M.batch_verdict(S.key, [pf, forged], 5) and M.batch_verdict(S.key, [], 5)
        assert len(pf.own()) == len(pf.own_bases()) == (6 if kind == CDL else 3)
        assert sum(s * b for s, b in zip(pf.own()[:4 if kind == CDL else 3], pf.own_bases())) % R == (0 if kind == CDL else (-sum(v * h for v, h in zip(pf.row(), S.key.params_scalars(5)))) % R)
    # a CDL proof with r1 = 0: Abar = O, and the first error is ZeroSignature
    S = Setup(300, 2)
    e, msgs = 5, [6, 7]
    z = M.prove_cdl(S.key, S.key.a(e, msgs), e, msgs, {0}, 0, 9, [1, 2, 3, 4, 5], 11)
    assert z.pts[0] == 0 and z.status(S.key) == 1
