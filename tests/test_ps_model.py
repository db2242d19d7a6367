"""CPU: the big-integer model of the PS (Coconut) calls (tests/ps_model.py) against itself and against the oracle's own G1 / G2 scalar multiplication, MSM and
pairing on the reference's equations (coconut/src/signature/ps_signature.rs:95-142, proof/signature_pok/proof.rs:32-56, randomized_signature.rs:62-89,
k.rs:99-115): a handful of signatures and proofs.  Nothing of the library runs here: these are checks of the yardstick the other tests measure with."""
import numpy as np
import oracle_c as O
import ps_model as M
from ps_model import R

lim = lambda v: O.int_to_limbs(v % R, 4)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def mul(G, k):
    k %= R
    return np.zeros(G.AW, np.uint64) if k == 0 else G.to_affine(G.mul(G.generator(), lim(k)))[0]


def g1(k):
    return mul(O.G1, k)


def g2(k):
    return mul(O.G2, k)


def g2_msm(bases, scalars):
    aff, inf = O.G2.to_affine(O.G2.msm(np.stack(bases), np.stack([lim(v) for v in scalars])))
    return np.zeros(24, np.uint64) if inf else aff


def pairing_is_one(ps, qs):
    keep = [i for i in range(len(ps)) if ps[i].any() and qs[i].any()]              # an identity contributes one
    if not keep:
        return True
    gt = O.final_exponentiation(O.multi_miller_loop(np.stack([ps[i] for i in keep]), np.stack([qs[i] for i in keep])))
    return gt is not None and bool((gt == O.fp12_one()).all())


class Setup:
    def __init__(self, seed, L):
        rng = np.random.default_rng(seed)
        self.rng, self.L = rng, L
        x, gamma, gamma_t = rand(rng, 3)
        self.key = M.Key(x, rand(rng, L), gamma, gamma_t)
        self.pk = [g2(k) for k in self.key.pk_scalars(L)]                          # alpha_tilde, beta_tilde .., g_tilde
        self.g_tilde = self.pk[L + 1]


def test_the_chunks_of_a_batch_line_up_and_the_rows_have_their_shapes():
    rng = np.random.default_rng(5)
    msgs = [rand(rng, 3) for _ in range(40)]
    whole = M.col_scalars(3, msgs)
    a, b = M.col_scalars(3, msgs[:25]), M.col_scalars(3, msgs[25:], i0=25)
    assert [x + y for x, y in zip(a, b)] == whole and len(whole) == 5 and whole[0][7] == pow(3, 7, R) and whole[4][7] == R - pow(3, 7, R)
    assert whole[2][9] == pow(3, 9, R) * msgs[9][1] % R
    assert M.verify_row([5, R + 6]) == [1, 5, 6]
    pf = M.Proof([1, 2], 3, 4, [10, 11, 12], [0, 1, 0], 9, 7)
    assert pf.rows() == ([0, 10, 0, 12, 9], [1, 0, 11, 0, 0])
    assert [M.status_of(s, a, b, p) for s in (0, 1) for a in (0, 1) for b in (0, 1) for p in (0, 1)] == [3] * 8 + [4, 0, 1, 1, 1, 1, 1, 1]


def test_signatures_against_the_oracle():
    """sigma = (s1 G, s2 G) verifies by the oracle's pairing exactly where the model says so: e(sigma_1, Q) e(-sigma_2, g_tilde) = 1 with Q from the oracle's G2
    MSM over [alpha_tilde, beta_tilde ..]; the batch equation's L + 2 pairs by the oracle too"""
    S = Setup(7, 3)
    rng, key = S.rng, S.key
    rs, msgs = rand(rng, 6), [rand(rng, 3) for _ in range(6)]
    msgs[1], msgs[2] = [0, 0, 0], [R - 1, 0, 1]
    sigs = [key.sign(r, m) for r, m in zip(rs, msgs)]
    for i in range(6):
        s1, s2 = sigs[i]
        assert (s1, s2) == (rs[i] * key.gamma % R, rs[i] * key.exponent(msgs[i]) * key.gamma % R)
        forged = i in (3, 5)
        if forged:
            s2 = (s2 + 1) % R
        assert key.verifies((s1, s2), msgs[i]) == (not forged)
        Q = g2_msm(S.pk[:4], M.verify_row(msgs[i]))
        assert (Q == g2(key.q(msgs[i]))).all()
        assert pairing_is_one([g1(s1), g1(R - s2)], [Q, S.g_tilde]) == (not forged), i
    assert not key.verifies((0, sigs[0][1]), msgs[0]) and not key.verifies((sigs[0][0], 0), msgs[0])
    # Q = O: m_0 solves x + sum y_j m_j = 0; sigma_2 is then the identity, and no sigma_2 != O verifies
    m = list(msgs[0]); m[0] = (-(key.x + sum(y * v for y, v in zip(key.ys[1:], m[1:]))) * M.inv(key.ys[0])) % R
    assert key.exponent(m) == 0 and key.q(m) == 0 and key.sign(5, m)[1] == 0 and not key.verifies((5, 7), m)
    for rho in (1, 2, 0x1234567):
        cols = M.col_scalars(rho, msgs)
        ps = [g1(sum(c * (s[1] if k == 4 else s[0]) for c, s in zip(cols[k], sigs))) for k in range(5)]
        assert pairing_is_one(ps, S.pk) and key.batch_verifies(sigs, msgs, rho)
    bad = sigs[:2] + [(sigs[2][0], sigs[2][1] + 1)] + sigs[3:]
    assert not key.batch_verifies(bad, msgs, 2) and key.batch_verifies([], [], 2)
    cols = M.col_scalars(2, msgs)
    assert not pairing_is_one([g1(sum(c * (s[1] if k == 4 else s[0]) for c, s in zip(cols[k], bad))) for k in range(5)], S.pk)
    # sigma_2 shifted by +X and -X in two rows: rho = 1 cannot tell, rho = 2 can
    X = 12345
    pair = [(sigs[0][0], sigs[0][1] + X), (sigs[1][0], sigs[1][1] - X)] + sigs[2:]
    assert key.batch_verifies(pair, msgs, 1) and not key.batch_verifies(pair, msgs, 2)


def confirm(S, pf, want_schnorr=True, want_pairing=True):
    """the reference's two equations for one proof by the oracle's G2 MSM and pairing"""
    L = S.L
    hidden = [j for j in range(L) if not pf.mask[j]]
    revealed = [j for j in range(L) if pf.mask[j]]
    k, t = g2(pf.k), g2(pf.t)
    # bases.msm(responses) - k c == t over [committed beta_tilde .., g_tilde]                                (k.rs:99-115, SchnorrResponse::is_valid)
    lhs = g2_msm([S.pk[1 + j] for j in hidden] + [S.g_tilde, k], [pf.values[j] for j in hidden] + [pf.z_r, R - pf.c])
    assert bool((lhs == t).all()) == want_schnorr
    # e(sigma_1', sum_revealed m_j beta_tilde_j + k + alpha_tilde) e(-sigma_2', g_tilde) = 1                 (randomized_signature.rs:83-86)
    Q = g2_msm([S.pk[1 + j] for j in revealed] + [k, S.pk[0]], [pf.values[j] for j in revealed] + [1, 1])
    assert pairing_is_one([g1(pf.sig[0]), g1(R - pf.sig[1])], [Q, S.g_tilde]) == want_pairing
    S_row, R_row = pf.rows()
    assert (g2_msm(S.pk, S_row) == g2_msm([S.pk[1 + j] for j in hidden] + [S.g_tilde], [pf.values[j] for j in hidden] + [pf.z_r])).all()
    assert (g2_msm(S.pk + [k], R_row + [1]) == Q).all()


def make(S, i, forge=0):
    rng, L = S.rng, S.L
    msgs = rand(rng, L)
    if i == 2:
        msgs[0], msgs[L - 1] = 0, R - 1
    c = {3: 0, 4: R - 1}.get(i, rand(rng, 1)[0])
    revealed = [set(), set(range(L)), {0}, {L - 1}, {1, 3}, {0, 2, 4}][i % 6]
    s1, s2 = S.key.sign(rand(rng, 1)[0], msgs)
    r, r_bar = rand(rng, 2)
    return M.prove(S.key, (s1, s2 + forge), msgs, revealed, r, r_bar, rand(rng, L + 1), c)


def test_proofs_against_the_oracle():
    """valid proofs under every mask kind, messages 0 and r - 1, c = 0 and c = r - 1: the oracle confirms both equations; a wrong response breaks the Schnorr
    equation alone, a forged sigma_2 the pairing alone; the order of the errors is 3, 1, 4"""
    S = Setup(100, 5)
    for i in range(6):
        pf = make(S, i)
        assert pf.checks(S.key) == (True, True, True) and pf.status(S.key) == 0, i
        confirm(S, pf)
        if i in (0, 4):
            q = pf.copy(); q.values[2] = (q.values[2] + 1) % R                       # (entry 2 is hidden under both masks)
            assert q.checks(S.key) == (False, True, True) and q.status(S.key) == 3
            confirm(S, q, want_schnorr=False)
            forged = make(S, i, forge=1)
            assert forged.checks(S.key) == (True, True, False) and forged.status(S.key) == 4
            confirm(S, forged, want_pairing=False)
    pf = make(S, 4)                                                                  # mask {1, 3}: entry 0 hidden, entry 1 revealed; c = r - 1
    assert pf.mask == [0, 1, 0, 1, 0]
    for field, want in (("t", 3), ("k", 3), ("z_r", 3), ("c", 3)):
        q = pf.copy(); setattr(q, field, (getattr(q, field) + 1) % R)
        assert q.status(S.key) == want, field
    q = pf.copy(); q.values[0] += 1
    assert q.status(S.key) == 3                                                      # a hidden response
    q = pf.copy(); q.values[1] += 1
    assert q.status(S.key) == 4                                                      # a revealed message: the Schnorr relation does not see it
    q = pf.copy(); q.mask[0] = 1
    assert q.status(S.key) == 3
    q = pf.copy(); q.mask[1] = 0
    assert q.status(S.key) == 3
    q = pf.copy(); q.sig[0] = 0
    assert q.status(S.key) == 1
    q = pf.copy(); q.sig[1] = 0
    assert q.status(S.key) == 1
    q = pf.copy(); q.sig[0] = 0; q.t += 1
    assert q.status(S.key) == 3                                                      # the Schnorr error comes first
    q = make(S, 4, forge=1); q.t += 1
    assert q.status(S.key) == 3
