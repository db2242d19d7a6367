"""Big-integer model of the accumulator proof calls of crypto_amd/csrc/dock_acc_pok.hip (dgpu_accumulator_membership_proofs_verify_each_g1 / _verify_batch_g1,
dgpu_accumulator_non_membership_proofs_verify_each_g1 / _verify_batch_g1) and of the scalar kernels in front of them (acc_pok_kernels.hip.h), in the manner of
bbs_pok_model.py: with P = pi G, Q = q G, V = v G, pk = alpha P~ and a witness C = w G, every point of a MembershipProof / NonMembershipProof
(vb_accumulator/src/proofs_cdh.rs) is a known multiple of G, so the reference's checks can be decided in the exponent.  Plain Python integers modulo r: nothing
here shares code with the library."""
from bbs_model import R


def inv(v):
    return pow(v % R, R - 2, R)


class Key:
    """the logs of everything the verifier holds: pk = alpha P~, P = pi G, Q = q G, V = v G"""

    def __init__(self, alpha, pi, q, v):
        self.alpha, self.pi, self.q, self.v = alpha % R, pi % R, q % R, v % R

    def membership_witness(self, y):
        """C = v / (y + alpha) G"""
        return self.v * inv(y + self.alpha) % R

    def non_membership_witness(self, y, d):
        """(C, d) with C (y + alpha) + d P = V"""
        return (self.v - d * self.pi) * inv(y + self.alpha) % R

    def shared(self, kind):
        return [self.v] if kind == 0 else [self.v, self.pi, self.q]


class Proof:
    """One proof as the logs of its points over G and its scalars.  kind 0 (membership): pts = [A', Abar, T], resp = [z1, z2]; kind 1 (non-membership):
    pts = [C', Cbar, J, T1, T2], resp = [s_r, s_y, s_d].  The fields are plain lists: a test tampers with them in place."""

    def __init__(self, kind, pts, resp, c):
        assert (len(pts), len(resp)) == ((3, 2) if kind == 0 else (5, 3))
        self.kind, self.pts, self.resp, self.c = kind, [v % R for v in pts], [v % R for v in resp], c % R

    def copy(self):
        return Proof(self.kind, self.pts, self.resp, self.c)

    def own(self):
        """the own scalars: (z1, -z2, -c, -1) over [V, A', Abar, T]; (s_d, -c, -1) over [Q, J, T2] then (s_r, -s_y, -s_d, -c, -1) over [V, C', P, Cbar, T1]"""
        n = lambda v: (R - v) % R
        if self.kind == 0:
            z1, z2 = self.resp
            return [z1, n(z2), n(self.c), R - 1]
        sr, sy, sd = self.resp
        return [sd, n(self.c), R - 1, sr, n(sy), n(sd), n(self.c), R - 1]

    def bases(self, key):
        """the logs of the bases of the row's segments, in the order of own()"""
        if self.kind == 0:
            ap, abar, t = self.pts
            return [key.v, ap, abar, t]
        cp, cbar, j, t1, t2 = self.pts
        return [key.q, j, t2, key.v, cp, key.pi, cbar, t1]

    def checks(self, key, v=None, pi=None, q=None):
        """the reference's checks in its order, in the exponent; v, pi, q: what the verifier is handed instead of the key's own"""
        v, pi, q = (key.v if v is None else v), (key.pi if pi is None else pi), (key.q if q is None else q)
        c = self.c
        if self.kind == 0:
            ap, abar, t = self.pts
            z1, z2 = self.resp
            return ap != 0, (z1 * v - z2 * ap - c * abar - t) % R == 0, (key.alpha * ap - abar) % R == 0
        cp, cbar, j, t1, t2 = self.pts
        sr, sy, sd = self.resp
        return (cp != 0, j != 0, (sd * q - c * j - t2) % R == 0, (sr * v - sy * cp - sd * pi - c * cbar - t1) % R == 0, (key.alpha * cp - cbar) % R == 0)

    def status(self, key, **kw):
        """0, or the number of the first failing check"""
        for k, ok in enumerate(self.checks(key, **kw)):
            if not ok:
                return k + 1
        return 0


def prove_membership(key, w, y, r, b_r, b_y, c):
    """PoKOfSignatureG1Protocol::init_with_given_randomness and gen_proof (weak_bb_sig_pok_cdh.rs:72-117) for the witness w G of the element y — w need not be
    v / (y + alpha): then everything but the pairing stays consistent.  r: sig_randomizer, b_r: its blinding, b_y: the element's blinding"""
    ap = r * w % R
    abar = (r * key.v - y * ap) % R
    t = (b_r * key.v - b_y * ap) % R
    return Proof(0, [ap, abar, t], [b_r + c * r, b_y + c * y], c)


def prove_non_membership(key, w, d, y, r, b_r, b_y, b_d, c):
    """NonMembershipProofProtocol::init and gen_proof (proofs_cdh.rs:225-266, :288-361) for the witness (w G, d) of the element y"""
    dp = d * r % R
    cp = r * w % R
    cbar = (r * key.v - y * cp - dp * key.pi) % R
    j = dp * key.q % R
    t1 = (b_r * key.v - b_y * cp - b_d * key.pi) % R
    t2 = b_d * key.q % R
    return Proof(1, [cp, cbar, j, t1, t2], [b_r + c * r, b_y + c * y, b_d + c * dp], c)


def weights(kind, rho, i):
    """(u_i, v_i, t_i): membership rho^i three times; non-membership (rho^(2i), rho^(2i+1), rho^i)"""
    t = pow(rho, i, R)
    if kind == 0:
        return t, t, t
    u = t * t % R
    return u, u * rho % R, t


def batch(proofs, rho, i0=0):
    """(S, w, tp, tn) of the proofs i0 .. of a batch: S the coefficients of the shared points (V: sum u z1, respectively V: sum u s_r, P: -sum u s_d,
    Q: sum v s_d), w[i] the weights of proof i over its own points, tp[i] = rho^i, tn[i] = -rho^i"""
    if not proofs:
        return [], [], [], []
    kind = proofs[0].kind
    S = [0] * (1 if kind == 0 else 3)
    w, tp, tn = [], [], []
    n = lambda x: (R - x % R) % R
    for k, p in enumerate(proofs):
        u, v, t = weights(kind, rho, i0 + k)
        if kind == 0:
            z1, z2 = p.resp
            S[0] = (S[0] + u * z1) % R
            w.append([n(u * z2), n(u * p.c), n(u)])
        else:
            sr, sy, sd = p.resp
            S = [(S[0] + u * sr) % R, (S[1] - u * sd) % R, (S[2] + v * sd) % R]
            w.append([n(u * sy), n(u * p.c), n(v * p.c), n(u), n(v)])
        tp.append(t)
        tn.append(n(t))
    return S, w, tp, tn


def batch_verdict(key, proofs, rho, **kw):
    """what the batch calls decide: no A' / C' / J the identity, the one G1 equation, the merged pairing — in the exponent"""
    if not proofs:
        return True
    kind = proofs[0].kind
    if any(p.pts[0] == 0 or (kind == 1 and p.pts[2] == 0) for p in proofs):
        return False
    S, w, tp, _ = batch(proofs, rho)
    shared = [kw.get("v", key.v)] if kind == 0 else [kw.get("v", key.v), kw.get("pi", key.pi), kw.get("q", key.q)]
    g = sum(s * b for s, b in zip(S, shared)) + sum(x * q for p, ws in zip(proofs, w) for x, q in zip(ws, p.pts))
    pairing = sum(t * (key.alpha * p.pts[0] - p.pts[1]) for p, t in zip(proofs, tp))
    return g % R == 0 and pairing % R == 0
