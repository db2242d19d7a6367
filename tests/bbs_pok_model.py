"""Big-integer model of the proof-of-knowledge calls of crypto_amd/csrc/dock_bbs.hip (dgpu_bbs_plus_pok_verify_each_g1, dgpu_bbs_plus_pok_verify_batch_g1) and of the
scalar kernels in front of them (bbs_pok_kernels.hip.h).  It extends the known-discrete-log idea of bbs_model.Key: with g1 = gamma G, h_k = eta_k G and a
signature A = a G, every point of a PoKOfSignatureG1Proof (bbs_plus/src/proof.rs:159-251) is a known multiple of G, so the reference's four checks (:529-611) can be
decided in the exponent.  Plain Python integers modulo r: nothing here shares code with the library."""
from bbs_model import R


def inv(v):
    return pow(v % R, R - 2, R)


class Proof:
    """One proof as the logs of its points over G and its scalars.  pts = [A', Abar, d, T1, T2]; fixed = [z1, z2, z3, z4]; values[j] is the revealed message or the
    response of the hidden message j; mask[j] = 1 where j is revealed.  The fields are plain lists: a test tampers with them in place."""

    def __init__(self, pts, fixed, values, mask, c):
        self.pts, self.fixed, self.values, self.mask, self.c = [v % R for v in pts], [v % R for v in fixed], [v % R for v in values], list(mask), c % R

    def copy(self):
        return Proof(self.pts, self.fixed, self.values, self.mask, self.c)

    def row(self):
        """the row of the many-row MSM: (c, z4, y_1 .. y_L), y_j = c m_j where revealed, the response where hidden"""
        return [self.c, self.fixed[3]] + [(self.c * v if m else v) % R for v, m in zip(self.values, self.mask)]

    def own(self):
        """the own-point scalars: (z1, z2, -c, c, -1) over [A', h_0, Abar, d, T1], then (z3, -1) over [d, T2]"""
        z1, z2, z3, _ = self.fixed
        return [z1, z2, (R - self.c) % R, self.c, R - 1, z3, R - 1]

    def checks(self, key):
        """(A' != O, first Schnorr check, second Schnorr check, pairing) in the exponent"""
        ap, abar, d, t1, t2 = self.pts
        z1, z2, z3, _ = self.fixed
        H = key.params_scalars(len(self.values))
        first = (z1 * ap + z2 * H[1] - self.c * (abar - d) - t1) % R == 0
        second = (sum(v * h for v, h in zip(self.row(), H)) + z3 * d - t2) % R == 0
        return ap != 0, first, second, (key.x * ap - abar) % R == 0

    def status(self, key):
        """0, or the first error PoKOfSignatureG1Proof::verify returns: 1 ZeroSignature, 2 / 3 the Schnorr checks, 4 the pairing"""
        for k, ok in enumerate(self.checks(key)):
            if not ok:
                return k + 1
        return 0


def prove(key, a, e, s, msgs, revealed, r1, r2, blind, c):
    """PoKOfSignatureG1Protocol::init and gen_proof for the signature (a G, e, s) — a need not be b / (x + e): then everything but the pairing stays consistent.
    blind: the blindings of (-e, r2) in the first protocol, of (-r3, s') in the second, then one per message (used where it is hidden)"""
    L = len(msgs)
    H = key.params_scalars(L)
    b = key.b(s, msgs)
    ap = r1 * a % R
    abar = (r1 * b - e * ap) % R
    d = (r1 * b - r2 * H[1]) % R
    r3 = inv(r1)
    sp = (s - r2 * r3) % R
    b1, b2, bd, bh = blind[:4]
    bl = blind[4:4 + L]
    mask = [1 if j in revealed else 0 for j in range(L)]
    t1 = (b1 * ap + b2 * H[1]) % R
    t2 = (sum(bl[j] * H[2 + j] for j in range(L) if not mask[j]) + bd * d + bh * H[1]) % R
    fixed = [b1 - e * c, b2 + r2 * c, bd - r3 * c, bh + sp * c]
    values = [msgs[j] if mask[j] else bl[j] + msgs[j] * c for j in range(L)]
    return Proof([ap, abar, d, t1, t2], fixed, values, mask, c)


def weights(rho, i):
    """(u_i, v_i, t_i) = (rho^(2i), rho^(2i+1), rho^i)"""
    t = pow(rho, i, R)
    u = t * t % R
    return u, u * rho % R, t


def batch(key, proofs, rho, i0=0):
    """(C, w5, tp, tn) of the proofs i0 .. of a batch: C_0 = sum v c, C_1 = sum (u z2 + v z4), C_(j+1) = sum v y_j; w5[i] the weights of proof i over its own points
    A', Abar, d, T1, T2; tp[i] = rho^i, tn[i] = -rho^i"""
    L = len(proofs[0].values) if proofs else 0
    C = [0] * (L + 2)
    w5, tp, tn = [], [], []
    for k, p in enumerate(proofs):
        u, v, t = weights(rho, i0 + k)
        z1, z2, z3, z4 = p.fixed
        row = p.row()
        C[0] = (C[0] + v * p.c) % R
        C[1] = (C[1] + u * z2 + v * z4) % R
        for j in range(L):
            C[2 + j] = (C[2 + j] + v * row[2 + j]) % R
        w5.append([u * z1 % R, (R - u * p.c) % R, (u * p.c + v * z3) % R, (R - u) % R, (R - v) % R])
        tp.append(t)
        tn.append((R - t) % R)
    return C, w5, tp, tn


def batch_verdict(key, proofs, rho):
    """what dgpu_bbs_plus_pok_verify_batch_g1 decides: no A' the identity, the one G1 equation, the merged pairing — in the exponent"""
    if not proofs:
        return True
    if any(p.pts[0] == 0 for p in proofs):
        return False
    C, w5, tp, _ = batch(key, proofs, rho)
    H = key.params_scalars(len(proofs[0].values))
    g = sum(c * h for c, h in zip(C, H)) + sum(w * q for p, ws in zip(proofs, w5) for w, q in zip(ws, p.pts))
    pairing = sum(t * (key.x * p.pts[0] - p.pts[1]) for p, t in zip(proofs, tp))
    return g % R == 0 and pairing % R == 0
