"""Big-integer model of the seven BBS (2023) calls of crypto_amd/csrc/dock_bbs.hip (dgpu_bbs23_*) and of the scalar kernels in front of them
(bbs_kernels.hip.h with one fixed column, bbs23_kernels.hip.h).  Key material from known discrete logs over the generator G of G1: g1 = gamma G, h_j = eta_j G.
With a signature A = a G every point of either PoKOfSignature23G1Proof (bbs_plus/src/proof_23_cdl.rs, proof_23_ietf.rs) is a known multiple of G, so the
reference's checks can be decided in the exponent.  Plain Python integers modulo r: nothing here shares code with the library."""

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CDL, IETF = 0, 1


def inv(v):
    return pow(v % R, R - 2, R)


# ---- signatures (signature_23.rs) ----------------------------------------------------------------------------------------------------------------------
def row(msgs, mult=1):
    """row of the many-row MSM for one signature: mult (1, m_1 .. m_L)"""
    return [mult * v % R for v in [1] + list(msgs)]


def inverses(x, es):
    """(t_i, zero_i): t_i = 1 / (x + e_i), or (0, True) where x + e_i = 0"""
    out = []
    for e in es:
        u = (x + e) % R
        out.append((0, True) if u == 0 else (inv(u), False))
    return out


def sign_rows(x, es, msgs):
    """the rows of dgpu_bbs23_sign_many_g1: t_i (1, m_i ..)"""
    return [row(m, t) for (t, _), m in zip(inverses(x, es), msgs)]


def columns(rho, es, msgs, i0=0):
    """(c, weights, weights times e) of the rows i0 .. of a batch: c_k = sum_i rho^(i0 + i) row_ik for the L + 1 columns"""
    n = len(es)
    L = len(msgs[0]) if n else 0
    c = [0] * (L + 1)
    w = pow(rho, i0, R)
    wts, we = [], []
    for i in range(n):
        for k, v in enumerate(row(msgs[i])):
            c[k] = (c[k] + w * v) % R
        wts.append(w); we.append(w * es[i] % R)
        w = w * rho % R
    return c, wts, we


class Key:
    """g1 = gamma G, h_j = eta_j G, the secret key x"""
    def __init__(self, x, gamma, etas):
        self.x, self.gamma, self.etas = x % R, gamma % R, [v % R for v in etas]

    def params_scalars(self, L):
        return [self.gamma] + self.etas[:L]

    def b(self, msgs):
        """log_G of b = g1 + sum m_j h_j"""
        return sum(v * h for v, h in zip(row(msgs), self.params_scalars(len(msgs)))) % R

    def a(self, e, msgs):
        """log_G of A = b / (x + e), or None where no signature exists (x + e = 0, or b the identity)"""
        u, b = (self.x + e) % R, self.b(msgs)
        if u == 0 or b == 0:
            return None
        return b * inv(u) % R

    def verifies(self, a, e, msgs):
        """Signature23G1::verify in the exponent: A != O and x a + e a - b = 0"""
        return a % R != 0 and (self.x * a + e * a - self.b(msgs)) % R == 0

    def batch_verifies(self, sigs, es, msgs, rho):
        """dgpu_bbs23_verify_batch_g1 in the exponent: no A the identity and x sum rho^i a_i + sum rho^i e_i a_i - sum c_k H_k = 0"""
        if any(a % R == 0 for a in sigs):
            return False
        c, wts, we = columns(rho, es, msgs)
        H = self.params_scalars(len(msgs[0])) if msgs else []
        return (self.x * sum(w * a for w, a in zip(wts, sigs)) + sum(w * a for w, a in zip(we, sigs)) - sum(ck * h for ck, h in zip(c, H))) % R == 0


# ---- proofs of knowledge -------------------------------------------------------------------------------------------------------------------------------------
class Proof:
    """One proof as the logs of its points over G and its scalars.  CDL: pts = [Abar, Bbar, d, T1, T2], fixed = [z1, z2, z3]; IETF: pts = [Abar, Bbar, T],
    fixed = [z_a, z_b].  values[j] is the revealed message or the response of the hidden message j; mask[j] = 1 where j is revealed.  The fields are plain
    lists: a test tampers with them in place."""

    def __init__(self, kind, pts, fixed, values, mask, c):
        self.kind = kind
        self.pts, self.fixed, self.values, self.mask, self.c = [v % R for v in pts], [v % R for v in fixed], [v % R for v in values], list(mask), c % R

    def copy(self):
        return Proof(self.kind, self.pts, self.fixed, self.values, self.mask, self.c)

    def row(self):
        """the row of the many-row MSM: (c, y_1 .. y_L), y_j = c m_j where revealed, the response where hidden"""
        return [self.c] + [(self.c * v if m else v) % R for v, m in zip(self.values, self.mask)]

    def own(self):
        """the own scalars: CDL (z1, z2, -c, -1) over [Abar, d, Bbar, T1], then (z3, -1) over [d, T2]; IETF (z_a, z_b, -1) over [Abar, Bbar, T]"""
        if self.kind == CDL:
            z1, z2, z3 = self.fixed
            return [z1, z2, (R - self.c) % R, R - 1, z3, R - 1]
        return [self.fixed[0], self.fixed[1], R - 1]

    def own_bases(self):
        """the logs of the bases the own scalars stand over, in segment order"""
        if self.kind == CDL:
            abar, bbar, d, t1, t2 = self.pts
            return [abar, d, bbar, t1, d, t2]
        return list(self.pts)

    def checks(self, key):
        """(Abar != O, first Schnorr check, second Schnorr check, pairing) in the exponent; IETF has no first check (True)"""
        H = key.params_scalars(len(self.values))
        p = sum(v * h for v, h in zip(self.row(), H))
        if self.kind == CDL:
            abar, bbar, d, t1, t2 = self.pts
            z1, z2, z3 = self.fixed
            first = (z1 * abar + z2 * d - self.c * bbar - t1) % R == 0
            second = (p + z3 * d - t2) % R == 0
        else:
            abar, bbar, t = self.pts
            first = True
            second = (p + self.fixed[0] * abar + self.fixed[1] * bbar - t) % R == 0
        return abar != 0, first, second, (key.x * abar - bbar) % R == 0

    def status(self, key):
        """0, or the first error the reference returns: 1 ZeroSignature, 2 / 3 the Schnorr checks (IETF: 3 alone), 4 the pairing"""
        for k, ok in enumerate(self.checks(key)):
            if not ok:
                return k + 1
        return 0


def prove_cdl(key, a, e, msgs, revealed, r1, r2, blind, c):
    """proof_23_cdl's init and gen_proof for the signature (a G, e) — a need not be b / (x + e): then everything but the pairing stays consistent.
    Abar = r1 r2 a, d = r2 b, Bbar = r1 d - e Abar; the witnesses are (-e, r1) over (Abar, d) and (-1 / r2, m_j) over (d, h_j).  blind: the blindings of
    -e, r1, -1 / r2, then one per message (used where it is hidden).  r2 != 0"""
    L = len(msgs)
    H = key.params_scalars(L)
    abar = r1 * r2 * a % R
    d = r2 * key.b(msgs) % R
    bbar = (r1 * d - e * abar) % R
    b1, b2, b3 = blind[:3]
    bl = blind[3:3 + L]
    mask = [1 if j in revealed else 0 for j in range(L)]
    t1 = (b1 * abar + b2 * d) % R
    t2 = (sum(bl[j] * H[1 + j] for j in range(L) if not mask[j]) + b3 * d) % R
    fixed = [b1 - e * c, b2 + r1 * c, b3 - inv(r2) * c]
    values = [msgs[j] if mask[j] else bl[j] + msgs[j] * c for j in range(L)]
    return Proof(CDL, [abar, bbar, d, t1, t2], fixed, values, mask, c)


def prove_ietf(key, a, e, msgs, revealed, r, blind, c):
    """proof_23_ietf's init and gen_proof: Abar = r a, Bbar = r b - e Abar; the witnesses are (-e / r, -1 / r) over (Abar, Bbar) and m_j over h_j.
    blind: the blindings of -e / r, -1 / r, then one per message.  r != 0"""
    L = len(msgs)
    H = key.params_scalars(L)
    abar = r * a % R
    bbar = (r * key.b(msgs) - e * abar) % R
    ba, bb = blind[:2]
    bl = blind[2:2 + L]
    mask = [1 if j in revealed else 0 for j in range(L)]
    t = (sum(bl[j] * H[1 + j] for j in range(L) if not mask[j]) + ba * abar + bb * bbar) % R
    ri = inv(r)
    fixed = [ba - e * ri * c, bb - ri * c]
    values = [msgs[j] if mask[j] else bl[j] + msgs[j] * c for j in range(L)]
    return Proof(IETF, [abar, bbar, t], fixed, values, mask, c)


def weights(kind, rho, i):
    """(u_i, v_i, t_i): CDL (rho^(2i), rho^(2i+1), rho^i); IETF (rho^i, rho^i, rho^i)"""
    t = pow(rho, i, R)
    if kind == IETF:
        return t, t, t
    u = t * t % R
    return u, u * rho % R, t


def batch(key, proofs, rho, i0=0):
    """(C, wts, tp, tn) of the proofs i0 .. of a batch: C_0 = sum w c, C_j = sum w y_j with w = v (CDL) or u (IETF); wts[i] the weights of proof i over its own
    points as uploaded; tp[i] = rho^i, tn[i] = -rho^i"""
    L = len(proofs[0].values) if proofs else 0
    C = [0] * (L + 1)
    wts, tp, tn = [], [], []
    for k, p in enumerate(proofs):
        u, v, t = weights(p.kind, rho, i0 + k)
        for j, y in enumerate(p.row()):
            C[j] = (C[j] + v * y) % R
        if p.kind == CDL:
            z1, z2, z3 = p.fixed
            wts.append([u * z1 % R, (R - u * p.c) % R, (u * z2 + v * z3) % R, (R - u) % R, (R - v) % R])
        else:
            wts.append([u * p.fixed[0] % R, u * p.fixed[1] % R, (R - u) % R])
        tp.append(t)
        tn.append((R - t) % R)
    return C, wts, tp, tn


def batch_verdict(key, proofs, rho):
    """what the ..._verify_batch_g1 calls decide: no Abar the identity, the one G1 equation, the merged pairing — in the exponent"""
    if not proofs:
        return True
    if any(p.pts[0] == 0 for p in proofs):
        return False
    C, wts, tp, _ = batch(key, proofs, rho)
    H = key.params_scalars(len(proofs[0].values))
    g = sum(c * h for c, h in zip(C, H)) + sum(w * q for p, ws in zip(proofs, wts) for w, q in zip(ws, p.pts))
    pairing = sum(t * (key.x * p.pts[0] - p.pts[1]) for p, t in zip(proofs, tp))
    return g % R == 0 and pairing % R == 0
