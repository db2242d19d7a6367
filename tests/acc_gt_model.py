"""Big-integer model of the accumulator proof calls of crypto_amd/csrc/dock_acc_gt.hip (dgpu_accumulator_gt_membership_proofs_verify_each_g1 / _verify_batch_g1,
dgpu_accumulator_gt_non_membership_proofs_verify_each_g1 / _verify_batch_g1) and of the scalar kernels in front of them (acc_gt_kernels.hip.h), in the manner of
acc_pok_model.py: both provers and both verifiers of vb_accumulator/src/proofs.rs transcribed in the exponent.  With P = pi G, V = v G, pk = alpha P~, the
proving key X = x G, Y = yk G, Z = z G, K = k G and a witness C = w G, every G1 point of a MembershipProof / NonMembershipProof is a known multiple of G and
its GT element is R_E = e(G, P~)^re, where e(a G, P~) e(b G, pk) = e(G, P~)^(a + alpha b): the reference's checks can be decided in the exponent.  Plain Python
integers modulo r: nothing here shares code with the library."""
from bbs_model import R

MEM, NM = 0, 1
NPTS = {MEM: 7, NM: 11}
NRESP = {MEM: 5, NM: 8}
CHECKS = {MEM: 4, NM: 6}                       # J: Schnorr checks a proof; the pairing is check J + 1
SEG_ENDS = {MEM: [3, 6, 9, 12, 15, 17], NM: [4, 8, 11, 14, 17, 20, 25, 27]}
# points: E_C, T_sigma, T_rho, R_sigma, R_rho, R_delta_sigma, R_delta_rho [, E_d, E_d_inv, R_A, R_B]
E_C, T_SIGMA, T_RHO, R_SIGMA, R_RHO, R_DSIGMA, R_DRHO, E_D, E_D_INV, R_A, R_B = range(11)
# responses: s_sigma, s_rho, s_delta_sigma, s_delta_rho, s_y [, s_u, s_v, s_w]
S_SIGMA, S_RHO, S_DSIGMA, S_DRHO, S_Y, S_U, S_V, S_W = range(8)


def inv(v):
    return pow(v % R, R - 2, R)


def neg(v):
    return (R - v % R) % R


class Key:
    """the logs of everything the verifier holds: pk = alpha P~, P = pi G, V = v G, X = x G, Y = yk G, Z = z G, K = k G"""

    def __init__(self, alpha, pi, v, x, yk, z, k):
        self.alpha, self.pi, self.v, self.x, self.yk, self.z, self.k = (a % R for a in (alpha, pi, v, x, yk, z, k))

    def membership_witness(self, y):
        """C = v / (y + alpha) G"""
        return self.v * inv(y + self.alpha) % R

    def non_membership_witness(self, y, d):
        """(C, d) with C (y + alpha) + d P = V"""
        return (self.v - d * self.pi) * inv(y + self.alpha) % R

    def prk(self, kind):
        return [self.x, self.yk, self.z] + ([self.k] if kind == NM else [])


class Proof:
    """One proof as the logs of its points over G, the log of R_E over e(G, P~), and its scalars.  The fields are plain lists: a test tampers with them in
    place."""

    def __init__(self, kind, pts, re, resp, c):
        assert (len(pts), len(resp)) == (NPTS[kind], NRESP[kind])
        self.kind, self.pts, self.re, self.resp, self.c = kind, [v % R for v in pts], re % R, [v % R for v in resp], c % R

    def copy(self):
        return Proof(self.kind, self.pts, self.re, self.resp, self.c)

    def own(self):
        """the own scalars of the row's segments, in segment order (acc_gt_kernels.hip.h own_code)"""
        s, c = self.resp, self.c
        four = [s[S_SIGMA], neg(c), R - 1, s[S_RHO], neg(c), R - 1, s[S_Y], neg(s[S_DSIGMA]), R - 1, s[S_Y], neg(s[S_DRHO]), R - 1]
        p = [s[S_Y], neg(s[S_DSIGMA] + s[S_DRHO]), neg(c)]
        q = [neg(s[S_SIGMA] + s[S_RHO]), c]
        if self.kind == MEM:
            return four + p + q
        return [s[S_U], s[S_V], neg(c), R - 1, s[S_W], s[S_U], neg(c), R - 1] + four + p + [c, neg(s[S_V])] + q

    def bases(self, key, **kw):
        """the logs of the bases of the row's segments, in the order of own()"""
        v, pi, x, yk, z, k = (kw.get(n, getattr(key, n)) for n in ("v", "pi", "x", "yk", "z", "k"))
        t = self.pts
        four = [x, t[T_SIGMA], t[R_SIGMA], yk, t[T_RHO], t[R_RHO], t[T_SIGMA], x, t[R_DSIGMA], t[T_RHO], yk, t[R_DRHO]]
        p, q = [t[E_C], z, v], [z, t[E_C]]
        if self.kind == MEM:
            return four + p + q
        return [pi, k, t[E_D], t[R_A], k, t[E_D_INV], pi, t[R_B]] + four + p + [t[E_D], k] + q

    def segment_sums(self, key, **kw):
        """the logs of the sums of the row's segments: J Schnorr checks (zero iff the check holds), then p and q"""
        own, bases = self.own(), self.bases(key, **kw)
        out, lo = [], 0
        for hi in SEG_ENDS[self.kind]:
            out.append(sum(a * b for a, b in zip(own[lo:hi], bases[lo:hi])) % R)
            lo = hi
        return out

    def checks(self, key, **kw):
        """the reference's checks in its order, in the exponent; kw: what the verifier is handed instead of the key's own (v, pi, x, yk, z, k)"""
        sums = self.segment_sums(key, **kw)
        p, q = sums[-2:]
        return [s == 0 for s in sums[:-2]] + [(p + key.alpha * q - self.re) % R == 0]

    def status(self, key, **kw):
        """0, or the number of the first failing check"""
        for k, ok in enumerate(self.checks(key, **kw)):
            if not ok:
                return k + 1
        return 0


def prove_membership(key, w, y, sigma, rho, r_y, r_sigma, r_rho, r_dsigma, r_drho, c, extra=None):
    """ProofProtocol::randomize_witness_and_compute_commitments and compute_responses (proofs.rs:517-601, :656-675) for the witness w G of the element y — w need
    not be v / (y + alpha): then everything but the pairing stays consistent.  extra: (log of pairing_extra, the points and responses non-membership adds)"""
    e_c = (w + (sigma + rho) * key.z) % R
    t_sigma, t_rho = sigma * key.x % R, rho * key.yk % R
    d_sigma, d_rho = y * sigma % R, y * rho % R
    p = (r_y * e_c - (r_dsigma + r_drho) * key.z + (extra[0] if extra else 0)) % R
    q = neg((r_sigma + r_rho) * key.z)
    re = (p + key.alpha * q) % R
    pts = [e_c, t_sigma, t_rho, r_sigma * key.x, r_rho * key.yk, r_y * t_sigma - r_dsigma * key.x, r_y * t_rho - r_drho * key.yk]
    resp = [r_sigma + c * sigma, r_rho + c * rho, r_dsigma + c * d_sigma, r_drho + c * d_rho, r_y + c * y]
    if extra:
        return Proof(NM, pts + extra[1], re, resp + extra[2], c)
    return Proof(MEM, pts, re, resp, c)


def prove_non_membership(key, w, d, y, sigma, rho, r_y, r_sigma, r_rho, r_dsigma, r_drho, tau, pi_, r_u, r_v, r_w, c):
    """NonMembershipProofProtocol::init and gen_proof (proofs.rs:1090-1175, :1215-1245) for the witness (w G, d) of the element y, d != 0"""
    e_d = (d * key.pi + tau * key.k) % R
    e_d_inv = (inv(d) * key.pi + pi_ * key.k) % R
    r_a = (r_u * key.pi + r_v * key.k) % R
    r_b = (r_u * e_d_inv + r_w * key.k) % R
    cd = c * d % R
    resp = [r_u + cd, r_v + c * tau, r_w - cd * pi_]
    return prove_membership(key, w, y, sigma, rho, r_y, r_sigma, r_rho, r_dsigma, r_drho, c, extra=(neg(r_v * key.k), [e_d, e_d_inv, r_a, r_b], resp))


def weights(kind, rho, i):
    """([w_0 .. w_{J-1}], t): w_j = rho^(J i + j) on Schnorr check j of proof i, t = rho^i on its pairing and its R_E"""
    J = CHECKS[kind]
    return [pow(rho, J * i + j, R) for j in range(J)], pow(rho, i, R)


def batch(proofs, rho, i0=0):
    """(S, w, wp, wq, tp) of the proofs i0 .. of a batch: S the columns' coefficients — X, Y [P, K, X, Y] in the G1 equation, then Z, V [, K] in the side against
    P~ and Z in the side against pk, those negated — w[i] the weights of proof i over its own points, wp[i] = t s_y, wq[i] = t c, tp[i] = t"""
    if not proofs:
        return [], [], [], [], []
    kind = proofs[0].kind
    o = CHECKS[kind] - 4
    S = [0] * (5 if kind == MEM else 8)
    w, wp, wq, tp = [], [], [], []
    for k, p in enumerate(proofs):
        W, t = weights(kind, rho, i0 + k)
        s, c = p.resp, p.c
        g = []
        if kind == NM:
            g = [W[0] * s[S_U] - W[1] * c, W[0] * s[S_V] + W[1] * s[S_W]]
        g += [W[o] * s[S_SIGMA] - W[o + 2] * s[S_DSIGMA], W[o + 1] * s[S_RHO] - W[o + 3] * s[S_DRHO]]
        sides = [-t * (s[S_DSIGMA] + s[S_DRHO]), -t * c] + ([-t * s[S_V]] if kind == NM else []) + [-t * (s[S_SIGMA] + s[S_RHO])]
        S = [(a + b) % R for a, b in zip(S, g + sides)]
        row = [0, W[o + 2] * s[S_Y] - W[o] * c, W[o + 3] * s[S_Y] - W[o + 1] * c] + [neg(W[o + j]) for j in range(4)]
        if kind == NM:
            row += [neg(W[0] * c), W[1] * s[S_U], neg(W[0]), neg(W[1])]
        w.append([x % R for x in row])
        wp.append(t * s[S_Y] % R)
        wq.append(t * c % R)
        tp.append(t)
    return S, w, wp, wq, tp


def batch_verdict(key, proofs, rho, **kw):
    """what the batch calls decide, in closed form: the one G1 equation over all weighed Schnorr checks, and e(sum t p, P~) e(sum t q, pk) = prod R_E^t — in
    the exponent"""
    if not proofs:
        return True
    kind = proofs[0].kind
    v, pi, x, yk, z, k = (kw.get(n, getattr(key, n)) for n in ("v", "pi", "x", "yk", "z", "k"))
    S, w, wp, wq, tp = batch(proofs, rho)
    g1_shared = ([pi, k] if kind == NM else []) + [x, yk]
    ng = len(g1_shared)
    g = sum(s * b for s, b in zip(S, g1_shared)) + sum(a * b for p, ws in zip(proofs, w) for a, b in zip(ws, p.pts))
    p_shared = [z, v] + ([k] if kind == NM else [])
    pside = sum(s * b for s, b in zip(S[ng:], p_shared)) + sum(a * p.pts[E_C] for a, p in zip(wp, proofs))
    if kind == NM:
        pside += sum(a * p.pts[E_D] for a, p in zip(wq, proofs))
    qside = S[-1] * z + sum(a * p.pts[E_C] for a, p in zip(wq, proofs))
    gt = sum(t * p.re for t, p in zip(tp, proofs))
    return g % R == 0 and (pside + key.alpha * qside - gt) % R == 0


# ---- tampering (what the tests plant) ----
# every single tamper of a proof and the check it breaks — the status the reference's order of errors gives it.  A value is moved by one; `forged` is a proof made
# for a wrong witness (everything but the pairing stays consistent)
TAMPERS = {MEM: {"R_sigma": 1, "s_sigma": 1, "T_sigma": 1, "c": 1, "R_rho": 2, "s_rho": 2, "T_rho": 2, "R_delta_sigma": 3, "s_delta_sigma": 3, "s_y": 3,
                 "R_delta_rho": 4, "s_delta_rho": 4, "E_C": 5, "R_E": 5, "forged": 5},
           NM: {"R_A": 1, "s_u": 1, "s_v": 1, "E_d": 1, "c": 1, "R_B": 2, "s_w": 2, "E_d_inv": 2, "R_sigma": 3, "s_sigma": 3, "T_sigma": 3, "R_rho": 4, "s_rho": 4,
                "T_rho": 4, "R_delta_sigma": 5, "s_delta_sigma": 5, "s_y": 5, "R_delta_rho": 6, "s_delta_rho": 6, "E_C": 7, "R_E": 7, "forged": 7}}
POINTS = ["E_C", "T_sigma", "T_rho", "R_sigma", "R_rho", "R_delta_sigma", "R_delta_rho", "E_d", "E_d_inv", "R_A", "R_B"]
RESPS = ["s_sigma", "s_rho", "s_delta_sigma", "s_delta_rho", "s_y", "s_u", "s_v", "s_w"]


def prove_row(key, kind, y, d, rnd, c, forged=False):
    """rnd: sigma, rho, r_y, r_sigma, r_rho, r_delta_sigma, r_delta_rho [, tau, pi, r_u, r_v, r_w]"""
    if kind == MEM:
        return prove_membership(key, key.membership_witness(y) + (1 if forged else 0), y, *rnd[:7], c)
    return prove_non_membership(key, key.non_membership_witness(y, d) + (1 if forged else 0), d, y, *rnd[:12], c)


def tamper(p, what):
    """a copy of the proof with one value moved by one (`forged` is made by prove_row)"""
    p = p.copy()
    if what == "c":
        p.c = (p.c + 1) % R
    elif what == "R_E":
        p.re = (p.re + 1) % R
    elif what in POINTS:
        k = POINTS.index(what)
        p.pts[k] = (p.pts[k] + 1) % R
    else:
        k = RESPS.index(what)
        p.resp[k] = (p.resp[k] + 1) % R
    return p
