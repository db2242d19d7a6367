"""Big-integer model of the range-proof calls of crypto_amd/csrc/dock_smc.hip (dgpu_smc_range_proofs_verify_each_g1 / _verify_batch_g1) and of the scalar kernels
in front of them (smc_kernels.hip.h), in the manner of acc_pok_model.py: with g1 = gamma G, g = kg G, h = kh G and pk = alpha g2, every point of a
CLSRangeProof / CCSArbitraryRangeProof (smc_range_proof/src/cls_range_proof/range_proof_cdh.rs, ccs_range_proof/arbitrary_range_cdh.rs) is a known multiple of
G, so the reference's checks can be decided in the exponent.  The statement rules (cls_range_proof/util.rs, ccs_range_proof/util.rs) are written out here a
second time, from the reference: nothing here shares code with the library."""
from bbs_model import R

CLS, CCS = 1, 2            # = the number of sides


def inv(v):
    return pow(v % R, R - 2, R)


# ---- the statement: cls_range_proof/util.rs and ccs_range_proof/util.rs ------------------------------------------------------------------------------
def range_and_rm(base, min_, max_):
    """get_range_and_randomness_multiple(base, min, max)"""
    rng, rm = max_ - min_, 1
    if rng % (base - 1) != 0:
        rng *= base - 1
        rm *= base - 1
    return rng, rm


def ilog(x, b):
    l = 0
    while b ** (l + 1) <= x:
        l += 1
    return l


def find_number_of_digits(rng, base):
    l = ilog(rng + 1, base)
    if base ** l < rng + 1:
        l += 1
    return l


def digits_of(value, base):
    d = []
    while value:
        d.append(value % base)
        value //= base
    return d


def find_sumset_boundaries(rng, base, num):
    if base == 2:
        return [(rng + (1 << i)) >> (i + 1) for i in range(num)]
    h = digits_of(rng, base)
    g = []
    for i in range(num):
        h_hat = rng // base ** (i + 1)
        g.append(h_hat + (1 + h[i] + sum(h[:i]) % (base - 1)) // base)
    return g


def decompose_for_sumset(value, G, base):
    out, target = [0] * len(G), value
    for i, g in enumerate(G):
        for u in range(base - 1, 0, -1):
            if target >= g * u:
                out[i] = u
                target -= g * u
                break
    assert target == 0, (value, G, base)
    return out


def find_l_for_arbitrary_range(max_, min_, base):
    diff = max_ - min_
    l = ilog(diff, base)
    return l if base ** l > diff else l + 1


class Statement:
    """(kind, min, max, base) -> sides, l, the weights w_j and per side (a, b, e):  a c C + (b c + sum_j w_j z2_j) g + e zr h = D"""

    def __init__(self, kind, min_, max_, base):
        assert min_ < max_
        self.kind, self.sides, self.min, self.max, self.base = kind, kind, min_, max_, base
        if kind == CLS:
            self.range, self.rm = range_and_rm(base, min_, max_ - 1)
            self.l = find_number_of_digits(self.range, base)
            self.G = find_sumset_boundaries(self.range, base, self.l)
            self.w = [g % R for g in self.G]
            self.consts = [((R - self.rm) % R, min_ * self.rm % R, self.rm)]
        else:
            self.l = find_l_for_arbitrary_range(max_, min_, base)
            self.w = [pow(base, j, R) for j in range(self.l)]
            self.consts = [(R - 1, min_ % R, 1), (R - 1, (R - (base ** self.l - max_)) % R, 1)]
        self.D, self.M = self.sides * self.l, self.sides * (self.l + 1)

    @classmethod
    def raw(cls, sides, l, w, consts):
        """a statement from its constants alone (what the calls are handed): any weights, any (a, b, e)"""
        st = cls.__new__(cls)
        st.kind = st.sides = sides
        st.l, st.w, st.consts = l, [v % R for v in w], [tuple(v % R for v in t) for t in consts]
        st.D, st.M = sides * l, sides * (l + 1)
        return st

    def as_tuple(self):
        return self.sides, self.l, list(self.w), list(self.consts)

    def digits(self, value):
        """the prover's digits, side-major: CLS get_sumset_parameters; CCS the base-n digits of value - min, then of value + base^l - max"""
        assert self.min <= value < self.max
        if self.kind == CLS:
            return [decompose_for_sumset((value - self.min) * self.rm, self.G, self.base)]
        pad = lambda v: (digits_of(v, self.base) + [0] * self.l)[:self.l]
        return [pad(value - self.min), pad(value + self.base ** self.l - self.max)]

    def ref_position(self, d):
        """where digit d (side-major) stands in the order the reference verifies them"""
        return d if self.sides == 1 else 2 * (d % self.l) + d // self.l


class Key:
    """the logs of everything the verifier holds: pk = alpha g2, g1 = gamma G, the commitment key g = kg G, h = kh G"""

    def __init__(self, alpha, gamma, kg, kh):
        self.alpha, self.gamma, self.kg, self.kh = alpha % R, gamma % R, kg % R, kh % R

    def sig(self, m):
        """the weak-BB signature on m: g1 / (alpha + m)"""
        return self.gamma * inv(self.alpha + m) % R


class Digit:
    """one PoKOfSignatureG1Proof: the logs of A', Abar, T and the responses z1, z2"""

    def __init__(self, ap, abar, t, z1, z2):
        self.ap, self.abar, self.t, self.z1, self.z2 = ap % R, abar % R, t % R, z1 % R, z2 % R

    def copy(self):
        return Digit(self.ap, self.abar, self.t, self.z1, self.z2)


def prove_digit(key, m, r, b_r, b_m, c, sig=None):
    """PoKOfSignatureG1Protocol::init_with_given_randomness and gen_proof (weak_bb_sig_pok_cdh.rs:72-117) for the signature `sig` (a log) on m — sig need not be
    g1 / (alpha + m): then everything but the pairing stays consistent.  r: sig_randomizer, b_m: msg_blinding, b_r: sc_blinding"""
    a = key.sig(m) if sig is None else sig
    ap = r * a % R
    abar = (r * key.gamma - m * ap) % R
    t = (b_r * key.gamma - b_m * ap) % R
    return Digit(ap, abar, t, b_r + c * r, b_m + c * m)


class Proof:
    """One proof as logs and scalars: C, c, per side D[s] and zr[s], and the digits side-major.  Plain fields: a test tampers with them in place."""

    def __init__(self, C, c, D, zr, digits):
        self.C, self.c, self.D, self.zr, self.digits = C % R, c % R, [v % R for v in D], [v % R for v in zr], digits

    def copy(self):
        return Proof(self.C, self.c, self.D, self.zr, [d.copy() for d in self.digits])

    def own(self, st):
        """the own scalars of the M equations, four each: sides first, then the digits"""
        n = lambda v: (R - v % R) % R
        out = []
        for s, (a, b, e) in enumerate(st.consts):
            ip = sum(w * d.z2 for w, d in zip(st.w, self.digits[s * st.l:(s + 1) * st.l]))
            out += [a * self.c % R, (b * self.c + ip) % R, e * self.zr[s] % R, R - 1]
        for d in self.digits:
            out += [d.z1, n(d.z2), n(self.c), R - 1]
        return out

    def bases(self, key, st):
        """the logs of the bases, in the order of own()"""
        out = []
        for s in range(st.sides):
            out += [self.C, key.kg, key.kh, self.D[s]]
        for d in self.digits:
            out += [key.gamma, d.ap, d.abar, d.t]
        return out

    def equations(self, key, st):
        own, bases = self.own(st), self.bases(key, st)
        return [sum(own[4 * m + t] * bases[4 * m + t] for t in range(4)) % R == 0 for m in range(st.M)]

    def pairing_errors(self, key):
        """alpha A' - Abar per digit, in the exponent: zero iff e(A', pk) e(-Abar, g2) = 1"""
        return [(key.alpha * d.ap - d.abar) % R for d in self.digits]

    def status(self, key, st, random=None):
        """(status, detail) in the reference's order of errors.  random: the merged form — ONE two-pair check with the weights random^q in the order of
        add_sources (side-major), a failure of which is (3, 0)"""
        eq = self.equations(key, st)
        for s in range(st.sides):
            if not eq[s]:
                return 1, s + 1
        perr = self.pairing_errors(key)
        best = 0
        for d, dg in enumerate(self.digits):
            k = 1 if dg.ap == 0 else 2 if not eq[st.sides + d] else 3 if random is None and perr[d] else 0
            if k and (not best or 4 * st.ref_position(d) + k < best):
                best = 4 * st.ref_position(d) + k
        if best:
            return 2, best
        if random is not None and sum(pow(random, q, R) * e for q, e in enumerate(perr)) % R:
            return 3, 0
        return 0, 0


def prove(key, st, value, rand, c, blind, other_key=False):
    """CLSRangeProofProtocol / CCSArbitraryRangeProofProtocol::init_given_base and gen_proof for C = value g + rand h.  blind(k) gives the k-th blinding
    (any deterministic source): per side m, then per digit msg_blinding, sig_randomizer, sc_blinding.  other_key: every digit's signature is one under the
    key alpha + 1 — the Schnorr proofs stay consistent, the pairings fail"""
    C = (value * key.kg + rand * key.kh) % R
    D, zr, digits, k = [], [], [], 0
    for s, side in enumerate(st.digits(value)):
        m = blind(k); k += 1
        mb = [blind(k + j) for j in range(st.l)]; k += st.l
        e = st.consts[s][2]
        D.append((sum(w * b for w, b in zip(st.w, mb)) * key.kg + m * e * key.kh) % R)
        zr.append((m + rand * c) % R)
        for j, dg in enumerate(side):
            r, b_r = blind(k) or 1, blind(k + 1); k += 2
            digits.append(prove_digit(key, dg, r, b_r, mb[j], c, sig=key.gamma * inv(key.alpha + 1 + dg) % R if other_key else None))
    return Proof(C, c, D, zr, digits)


def tamper(p, what, d=0, s=0, forged=None, delta=1):
    """a copy of p with one thing wrong.  D: D_s + G (1, s + 1); A_identity: A'_d = O (k = 1); z1: z1_d + 1 (k = 2); forged: digit d from `forged`, the same proof
    made with other_key (k = 3); shift: Abar_d + delta g1 with T_d moved so that the Schnorr check still holds (k = 3: the pairing alone is off, by -delta gamma)"""
    q = p.copy()
    if what == "D":
        q.D[s] = (q.D[s] + 1) % R
    elif what == "A_identity":
        q.digits[d].ap = 0
    elif what == "z1":
        q.digits[d].z1 = (q.digits[d].z1 + 1) % R
    elif what == "forged":
        q.digits[d] = forged.digits[d].copy()
    elif what == "shift":
        q.digits[d].abar = (q.digits[d].abar + delta) % R
        q.digits[d].t = (q.digits[d].t - q.c * delta) % R
    else:
        raise KeyError(what)
    return q


# ---- the batch ------------------------------------------------------------------------------------------------------------------------------------------
def batch(st, proofs, rho, i0=0):
    """(S, w_side, w_digit, tp, tn) of the proofs i0 .. of a batch.  Equation m of proof i weighs u = rho^(i M + m), slice i D + d weighs rho^(i D + d).
    S: the coefficients of g1, g, h; w_side: over C_i (n of them), then over D_is; w_digit: over A', Abar, T per slice; tp, tn: +- the slices' weights"""
    S = [0, 0, 0]
    wc, wd, wdig, tp, tn = [], [], [], [], []
    for k, p in enumerate(proofs):
        i = i0 + k
        own = p.own(st)
        u = [pow(rho, i * st.M + m, R) for m in range(st.M)]
        wc.append(sum(u[s] * own[4 * s] for s in range(st.sides)) % R)
        for s in range(st.sides):
            S[1] = (S[1] + u[s] * own[4 * s + 1]) % R
            S[2] = (S[2] + u[s] * own[4 * s + 2]) % R
            wd.append(u[s] * own[4 * s + 3] % R)
        for d in range(st.D):
            m = st.sides + d
            S[0] = (S[0] + u[m] * own[4 * m]) % R
            wdig += [u[m] * own[4 * m + t] % R for t in (1, 2, 3)]
            t = pow(rho, i * st.D + d, R)
            tp.append(t)
            tn.append((R - t) % R)
    return S, wc + wd, wdig, tp, tn


def batch_verdict(key, st, proofs, rho):
    """what the batch call decides: no A' the identity, the one G1 equation, the merged pairing — in the exponent"""
    if any(d.ap == 0 for p in proofs for d in p.digits):
        return False
    S, ws, wdig, tp, _ = batch(st, proofs, rho)
    n = len(proofs)
    g = S[0] * key.gamma + S[1] * key.kg + S[2] * key.kh
    g += sum(w * p.C for w, p in zip(ws[:n], proofs)) + sum(w * q for w, q in zip(ws[n:], [v for p in proofs for v in p.D]))
    g += sum(w * q for w, q in zip(wdig, [v for p in proofs for d in p.digits for v in (d.ap, d.abar, d.t)]))
    pairing = sum(t * e for t, e in zip(tp, [e for p in proofs for e in p.pairing_errors(key)]))
    return g % R == 0 and pairing % R == 0
