"""Big-integer model of the four PS (Coconut) calls of crypto_amd/csrc/dock_ps.hip (dgpu_ps_*) and of the scalar kernels in front of them
(ps_kernels.hip.h).  Key material from known discrete logs: g = gamma G over the generator G of G1; g_tilde = gamma' G2, alpha_tilde = x g_tilde,
beta_tilde_j = y_j g_tilde over the generator G2 of G2.  A G1 point is its log over G, a G2 point its log over G2, and every check of the reference
(coconut/src/signature/ps_signature.rs, proof/signature_pok/) is decided in the exponent: e(a G, b G2) e(-c G, d G2) = 1 iff a b = c d.  Plain Python
integers modulo r: nothing here shares code with the library."""

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def inv(v):
    return pow(v % R, R - 2, R)


# ---- the scalar kernels ----------------------------------------------------------------------------------------------------------------------------------
def sign_scalars(x, ys, r, msgs):
    """k_ps_sign_rows for one row: (r, u) with u = r (x + sum_j y_j m_j)"""
    return r % R, r * (x + sum(y * m for y, m in zip(ys, msgs))) % R


def verify_row(msgs):
    """the row of the many-row G2 MSM over pk[0 .. L]: (1, m_1 .. m_L)"""
    return [1] + [m % R for m in msgs]


def col_scalars(rho, msgs, i0=0):
    """k_ps_col_scalars over the rows i0 .. of a batch: the L + 2 columns — w_i = rho^(i0 + i); w_i m_ij; -w_i — each a list over the rows"""
    n = len(msgs)
    L = len(msgs[0]) if n else 0
    w = [pow(rho, i0 + i, R) for i in range(n)]
    return [w] + [[w[i] * msgs[i][j] % R for i in range(n)] for j in range(L)] + [[(R - v) % R for v in w]]


class Key:
    """sk = (x, y_1 ..); g = gamma G; g_tilde = gamma' G2, alpha_tilde = x g_tilde, beta_tilde_j = y_j g_tilde"""
    def __init__(self, x, ys, gamma, gamma_t):
        self.x, self.ys, self.gamma, self.gamma_t = x % R, [y % R for y in ys], gamma % R, gamma_t % R

    def sk(self, L):
        return [self.x] + self.ys[:L]

    def pk_scalars(self, L):
        """the logs over G2 of the handle [alpha_tilde, beta_tilde_1 .. beta_tilde_L, g_tilde]"""
        return [self.gamma_t * v % R for v in [self.x] + self.ys[:L] + [1]]

    def exponent(self, msgs):
        """x + sum_j y_j m_j"""
        return (self.x + sum(y * m for y, m in zip(self.ys, msgs))) % R

    def sign(self, r, msgs):
        """Signature::new with r for its draw: the logs over G of (sigma_1, sigma_2) = (r g, (r (x + sum y_j m_j)) g)"""
        s1, u = sign_scalars(self.x, self.ys[:len(msgs)], r, msgs)
        return s1 * self.gamma % R, u * self.gamma % R

    def q(self, msgs):
        """log over G2 of alpha_tilde + sum_j m_j beta_tilde_j"""
        return sum(a * b for a, b in zip(verify_row(msgs), self.pk_scalars(len(msgs)))) % R

    def verifies(self, sig, msgs):
        """Signature::verify in the exponent: no element the identity and sigma_1 q = sigma_2 gamma'"""
        s1, s2 = sig
        return s1 % R != 0 and s2 % R != 0 and (s1 * self.q(msgs) - s2 * self.gamma_t) % R == 0

    def batch_verifies(self, sigs, msgs, rho):
        """dgpu_ps_verify_batch in the exponent: no element the identity and the L + 2 pairs' exponents add up to zero"""
        if not sigs:
            return True
        if any(s1 % R == 0 or s2 % R == 0 for s1, s2 in sigs):
            return False
        L = len(msgs[0])
        cols, pk = col_scalars(rho, msgs), self.pk_scalars(L)
        total = 0
        for k in range(L + 2):
            side = sum(c * (s[1] if k == L + 1 else s[0]) for c, s in zip(cols[k], sigs))
            total += side * pk[k]
        return total % R == 0


# ---- proofs of knowledge -------------------------------------------------------------------------------------------------------------------------------------
class Proof:
    """One SignaturePoK as logs and scalars: sig = [sigma_1', sigma_2'] over G; k, t over G2; values[j] the revealed message or the response of the hidden
    message j; mask[j] = 1 where j is revealed; z_r the last response (over g_tilde); c the challenge.  Plain lists: a test tampers with them in place."""

    def __init__(self, sig, k, t, values, mask, z_r, c):
        self.sig, self.k, self.t = [v % R for v in sig], k % R, t % R
        self.values, self.mask, self.z_r, self.c = [v % R for v in values], list(mask), z_r % R, c % R

    def copy(self):
        return Proof(self.sig, self.k, self.t, self.values, self.mask, self.z_r, self.c)

    def rows(self):
        """k_ps_pok_rows: (S, R), S = (0, hidden ? z : 0 .., z_r), R = (1, revealed ? m : 0 .., 0)"""
        return ([0] + [0 if m else v for v, m in zip(self.values, self.mask)] + [self.z_r], [1] + [v if m else 0 for v, m in zip(self.values, self.mask)] + [0])

    def checks(self, key):
        """(Schnorr, no identity element, pairing) in the exponent"""
        pk = key.pk_scalars(len(self.values))
        S, Rr = (sum(a * b for a, b in zip(row, pk)) % R for row in self.rows())
        schnorr = (S - self.c * self.k - self.t) % R == 0
        pairing = (self.sig[0] * (Rr + self.k) - self.sig[1] * key.gamma_t) % R == 0
        return schnorr, self.sig[0] != 0 and self.sig[1] != 0, pairing

    def status(self, key):
        """0, or the first error the reference returns (proof.rs:46-55: proof_res.and(sig_res)): 3 the Schnorr check, 1 ZeroSignature, 4 the pairing"""
        schnorr, nonzero, pairing = self.checks(key)
        return 3 if not schnorr else 1 if not nonzero else 4 if not pairing else 0


def status_of(schnorr_ok, s1_inf, s2_inf, pairing_ok):
    """ps_kernels.hip.h status_of: 3 over 1 over 4"""
    return 3 if not schnorr_ok else 1 if (s1_inf or s2_inf) else 4 if not pairing_ok else 0


def prove(key, sig, msgs, revealed, r, r_bar, blind, c):
    """SignaturePoK as the reference builds it, for the signature `sig` (logs; it need not verify: then everything but the pairing stays consistent):
    RandomizedSignature::new(sig, r, r_bar) = (r_bar sigma_1, r_bar sigma_2 + r r_bar sigma_1); K::new over the hidden messages, k = sum_hidden m_j beta_tilde_j
    + r g_tilde; the Schnorr commitment t = sum_hidden b_j beta_tilde_j + b_r g_tilde and the responses b + c witness.  blind: one blinding per message (used
    where it is hidden), then b_r"""
    L = len(msgs)
    pk = key.pk_scalars(L)
    mask = [1 if j in revealed else 0 for j in range(L)]
    s1 = r_bar * sig[0] % R
    s2 = (r_bar * sig[1] + r * s1) % R
    k = (sum(msgs[j] * pk[1 + j] for j in range(L) if not mask[j]) + r * pk[L + 1]) % R
    t = (sum(blind[j] * pk[1 + j] for j in range(L) if not mask[j]) + blind[L] * pk[L + 1]) % R
    values = [msgs[j] if mask[j] else blind[j] + c * msgs[j] for j in range(L)]
    return Proof([s1, s2], k, t, values, mask, blind[L] + c * r, c)
