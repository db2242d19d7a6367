"""Big-integer model of the BBS+ calls of crypto_amd/csrc/dock_bbs.hip and of the scalar kernels in front of them (bbs_kernels.hip.h): the rows of the many-row
MSM, the column sums of the batch verifier and, for key material made from known discrete logs, the signatures themselves as multiples of the group's generator.
Plain Python integers modulo r: nothing here shares code with the library."""

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def row(s, msgs, mult=1):
    """row of the many-row MSM for one signature: mult (1, s, m_1 .. m_L)"""
    return [mult * v % R for v in [1, s] + list(msgs)]


def inverses(x, es):
    """(t_i, zero_i): t_i = 1 / (x + e_i), or (0, True) where x + e_i = 0"""
    out = []
    for e in es:
        u = (x + e) % R
        out.append((0, True) if u == 0 else (pow(u, R - 2, R), False))
    return out


def sign_rows(x, es, ss, msgs):
    """the rows of dgpu_bbs_plus_sign_many_g1: t_i (1, s_i, m_i ..)"""
    return [row(s, m, t) for (t, _), s, m in zip(inverses(x, es), ss, msgs)]


def columns(rho, es, ss, msgs, i0=0):
    """(c, weights, weights times e) of the rows i0 .. of a batch: c_k = sum_i rho^(i0 + i) row_ik"""
    n = len(ss)
    L = len(msgs[0]) if n else 0
    c = [0] * (L + 2)
    w = pow(rho, i0, R)
    wts, we = [], []
    for i in range(n):
        for k, v in enumerate(row(ss[i], msgs[i])):
            c[k] = (c[k] + w * v) % R
        wts.append(w); we.append(w * es[i] % R)
        w = w * rho % R
    return c, wts, we


class Key:
    """key material from known discrete logs over the generator G of G1: g1 = gamma G, h_k = eta_k G (eta_0 for h_0), the secret key x"""
    def __init__(self, x, gamma, etas):
        self.x, self.gamma, self.etas = x % R, gamma % R, [v % R for v in etas]

    def params_scalars(self, L):
        return [self.gamma] + self.etas[:L + 1]

    def b(self, s, msgs):
        """log_G of b = g1 + s h_0 + sum m_j h_j"""
        return sum(v * h for v, h in zip(row(s, msgs), self.params_scalars(len(msgs)))) % R

    def a(self, e, s, msgs):
        """log_G of A = b / (x + e), or None where no signature exists (x + e = 0, or b the identity)"""
        u, b = (self.x + e) % R, self.b(s, msgs)
        if u == 0 or b == 0:
            return None
        return b * pow(u, R - 2, R) % R

    def d(self, a, e, s, msgs):
        """log_G of e A - b for a signature A = a G"""
        return (e * a - self.b(s, msgs)) % R

    def verifies(self, a, e, s, msgs):
        """SignatureG1::verify in the exponent: A != O and x a + e a - b = 0"""
        return a % R != 0 and (self.x * a + self.d(a, e, s, msgs)) % R == 0
