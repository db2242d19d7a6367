"""Big-integer model of the SAVER calls of crypto_amd/csrc/dock_saver.hip (dgpu_saver_*).  Key material from known discrete logs: g_j = a_j G and
delta_g = d G over the generator G of G1, H = h G2 over the generator G2 of G2, and the keys of saver/src/keygen.rs:256-299 from chosen rho, s, t, v:
    X_0 = delta_g, X_j = s_j delta_g, Y_j = t_j g_j, Z_j = t_j H (j = 0 .. K), P_1 = (t_0 + sum_j s_j t_j) delta_g
    V_0 = rho H, V_1_j = s_j v_j H, V_2_j = rho v_j H
(chunks j = 1 .. K here; s, v are lists of K values for them, t one of K + 1).  A G1 point is its log over G, a G2 point its log over G2, a GT element its
log over e(G, G2), and every check of the reference (saver/src/encryption.rs) is decided in the exponent.  Plain Python integers modulo r: nothing here shares
code with the library."""

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def inv(v):
    return pow(v % R, R - 2, R)


# ---- utils.rs:12-73 --------------------------------------------------------------------------------------------------------------------------------------
def decompose(value, b):
    """the chunks of a scalar, big-endian (decompose): 64, 32 or 16 of them"""
    by = (value % R).to_bytes(32, "big")
    if b == 4:
        return [c for x in by for c in (x >> 4, x & 15)]
    if b == 8:
        return list(by)
    if b == 16:
        return [(by[i] << 8) + by[i + 1] for i in range(0, 32, 2)]
    raise ValueError("UnexpectedBase(%d)" % b)


def compose(chunks, b):
    """the scalar of big-endian chunks, mod r (compose); every chunk is cut to its b bits the way the reference's `as u8` casts cut it"""
    if b not in (4, 8, 16):
        raise ValueError("UnexpectedBase(%d)" % b)
    if b == 4 and len(chunks) % 2:
        raise ValueError("InvalidDecomposition")
    if b == 4:
        by = [((chunks[i] << 4) + chunks[i + 1]) & 255 for i in range(0, len(chunks), 2)]
    elif b == 8:
        by = [c & 255 for c in chunks]
    else:
        by = [x for c in chunks for x in ((c >> 8) & 255, c & 255)]
    return int.from_bytes(bytes(by), "big") % R


class Key:
    def __init__(self, a, d, h, rho, s, t, v, b):
        K = len(a)
        assert len(s) == K and len(v) == K and len(t) == K + 1
        self.K, self.b, self.E = K, b, (1 << b) - 1
        self.a, self.d, self.h, self.rho = [x % R for x in a], d % R, h % R, rho % R
        self.s, self.t, self.v = [x % R for x in s], [x % R for x in t], [x % R for x in v]

    # logs over G2
    def H(self):
        return self.h

    def V_0(self):
        return self.rho * self.h % R

    def V_1(self):
        return [s * v * self.h % R for s, v in zip(self.s, self.v)]

    def V_2(self):
        return [self.rho * v * self.h % R for v in self.v]

    def Z(self):
        return [t * self.h % R for t in self.t]

    def commitment_g2(self):
        """[Z_0 .. Z_K, H]: the G2 side of the commitment checks, in the order of all_pc"""
        return self.Z() + [self.h]

    # logs over e(G, G2)
    def base(self, j):
        """e(g_j, V_2_j)"""
        return self.a[j] * self.V_2()[j] % R

    def power(self, j, m):
        """T_j[m]"""
        return m * self.base(j) % R

    def encrypt(self, msgs, r):
        """the ciphertext row [c_0, c_1 .. c_K, psi] of ANY scalar vector (encryption.rs:627-663, not only legal chunks)"""
        r %= R
        c0 = r * self.d % R
        c = [(r * s * self.d + m * a) % R for s, m, a in zip(self.s, msgs, self.a)]
        p1 = (self.t[0] + sum(s * t for s, t in zip(self.s, self.t[1:]))) * self.d % R
        psi = (sum(m * t * a for m, t, a in zip(msgs, self.t[1:], self.a)) + r * p1) % R
        return [c0] + c + [psi]

    def pairing_values(self, row, second=None):
        """the logs of p_j = e(c_j, V_2_j) e(second, V_1_j); second defaults to -rho c_0"""
        sec = (R - self.rho * row[0]) % R if second is None else second % R
        V1, V2 = self.V_1(), self.V_2()
        return [(row[1 + j] * V2[j] + sec * V1[j]) % R for j in range(self.K)]

    def find(self, j, p):
        """the chunk m <= E with T_j[m] = p, or None (0 for one first, then the lowest m: the reference's walk)"""
        if p % R == 0:
            return 0
        base = self.base(j)
        if base == 0:
            return None
        m = p * inv(base) % R
        return m if 1 <= m <= self.E else None

    def decrypt(self, row):
        """(status, chunks, nu): 0 and the chunks, or 1 (CouldNotFindDiscreteLog) and zeros; nu = rho c_0"""
        found = [self.find(j, p) for j, p in enumerate(self.pairing_values(row))]
        nu = self.rho * row[0] % R
        if any(m is None for m in found):
            return 1, [0] * self.K, nu
        return 0, found, nu

    def decryption_verifies(self, row, chunks, nu):
        """verify_decryption (encryption.rs:425-469) in the exponent, the reference's own two conditions"""
        nu %= R
        if (-nu * self.h + row[0] * self.V_0()) % R:
            return False
        V1, V2 = self.V_1(), self.V_2()
        return all(m <= self.E and ((m * self.a[j] - row[1 + j]) * V2[j] + nu * V1[j]) % R == 0 for j, m in enumerate(chunks))

    def nu_for_chunk_columns_only(self, row, chunks):
        """a nu that satisfies every chunk column for `chunks` but not the V_0 check, when one exists (K = 1, or all columns agree): solves column 0"""
        V1, V2 = self.V_1(), self.V_2()
        return (row[1] - chunks[0] * self.a[0]) * V2[0] % R * inv(V1[0]) % R

    def commitment_verifies(self, row):
        g2 = self.commitment_g2()
        return (sum(p * q for p, q in zip(row[:-1], g2[:-1])) - row[-1] * g2[-1]) % R == 0

    def batch_verifies(self, rows, weights):
        """verify_commitments_in_batch: the K + 2 column sums against [Z_0 .. Z_K, H], the last negated"""
        if not rows:
            return True
        g2 = self.commitment_g2()
        total = 0
        for k in range(self.K + 2):
            col = sum(w * row[k] for w, row in zip(weights, rows)) % R
            total += (R - col if k == self.K + 1 else col) * g2[k]
        return total % R == 0
