"""Small R1CS circuits and assignment rows for the many-row witness map's tests (test_witness_map_many_device_code_on_host.py on the host,
test_gpu_witness_map_many.py on the device): every domain from 2 to 2^11, the shapes at which the block kernel can go wrong, and the oracle's h for
them.  Not a test module."""
import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def limbs(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def to_words(vals):
    return np.array([limbs(v) for v in vals], dtype=np.uint64).reshape(-1, 4)


def csr(rows):
    rp, cols, vals = [0], [], []
    for row in rows:
        for co, idx in row:
            cols.append(idx); vals.append(limbs(co))
        rp.append(len(cols))
    return (np.array(rp, dtype=np.uint64), np.array(cols, dtype=np.uint32), np.array(vals, dtype=np.uint64).reshape(-1, 4))


class Circuit:
    """A, B, C as lists of rows [(coeff, var), ...]; z0 an assignment that satisfies it (z0[0] = 1)"""

    def __init__(self, rows_a, rows_b, rows_c, num_vars, num_inputs, z0=None):
        self.rows = (rows_a, rows_b, rows_c)
        self.mats = tuple(csr(r) for r in self.rows)
        self.num_vars, self.num_inputs, self.num_constraints = num_vars, num_inputs, len(rows_a)
        self.z0 = z0
        D = 2
        while D < self.num_constraints + num_inputs:
            D *= 2
        self.D, self.logn = D, D.bit_length() - 1

    def args(self):
        """the twelve matrix arguments of dgpu_r1cs_upload / the shim, as (array, ...) kept alive by the caller"""
        return self.mats


def dot(row, z):
    return sum(co * z[v] for co, v in row) % R


def random_circuit(seed, num_constraints, num_inputs, num_vars, terms=3, empty_row=None, dense_row=None):
    """`terms` non-zeros per row of A and B; C is one term per row whose coefficient makes z0 satisfy the row.  empty_row: that row of A, B and C has no
    term.  dense_row: that row of A, B and C holds num_vars terms of value r - 1 (the worst case for the lazy accumulation against z = r - 1)."""
    rng = np.random.default_rng(seed)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % R
    z0 = [1] + [rnd() or 1 for _ in range(num_vars - 1)]
    A, B, Cm = [], [], []
    for i in range(num_constraints):
        if i == empty_row:
            A.append([]); B.append([]); Cm.append([]); continue
        if i == dense_row:
            row = [(R - 1, v) for v in range(num_vars)]
            A.append(list(row)); B.append(list(row)); Cm.append(list(row)); continue
        ra = [(rnd(), int(rng.integers(num_vars))) for _ in range(terms)]
        rb = [(rnd(), int(rng.integers(num_vars))) for _ in range(terms)]
        v = int(rng.integers(num_vars))
        A.append(ra); B.append(rb); Cm.append([(dot(ra, z0) * dot(rb, z0) * pow(z0[v], R - 2, R) % R, v)])
    return Circuit(A, B, Cm, num_vars, num_inputs, z0)


def rows_for(circ, m, seed, kinds=("sat", "rand")):
    """m assignment rows (m, num_vars, 4) canonical: `sat` the satisfying z0, `rand` random (does not satisfy), `zero` all zeros, `max` all r - 1"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(m):
        k = kinds[j % len(kinds)]
        if k == "sat":
            out.append(to_words(circ.z0))
        elif k == "zero":
            out.append(np.zeros((circ.num_vars, 4), np.uint64))
        elif k == "max":
            out.append(to_words([R - 1] * circ.num_vars))
        else:
            out.append(to_words([int.from_bytes(rng.bytes(40), "little") % R for _ in range(circ.num_vars)]))
    return np.ascontiguousarray(np.stack(out))


def oracle_h(circ, rows):
    """(m, D, 4) canonical: the oracle's witness map of every row"""
    import oracle_c as O
    return np.stack([O.witness_map(circ.mats, rows[j], circ.num_inputs, circ.num_constraints) for j in range(len(rows))])


def fill_exact(seed, logn, **kw):
    """num_constraints + num_inputs = D exactly"""
    D = 1 << logn
    ni = 1 if D == 2 else 2
    return random_circuit(seed, D - ni, ni, max(D - ni + 3, ni + 2), **kw)


def one_past(seed, logn, **kw):
    """num_constraints + num_inputs one past the previous power of two: the upper half of the domain is padding"""
    D = 1 << logn
    ni = 1 if D <= 4 else 2
    return random_circuit(seed, D // 2 + 1 - ni, ni, D // 2 + 4, **kw)
