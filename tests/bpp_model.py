"""Big-integer model of the Bulletproofs++ calls of crypto_amd/csrc/dock_bpp.hip (dgpu_bpp_range_proofs_verify_each_g1 / _verify_batch_g1) and of the scalar
kernels in front of them (bpp_kernels.hip.h), in the manner of smc_model.py: every generator of the setup is a known multiple of one point, so every point of a
proof is a known multiple too and the verifier's ONE equation is decided in the exponent.  A "point" here is its discrete logarithm, an integer modulo r.

    prove            the reference's prover, line by line (bulletproofs_plus_plus/src/range_proof.rs:255-719) over wnla_prove
                     (weighted_norm_linear_argument.rs:26-188); challenges are drawn where the transcript would give them
    verify_literal   the reference's verifier as it stands: the vector pipeline of range_proof.rs:773-873 (q_pows, batch-inverted q_inv_pows, alpha_*, add_vecs
                     with padding) and get_bases_and_scalars_for_reduced_commitment (weighted_norm_linear_argument.rs:380-453: get_g_multiples, get_h_multiples),
                     collected per base
    verify_closed    the closed form include/dock_gpu_bpp.h states and the kernels compute

Nothing here shares code with the library."""
from bbs_model import R

N_H = 8
SHAPES = [(2, 8, 1), (2, 8, 2), (4, 8, 2), (16, 8, 1), (16, 32, 1), (4, 16, 4), (16, 64, 2), (2, 64, 2), (2, 4, 1), (2, 4, 2)]      # (base, num_bits, values)
CHAL = ["e", "x", "y", "r", "lambda", "delta", "t"]


def inv(v):
    assert v % R, "inverse of zero"
    return pow(v % R, R - 2, R)


# ---- the shape -----------------------------------------------------------------------------------------------------------------------------------
class Shape:
    def __init__(self, base, num_bits, m):
        self.base, self.num_bits, self.m = base, num_bits, m
        self.bb = base.bit_length() - 1                      # util::base_bits
        self.dp = num_bits // self.bb
        self.D = self.dp * m
        self.NG = max(self.dp, base) * m                     # setup.rs:114-116 get_no_of_G
        self.lg = self.NG.bit_length() - 1
        self.K = max(3, self.lg)
        self.own = m + 4 + 2 * self.K
        self.shared = 1 + N_H + self.NG


class Setup:
    """the logs of G, G_vec, H_vec"""

    def __init__(self, shape, rnd):
        self.g = rnd()
        self.G = [rnd() for _ in range(shape.NG)]
        self.H = [rnd() for _ in range(N_H)]

    def logs(self):
        """in the order of the resident handle: [G, H_0 .. H_7, G_0 ..]"""
        return [self.g] + self.H + self.G

    def commit(self, v, l, n):
        """compute_commitment: v g + <g_vec, n> + <h_vec, l> (msm_unchecked stops at the shorter side)"""
        return (v * self.g + sum(a * b for a, b in zip(self.G, n)) + sum(a * b for a, b in zip(self.H, l))) % R


# ---- utils/src/ff.rs -------------------------------------------------------------------------------------------------------------------------------
def inner_product(a, b):
    return sum(x * y for x, y in zip(a, b)) % R


def hadamard_product(a, b):
    return [x * y % R for x, y in zip(a, b)]


def add_vecs(a, b):
    n = max(len(a), len(b))
    return [((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % R for i in range(n)]


def powers(s, num):
    out = []
    for i in range(num):
        out.append(1 if i == 0 else out[-1] * s % R)
    return out


def powers_starting_from(start, exp, num):
    out = []
    for i in range(num):
        out.append(start % R if i == 0 else out[-1] * exp % R)
    return out


def weighted_inner_product(a, b, w):
    size = min(len(a), len(b))
    weights = powers(w, size + 1)[1:]
    return sum(a[i] * b[i] * weights[i] for i in range(size)) % R


def weighted_norm(n, w):
    return weighted_inner_product(n, n, w)


def scale(arr, f):
    return [v * f % R for v in arr]


def batch_inversion(v):
    return [inv(x) if x % R else 0 for x in v]


# ---- range_proof.rs: the helpers below line 889 -----------------------------------------------------------------------------------------------------
def alpha_d(base, dp, num_proofs, lam):
    return [lp * bp % R for lp in powers(lam, num_proofs) for bp in powers(base, dp)]


def alpha_m(e, x, n):
    return [x * inv(e + i) % R for i in range(n)]


def alpha_r(n, x, delta):
    return [(-x * delta) % R] * n


def alpha_r2(n, e):
    return [e % R] * n


def t_pow_in_c(i):
    return [1, 0, 2, 3, 4, 6, 7, 8, 9][i]


def c_poly(y):
    return [[1]] + [[y]] * 7 + [[0]]


def create_c_vec(y, t):
    ti = inv(t)
    return [y * ti % R] + [y * pow(t, k, R) % R for k in (1, 2, 3, 5, 6, 7)] + [0]


def t_power(t, i):
    """TPowers::nth_power"""
    return inv(t) if i == -1 else pow(t, i, R)


def poly_eval(coeffs, t):
    res = [0] * len(coeffs[0])
    for j, cs in enumerate(coeffs):
        for i, c in enumerate(cs):
            res[i] = (res[i] + t_power(t, j - 1) * c) % R
    return res


def w_q_norm(coeffs, q):
    res = [0] * (2 * len(coeffs) - 1)
    for i, a in enumerate(coeffs):
        for j, b in enumerate(coeffs):
            n = min(len(a), len(b))
            qp = powers_starting_from(q, q, n)
            res[i + j] = (res[i + j] + sum(a[k] * b[k] * qp[k] for k in range(n))) % R
    return res


def multiply_with_poly_of_constants(coeffs, c):
    res = [0] * (len(coeffs) + len(c) - 1)
    for l, lv in enumerate(coeffs):
        for i, v in enumerate(lv):
            tp = t_pow_in_c(i)
            if tp >= len(c):
                continue
            res[l + tp] = (res[l + tp] + v * c[i][0]) % R
    return res


# ---- the proof ---------------------------------------------------------------------------------------------------------------------------------------
class Proof:
    """points as logs: V (m), D, M, R, S, X (K), Rr (K); scalars l0, n0; chal: e, x, y, r, lambda, delta, t, gamma_0 .."""

    def __init__(self, V, D, M, Rp, S, X, Rr, l, n, chal):
        self.V, self.D, self.M, self.R, self.S, self.X, self.Rr, self.l, self.n, self.chal = list(V), D, M, Rp, S, list(X), list(Rr), list(l), list(n), list(chal)

    @property
    def l0(self):
        return self.l[0]

    @property
    def n0(self):
        return self.n[0]

    def own_points(self):
        """in the order of the calls' own scalars: V .., D, M, R, S, X .., R .."""
        return self.V + [self.D, self.M, self.R, self.S] + self.X + self.Rr

    def copy(self):
        return Proof(self.V, self.D, self.M, self.R, self.S, self.X, self.Rr, self.l, self.n, self.chal)


def split_vec(v):
    return list(v[0::2]), list(v[1::2])


def wnla_prove(l, n, c, rho, setup_g, g_vec, h_vec, challenge):
    """WeightedNormLinearArgument::new; challenge(): the next gamma"""
    l, n, c, g_vec, h_vec = list(l), list(n), list(c), list(g_vec), list(h_vec)
    assert len(l) == len(c) == len(h_vec) and len(n) == len(g_vec)
    mu = rho * rho % R
    X, Rs, gammas = [], [], []
    while len(l) > 1 or len(n) > 1:
        l_0, l_1 = split_vec(l)
        n_0, n_1 = split_vec(n)
        c_0, c_1 = split_vec(c)
        g_0, g_1 = split_vec(g_vec)
        h_0, h_1 = split_vec(h_vec)
        rho_inv = inv(rho)
        mu_sqr = mu * mu % R
        v_x = (2 * rho_inv * weighted_inner_product(n_0, n_1, mu_sqr) + inner_product(c_0, l_1) + inner_product(c_1, l_0)) % R
        v_r = (weighted_norm(n_1, mu_sqr) + inner_product(c_1, l_1)) % R
        scaled_n_0 = scale(n_0, rho_inv)
        scaled_n_1 = scale(n_1, rho)
        X_i = (setup_g * v_x + inner_product(h_0, l_1) + inner_product(h_1, l_0) + inner_product(g_0, scaled_n_1) + inner_product(g_1, scaled_n_0)) % R
        R_i = (setup_g * v_r + inner_product(h_1, l_1) + inner_product(g_1, n_1)) % R
        gamma = challenge()
        if len(l) > 1:
            l = [(a + gamma * b) % R for a, b in zip(l_0, l_1)]
            c = [(a + gamma * b) % R for a, b in zip(c_0, c_1)]
            h_vec = [(a + b * gamma) % R for a, b in zip(h_0, h_1)]
        if len(n) > 1:
            n = [(a * rho_inv + gamma * b) % R for a, b in zip(n_0, n_1)]
            g_vec = [(a * rho + b * gamma) % R for a, b in zip(g_0, g_1)]
        rho, mu = mu, mu_sqr
        X.append(X_i); Rs.append(R_i); gammas.append(gamma)
    return X, Rs, l, n, gammas


def prove(shape, setup, values, rnd):
    """Prover::prove.  rnd(): the next random scalar, the prover's and the transcript's alike.  The digits are the low dp digits of every value, whatever its size,
    as round_1 takes them"""
    base, dp, m = shape.base, shape.dp, shape.m
    assert len(values) == m
    gam = [rnd() for _ in values]
    V = [(v * setup.g + g * setup.H[0]) % R for v, g in zip(values, gam)]            # compute_pedersen_commitment
    # round 1
    d, mult, mask = [], [0] * base, (1 << shape.bb) - 1
    for v in values:
        v1 = v
        for _ in range(dp):
            dig = v1 & mask
            d.append(dig)
            mult[dig] += 1
            v1 >>= shape.bb
    r_m1 = [rnd() for _ in range(8)]
    r_d1 = [0] * 8
    r_m1[6] = 0; r_d1[5] = rnd()
    r_m1[3] = 0; r_d1[2] = rnd()
    r_d0, r_m0 = rnd(), rnd()
    Dp, Mp = setup.commit(r_d0, r_d1, d), setup.commit(r_m0, r_m1, mult)
    e = rnd()
    # round 2
    rv = batch_inversion([(e + x) % R for x in d])
    r_r1 = [0] * 8
    r_r1[4] = -r_d1[5] % R
    r_r1[1] = -r_d1[2] % R
    r_r0 = rnd()
    Rp = setup.commit(r_r0, r_r1, rv)
    x, y, r, lam, delta = rnd(), rnd(), rnd(), rnd(), rnd()
    q = r * r % R
    # round 3
    mvec = scale(mult, delta)
    q_inv = inv(q)
    q_inv_pows = powers_starting_from(q_inv, q_inv, len(setup.G))
    al_r = add_vecs(hadamard_product(alpha_r(shape.D, x, delta), q_inv_pows), alpha_r2(shape.D, e))
    al_d = hadamard_product(alpha_d(base, dp, m, lam), q_inv_pows)
    al_m = hadamard_product(alpha_m(e, x, base), q_inv_pows)
    t_2, t_3 = add_vecs(d, al_r), add_vecs(rv, al_d)
    s = [rnd() for _ in range(len(setup.G))]
    w_coeffs = [s, mvec, t_2, t_3, al_m]
    w_w_q = w_q_norm(w_coeffs, q)
    y_inv = inv(y)
    c = c_poly(y)
    gamma_v = inner_product(gam, powers_starting_from(2, lam, len(gam)))
    lm1, ld1, lr1 = [-r_m0 % R] + r_m1, [-r_d0 % R] + r_d1, [-r_r0 % R] + r_r1
    lm1 = scale(lm1, delta)
    l_coeffs = [[], lm1, ld1, lr1, [0, gamma_v], [], [], []]
    l_vec_w_q = multiply_with_poly_of_constants(l_coeffs, c)
    l_s = [(-a - b) % R for _, a, b in zip(range(len(setup.H) + 1), w_w_q, l_vec_w_q)]
    l_s.pop(5)
    b_s = l_s.pop(1)
    l_s.append(0)
    l_s = scale(l_s, y_inv)
    l_coeffs[0] = list(l_s)
    S = setup.commit(-b_s % R, l_s, s)
    for k in (1, 2, 3, 4):
        l_coeffs[k] = l_coeffs[k][1:]
    t = rnd()
    # round 4
    w_eval, l_eval = poly_eval(w_coeffs, t), poly_eval(l_coeffs, t)
    X, Rs, l, n, gammas = wnla_prove(l_eval, w_eval, create_c_vec(y, t), r, setup.g, setup.G, setup.H, rnd)
    return Proof(V, Dp, Mp, Rp, S, X, Rs, l, n, [e, x, y, r, lam, delta, t] + gammas)


# ---- the reference's verifier, literally ---------------------------------------------------------------------------------------------------------------
def get_h_multiples(n, gamma):
    mult = [1] * n
    for i in range(n.bit_length() - 1):
        ps = 1 << i
        for j in range(n // ps):
            if j % 2 == 1:
                for l in range(ps):
                    mult[j * ps + l] = mult[j * ps + l] * gamma[i] % R
    return mult


def get_g_multiples(n, rho, gamma):
    mult = [1] * n
    rho_i = rho
    for i in range(n.bit_length() - 1):
        ps = 1 << i
        for j in range(n // ps):
            f = rho_i if j % 2 == 0 else gamma[i]
            for l in range(ps):
                mult[j * ps + l] = mult[j * ps + l] * f % R
        rho_i = rho_i * rho_i % R
    return mult


def verify_literal(shape, n_g, proof):
    """Proof::verify up to the MSM: (shared, own) — the scalar of every base, the terms of one base added up: shared[0] G, shared[1 + k] H_k, shared[9 + k] G_k; own in
    the order of Proof.own_points.  n_g = |G_vec|.  Raises where the reference unwrap()s the inverse of zero"""
    base, dp, m, D = shape.base, shape.dp, shape.m, shape.D
    e, x, y, r, lam, delta, t = proof.chal[:7]
    gamma = proof.chal[7:]
    q = r * r % R
    c_vec = create_c_vec(y, t)
    t_inv, t_sqr, t_cube = t_power(t, -1), t_power(t, 2), t_power(t, 3)
    q_pows = powers_starting_from(q, q, n_g)
    assert all(v for v in q_pows), "inverse of zero"
    q_inv_pows = batch_inversion(q_pows)
    lambda_powers = powers(lam, m)
    al_d = [lp * bp % R for lp in lambda_powers for bp in powers(base, dp)]            # alpha_d_given_lambda_powers
    al_d_q = hadamard_product(al_d, q_inv_pows)
    al_r2 = alpha_r2(D, e)
    al_r = alpha_r(D, x, delta)
    al_r_q = add_vecs(hadamard_product(al_r, q_inv_pows), al_r2)
    # g_offset
    two_t_3 = 2 * t_cube % R
    v_hat_1 = inner_product([two_t_3] * D, q_pows)
    v_hat_2 = inner_product(al_d, al_r2) * two_t_3 % R
    v_hat_3 = inner_product(al_d_q, al_r) * two_t_3 % R
    g_offset = (v_hat_1 + v_hat_2 + v_hat_3) % R
    # g_vec_pub_offsets
    al_m = hadamard_product(alpha_m(e, x, base), q_inv_pows)
    pub = add_vecs(add_vecs(scale(al_d_q, t_sqr), scale(al_r_q, t)), scale(al_m, t_cube))
    # get_bases_and_scalars_for_reduced_commitment
    mu = r * r % R
    for _ in range(n_g.bit_length() - 1):
        mu = mu * mu % R
    g_mult = get_g_multiples(n_g, r, gamma)
    h_mult = get_h_multiples(N_H, gamma)
    v = (proof.l0 * inner_product(c_vec, h_mult) + weighted_norm(proof.n, mu)) % R
    shared = [0] * (1 + N_H + n_g)
    shared[0] = (v - g_offset) % R
    for k, hm in enumerate(h_mult):
        shared[1 + k] = hm * proof.l0 % R
    for k, gm in enumerate(g_mult):
        shared[1 + N_H + k] = gm * proof.n0 % R
    for k, p in enumerate(pub):
        shared[1 + N_H + k] = (shared[1 + N_H + k] - p) % R
    own = [-(lp * two_t_3) % R for lp in lambda_powers] + [-t % R, -delta % R, -t_sqr % R, -t_inv % R] + [-g % R for g in gamma] + [-(g * g - 1) % R for g in gamma]
    return shared, own


# ---- the closed form ------------------------------------------------------------------------------------------------------------------------------------
def status2(shape, chal):
    e, r, t = chal[0], chal[3], chal[6]
    return t % R == 0 or r % R == 0 or any((e + k) % R == 0 for k in range(shape.base))


def verify_closed(shape, proof):
    """(shared, own) by the formulas of include/dock_gpu_bpp.h, or None for status 2"""
    base, dp, m, D, NG, lg, K = shape.base, shape.dp, shape.m, shape.D, shape.NG, shape.lg, shape.K
    if status2(shape, proof.chal):
        return None
    e, x, y, r, lam, delta, t = [v % R for v in proof.chal[:7]]
    gamma = [v % R for v in proof.chal[7:7 + K]]
    l0, n0 = proof.l0 % R, proof.n0 % R
    q = r * r % R
    qi, ti = inv(q), inv(t)
    hm = [1] * 8
    for k in range(8):
        for j in range(3):
            if k >> j & 1:
                hm[k] = hm[k] * gamma[j] % R
    gm = [1] * NG
    for k in range(NG):
        for j in range(lg):
            gm[k] = gm[k] * (gamma[j] if k >> j & 1 else pow(r, 1 << j, R)) % R
    c = [y * v % R for v in (ti, t, pow(t, 2, R), pow(t, 3, R), pow(t, 5, R), pow(t, 6, R), pow(t, 7, R), 0)]
    mu = pow(r, 2 * NG, R)
    v = (l0 * sum(a * b for a, b in zip(c, hm)) + n0 * n0 * mu) % R
    ad = [pow(lam, k // dp, R) * pow(base, k % dp, R) % R for k in range(D)]
    qik = [pow(qi, k + 1, R) for k in range(NG)]
    t2, t3 = t * t % R, pow(t, 3, R)
    pub = [0] * NG
    for k in range(NG):
        if k < D:
            pub[k] += t2 * ad[k] * qik[k] + t * (e - x * delta * qik[k])
        if k < base:
            pub[k] += t3 * x * qik[k] * inv(e + k)
        pub[k] %= R
    g_off = 2 * t3 * (sum(pow(q, k + 1, R) for k in range(D)) + e * sum(ad) - x * delta * sum(ad[k] * qik[k] for k in range(D))) % R
    shared = [(v - g_off) % R] + [l0 * h % R for h in hm] + [(n0 * gm[k] - pub[k]) % R for k in range(NG)]
    own = [-2 * t3 * pow(lam, k, R) % R for k in range(m)] + [-t % R, -delta % R, -t2 % R, -ti % R] + [-g % R for g in gamma] + [(1 - g * g) % R for g in gamma]
    return shared, own


def equation(setup, proof, shared, own):
    """the verifier's sum, in the exponent"""
    return (sum(a * b for a, b in zip(shared, setup.logs())) + sum(a * b for a, b in zip(own, proof.own_points()))) % R


def status(shape, setup, proof):
    """what dgpu_bpp_range_proofs_verify_each_g1 answers"""
    sc = verify_closed(shape, proof)
    if sc is None:
        return 2
    return 0 if equation(setup, proof, *sc) == 0 else 1


def batch_ok(shape, setup, proofs, rho):
    """what dgpu_bpp_range_proofs_verify_batch_g1 answers: no status 2 and sum_i rho^i (equation i) = 0"""
    total = 0
    for i, p in enumerate(proofs):
        sc = verify_closed(shape, p)
        if sc is None:
            return False
        total += pow(rho, i, R) * equation(setup, p, *sc)
    return total % R == 0


def batch_columns(shape, proofs, rho, i0=0):
    """(the coefficients of the shared points, the weights over the own points proof by proof) of the proofs i0 .. of a batch"""
    coeff, wts = [0] * shape.shared, []
    for i, p in enumerate(proofs):
        shared, own = verify_closed(shape, p)
        w = pow(rho, i0 + i, R)
        coeff = [(c + w * s) % R for c, s in zip(coeff, shared)]
        wts.append([w * o % R for o in own])
    return coeff, wts


# ---- tampers ----------------------------------------------------------------------------------------------------------------------------------------------
def own_slots(shape):
    return ["V%d" % k for k in range(shape.m)] + ["D", "M", "R", "S"] + ["X%d" % j for j in range(shape.K)] + ["R%d" % j for j in range(shape.K)]


def tamper(proof, what, delta=1):
    """a copy with one thing moved: an own point by its slot name (own_slots), "l0", "n0", or a challenge by its name (CHAL, "gamma<j>")"""
    p = proof.copy()
    if what == "l0":
        p.l[0] = (p.l[0] + delta) % R
    elif what == "n0":
        p.n[0] = (p.n[0] + delta) % R
    elif what in CHAL:
        p.chal[CHAL.index(what)] = (p.chal[CHAL.index(what)] + delta) % R
    elif what.startswith("gamma"):
        p.chal[7 + int(what[5:])] = (p.chal[7 + int(what[5:])] + delta) % R
    elif what in ("D", "M", "R", "S"):
        setattr(p, what, (getattr(p, what) + delta) % R)
    elif what[0] == "V":
        p.V[int(what[1:])] = (p.V[int(what[1:])] + delta) % R
    elif what[0] == "X":
        p.X[int(what[1:])] = (p.X[int(what[1:])] + delta) % R
    elif what[0] == "R":
        p.Rr[int(what[1:])] = (p.Rr[int(what[1:])] + delta) % R
    else:
        raise ValueError(what)
    return p


def tamper_kinds(shape):
    return own_slots(shape) + ["l0", "n0"] + CHAL + ["gamma%d" % j for j in range(shape.K)]


def make_rnd(seed):
    import random
    g = random.Random(seed)
    return lambda: g.randrange(1, R)
