"""Python big-integer model of the accumulator's update from public information: the coefficients of Poly_v_AD::generate (vb_accumulator/src/batch_utils.rs:
115-140,271-300,433-440) by the recurrences on coefficient lists
    additions   S <- S (a_s - x) + F_s,              F_s = prod_{i<s} (a_i + alpha)              from S = 0 to v_A
    removals    D <- D + G_s P,  P <- P (r_s - x),   G_s = prod_{i<=s} (r_i + alpha)^-1          from D = 0, P = 1 to v_D
    v_AD = v_A - Phi v_D, trimmed like ark-poly trims a DensePolynomial (trailing zero coefficients dropped)
and the holder's factors and scaled powers of Witness::compute_update_using_public_info_after_batch_updates (witness.rs:292-314, batch_utils.rs:664-691).
Shared by tests/test_acc_public_device_code_on_host.py and tests/test_gpu_accumulator_public.py."""
from acc_model import R


def mul_linear(p, u):
    """p(x) (u - x), lowest degree first"""
    q = [0] * (len(p) + 1)
    for k, c in enumerate(p):
        q[k] = (q[k] + c * u) % R
        q[k + 1] = (q[k + 1] - c) % R
    return q


def v_ad_coefficients(additions, removals, alpha, trim=True):
    additions = [a % R for a in additions]; removals = [r % R for r in removals]; alpha %= R
    S, F = [], 1
    for a in additions:
        S = mul_linear(S, a) if S else [0]
        S[0] = (S[0] + F) % R
        F = F * (a + alpha) % R
    D, P, G = [0] * len(removals), [1], 1
    for r in removals:
        G = G * pow(r + alpha, R - 2, R) % R
        for k, c in enumerate(P):
            D[k] = (D[k] + c * G) % R
        P = mul_linear(P, r)
    n = max(len(additions), len(removals))
    c = [((S[k] if k < len(S) else 0) - F * (D[k] if k < len(D) else 0)) % R for k in range(n)]
    if trim:
        while c and c[-1] == 0:
            c.pop()
    return c


def poly_eval(c, x):
    acc = 0
    for k in reversed(c):
        acc = (acc * x + k) % R
    return acc


def roots_of_unity(logn):
    w = pow(7, (R - 1) >> logn, R)                   # 7 = Fr::GENERATOR: the radix-2 domain generator ark-poly uses
    return [pow(w, i, R) for i in range(1 << logn)]


def public_factors(additions, removals, y):
    """(d_A / d_D, 1 / d_D, ok); a zero d_D (the reference's CannotBeZero) gives (0, 0, False)"""
    y %= R
    d_a = d_d = 1
    for a in additions:
        d_a = (a - y) * d_a % R
    for r in removals:
        d_d = (r - y) * d_d % R
    if d_d == 0:
        return 0, 0, False
    inv = pow(d_d, R - 2, R)
    return d_a * inv % R, inv, True


def scaled_powers(y, s, n):
    """Omega::scaled_powers_of_y"""
    out, cur = [], s % R
    for _ in range(n):
        out.append(cur)
        cur = cur * y % R
    return out
