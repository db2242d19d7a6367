"""Python big-integer transcription of the reference's accumulator witness update with the secret key: Poly_d::eval_direct, Poly_v_A::eval_direct,
Poly_v_D::eval_direct, Poly_v_AD::eval_direct (vb_accumulator/src/batch_utils.rs:102-106,171-199,328-359,448-454, the memoized forms, line by line)
and the factors of Witness::compute_update_using_secret_key_after_batch_updates (vb_accumulator/src/witness.rs:252-283).  Shared by
tests/test_acc_device_code_on_host.py and tests/test_gpu_accumulator.py; also the host tables the device routines are fed with."""
import functools

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


@functools.lru_cache(maxsize=4096)
def inv_or_zero(x):
    """ark-ff's batch_inversion leaves a zero entry as it is (cached: eval_direct inverts the same removals + alpha for every element)"""
    return pow(x, R - 2, R)


def poly_d_eval_direct(updates, x):
    a = 1
    for y in updates:
        a = (y - x) * a % R
    return a


def poly_v_a_eval_direct(additions, alpha, x):
    n = len(additions)
    if n == 0:
        return 0
    if n == 1:
        return 1
    factors = [1] * n
    polys = [1] * n
    for s in range(1, n):
        factors[s] = factors[s - 1] * (additions[s - 1] + alpha) % R
        polys[n - 1 - s] = polys[n - s] * (additions[n - s] - x) % R
    return sum(p * f for f, p in zip(factors, polys)) % R


def poly_v_d_eval_direct(removals, alpha, x):
    n = len(removals)
    if n == 0:
        return 0
    y_plus_alpha_inv = [inv_or_zero((y + alpha) % R) for y in removals]
    factors = [1] * n
    polys = [1] * n
    factors[0] = y_plus_alpha_inv[0]
    for s in range(1, n):
        factors[s] = factors[s - 1] * y_plus_alpha_inv[s] % R
        polys[s] = polys[s - 1] * (removals[s - 1] - x) % R
    return sum(p * f for f, p in zip(factors, polys)) % R


def poly_v_ad_eval_direct(additions, removals, alpha, x):
    e = poly_v_a_eval_direct(additions, alpha, x)
    if removals:
        f = 1
        for a in additions:
            f = f * (a + alpha) % R
        e = (e - poly_v_d_eval_direct(removals, alpha, x) * f) % R
    return e


def update_factors(additions, removals, alpha, elements):
    """(d_A / d_D, v_AD / d_D) per element, a zero d_D giving (0, 0)"""
    additions = [a % R for a in additions]; removals = [r % R for r in removals]; alpha %= R
    fs, gs = [], []
    for y in elements:
        y %= R
        d_a, d_d_inv = poly_d_eval_direct(additions, y), inv_or_zero(poly_d_eval_direct(removals, y))
        fs.append(d_a * d_d_inv % R)
        gs.append(poly_v_ad_eval_direct(additions, removals, alpha, y) * d_d_inv % R)
    return fs, gs


def host_tables(additions, removals, alpha):
    """[a_s | F_s | r_s | G_s | Phi]: F_s = prod_{i<s} (a_i + alpha), G_s = prod_{i<=s} (r_i + alpha)^-1, Phi = prod_i (a_i + alpha)"""
    F, acc = [], 1
    for a in additions:
        F.append(acc); acc = acc * (a + alpha) % R
    phi = acc
    G, acc = [], 1
    for r in removals:
        acc = acc * (r + alpha) % R; G.append(pow(acc, R - 2, R))
    return [a % R for a in additions] + F + [r % R for r in removals] + G + [phi]
