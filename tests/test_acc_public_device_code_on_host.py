"""CPU: the per-lane routines of the accumulator's update from public information (crypto_amd/csrc/acc_kernels.hip.h: omega_value, omega_pair, pub_chunk,
pub_finish_share, pub_row_run) compiled for the host with the FP29_CHECK operand asserts (tests/native/acc_public_dev_host_shim.cpp) and driven as the
kernels drive them.  The raw finishing mode (v_AD at the roots of unity, one to many chunks) against tests/acc_model.py's evaluation formulas, and
its inverse transform — done here with big integers — against the coefficient model of tests/acc_public_model.py: that is the statement the device
pipeline rests on (the interpolated coefficients are the direct ones, and there are max(n_add, n_rem) of them).  The factor routine against the
model with a removed holder at every position of a share; the power rows for y = 0, 1, r - 1, run lengths around the row length, and operands
pushed to the top of their bounds.  A green run shows the values are right and that no product leaves fr_mul's operand contract."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import acc_model as AM
import acc_public_model as PM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "acc_public_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libacc_public_dev_host_shim.so")
R = AM.R
SHAPES = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (5, 3), (0, 6), (4, 4), (33, 31), (64, 65)]
p_ = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "acc_kernels.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz = C.c_void_p, C.c_size_t
    L.shim_omega_values.argtypes = [sz, sz, vp, sz, vp, sz, vp, C.c_int]
    L.shim_omega_pair.argtypes = [vp, vp, vp, vp, vp, C.c_int]
    L.shim_pub_factors.argtypes = [sz, sz, vp, sz, vp, sz, sz, vp, vp, vp, C.c_int]
    L.shim_pub_rows.argtypes = [sz, vp, vp, sz, sz, vp, C.c_int]
    for f in (L.shim_omega_values, L.shim_omega_pair, L.shim_pub_factors, L.shim_pub_rows):
        f.restype = None
    return L


def words(vals):
    return np.array([(v >> (32 * k)) & 0xFFFFFFFF for v in vals for k in range(8)], dtype=np.uint32)


def ints(w):
    return [sum(int(x) << (32 * k) for k, x in enumerate(row)) for row in w.reshape(-1, 8)]


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def test_the_run_length_is_the_launchers():
    hdr = open(os.path.join(CSRC, "acc_launch.hip.h")).read()
    assert re.search(r"ACC_ROW_RUN = (\d+)", hdr).group(1) == "32"


def inverse_dft(values, logn):
    n = 1 << logn
    w_inv = pow(pow(7, (R - 1) >> logn, R), R - 2, R)
    n_inv = pow(n, R - 2, R)
    return [sum(v * pow(w_inv, i * j, R) for i, v in enumerate(values)) * n_inv % R for j in range(n)]


@pytest.mark.parametrize("stress", [0, 1])
@pytest.mark.parametrize("na,nr", SHAPES)
def test_values_at_the_roots_of_unity_interpolate_to_the_coefficients(shim, na, nr, stress):
    rng = np.random.default_rng(2000 * na + nr)
    alpha = rand(rng, 1)[0]
    adds, rems = rand(rng, na), rand(rng, nr)
    if na > 2:
        adds[1] = R - 1
    if nr > 2:
        rems[2] = 0
    coeffs = PM.v_ad_coefficients(adds, rems, alpha)
    assert len(coeffs) == max(na, nr)                              # a random batch: the leading coefficient does not vanish
    logn = max(na, nr, 1).bit_length() - (1 if max(na, nr, 1) & (max(na, nr, 1) - 1) == 0 else 0)
    pts = PM.roots_of_unity(logn)
    N = len(pts)
    assert N >= max(na, nr) and (N == 1 or N // 2 < max(na, nr))
    want = [AM.poly_v_ad_eval_direct(adds, rems, alpha, x) for x in pts]
    assert want == [PM.poly_eval(coeffs, x) for x in pts]
    tables = words(AM.host_tables(adds, rems, alpha))
    for K in sorted({1, 2, 5, max(na, nr, 1)}):
        out = np.zeros(8 * N, np.uint32)
        shim.shim_omega_values(na, nr, p_(tables), N, p_(words(pts)), K, p_(out), stress)
        assert ints(out) == want, K
    assert inverse_dft(want, logn) == coeffs + [0] * (N - len(coeffs))
    if N == 2:                                                     # the size the finishing kernel transforms itself
        c0, c1 = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
        shim.shim_omega_pair(p_(words(want[:1])), p_(words(want[1:])), p_(words([pow(2, R - 2, R)])), p_(c0), p_(c1), stress)
        assert ints(c0) + ints(c1) == coeffs + [0] * (2 - len(coeffs))


def test_a_vanishing_polynomial_and_extreme_pairs(shim):
    alpha, a = 5, 11
    assert PM.v_ad_coefficients([a], [a], alpha) == []             # 1 - (a + alpha) / (a + alpha)
    out = np.ones(8, np.uint32)
    shim.shim_omega_values(1, 1, p_(words(AM.host_tables([a], [a], alpha))), 1, p_(words([1])), 1, p_(out), 0)
    assert ints(out) == [0]
    half = pow(2, R - 2, R)
    for e0, e1 in [(0, 0), (R - 1, R - 1), (0, R - 1), (R - 1, 0), (1, R - 2)]:
        for stress in (0, 1):
            c0, c1 = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
            shim.shim_omega_pair(p_(words([e0])), p_(words([e1])), p_(words([half])), p_(c0), p_(c1), stress)
            assert ints(c0) == [(e0 + e1) * half % R] and ints(c1) == [(e0 - e1) * half % R]


def run_factors(shim, adds, rems, ys, K, G, stress):
    m = len(ys)
    f, s, ok = np.zeros(8 * m, np.uint32), np.zeros(8 * m, np.uint32), np.full(m, 7, np.uint8)
    shim.shim_pub_factors(len(adds), len(rems), p_(words(adds + rems)), m, p_(words(ys)), K, G, p_(f), p_(s), p_(ok), stress)
    return list(zip(ints(f), ints(s), [bool(x) for x in ok]))


@pytest.mark.parametrize("stress", [0, 1])
@pytest.mark.parametrize("na,nr", SHAPES + [(31, 33), (97, 64)])
def test_public_factors_match_the_reference_formulas(shim, na, nr, stress):
    rng = np.random.default_rng(3000 * na + nr)
    adds, rems = rand(rng, na), rand(rng, nr)
    if na > 2:
        adds[1] = R - 1
    if nr > 2:
        rems[2] = 0
    ys = [0, 1, R - 1] + rand(rng, 3)
    ys += [adds[0], adds[-1]] if na else []                        # just added: f = 0, s = 1 / d_D
    ys += [rems[0], rems[-1], rems[nr // 2]] if nr else []         # removed: CannotBeZero
    want = [PM.public_factors(adds, rems, y) for y in ys]
    if nr:
        assert want[-1] == (0, 0, False)
    m = len(ys)
    for K in sorted({1, 2, 3, max(na, nr, 1)}):
        for G in (1, 3, m):
            assert run_factors(shim, adds, rems, ys, K, G, stress) == want, (K, G)


@pytest.mark.parametrize("n", [1, 2, 31])
def test_a_share_with_a_removed_holder_at_any_position(shim, n):
    rng = np.random.default_rng(n)
    adds, rems = rand(rng, 3), rand(rng, 4)
    base = rand(rng, n)
    for zeros in [[0], [n - 1], list(range(n))] + [[k] for k in range(1, n - 1)]:
        ys = list(base)
        for k in zeros:
            ys[k] = rems[k % 4]
        want = [PM.public_factors(adds, rems, y) for y in ys]
        assert all(want[k] == (0, 0, False) for k in zeros)
        for K in (1, 2):
            assert run_factors(shim, adds, rems, ys, K, 1, n & 1) == want, (zeros, K)


@pytest.mark.parametrize("stress", [0, 1])
@pytest.mark.parametrize("n,run", [(1, 32), (31, 32), (32, 32), (33, 32), (129, 32), (300, 32), (70, 1), (70, 7), (1000, 64)])
def test_power_rows(shim, n, run, stress):
    rng = np.random.default_rng(n * 100 + run)
    ys = [0, 1, R - 1, 2] + rand(rng, 2)
    ss = rand(rng, 3) + [0, R - 1, 1]                              # a removed holder's s is 0: a row of zeros
    rows = np.zeros(8 * len(ys) * n, np.uint32)
    shim.shim_pub_rows(len(ys), p_(words(ys)), p_(words(ss)), n, run, p_(rows), stress)
    want = [v for y, s in zip(ys, ss) for v in PM.scaled_powers(y, s, n)]
    assert ints(rows) == want
