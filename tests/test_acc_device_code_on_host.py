"""CPU: the per-lane routines of the accumulator witness update (crypto_amd/csrc/acc_kernels.hip.h: add_step, rem_step, eval_chunk, combine_step,
finish_share) compiled for the host with the FP29_CHECK operand asserts (tests/native/acc_dev_host_shim.cpp) and driven as the kernels drive them,
against the Python big-integer transcription of the reference's memoized formulas (tests/acc_model.py); and the host's tables that depend on the
secret key (crypto_amd/csrc/acc_host_tables.hpp) against the same model.  A green run shows the values are right and
that no product leaves fr_mul's operand contract: list lengths around the minimum chunk length, one to many chunks, elements that are 0, 1, r - 1,
an addition (f = 0, g still right) or a removal (f = g = 0), operands pushed to the top of their bounds, and shares of the batch inversion with a
zero at every position."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import acc_model as AM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "acc_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libacc_dev_host_shim.so")
R = AM.R
CH = 32            # acck::ACC_MIN_CHUNK
SHAPES = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (5, 3), (0, 6), (CH - 1, CH + 1), (3 * CH + 1, 2 * CH)]
p_ = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "acc_kernels.hip.h", "acc_host_tables.hpp", "host_field.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-mbmi2", "-madx", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.shim_acc_update.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    L.shim_acc_update.restype = None
    L.shim_acc_host_tables.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
    L.shim_acc_host_tables.restype = C.c_int
    return L


def words(vals):
    return np.array([(v >> (32 * k)) & 0xFFFFFFFF for v in vals for k in range(8)], dtype=np.uint32)


def ints(w):
    return [sum(int(x) << (32 * k) for k, x in enumerate(row)) for row in w.reshape(-1, 8)]


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def run(shim, adds, rems, alpha, ys, K, G, stress):
    m = len(ys)
    f, g = np.zeros(8 * m, np.uint32), np.zeros(8 * m, np.uint32)
    shim.shim_acc_update(len(adds), len(rems), p_(words(AM.host_tables(adds, rems, alpha))), m, p_(words(ys)), K, G, p_(f), p_(g), stress)
    return ints(f), ints(g)


def test_the_minimum_chunk_length_is_the_launchers():
    hdr = open(os.path.join(CSRC, "acc_launch.hip.h")).read()
    assert re.search(r"ACC_MIN_CHUNK = (\d+)", hdr).group(1) == str(CH)


@pytest.mark.parametrize("stress", [0, 1])
@pytest.mark.parametrize("na,nr", SHAPES)
def test_factors_match_the_reference_formulas(shim, na, nr, stress):
    rng = np.random.default_rng(1000 * na + nr)
    alpha = rand(rng, 1)[0]
    adds, rems = rand(rng, na), rand(rng, nr)
    if na > 2:
        adds[1] = R - 1                                       # extreme entries in the lists too
    if nr > 2:
        rems[2] = 0
    ys = [0, 1, R - 1] + rand(rng, 3)
    ys += [adds[0], adds[-1]] if na else []                   # just added: d_A = 0, so f = 0 and g = v_AD / d_D
    ys += [rems[0], rems[-1], rems[nr // 2]] if nr else []    # removed: d_D = 0, so f = g = 0
    want = AM.update_factors(adds, rems, alpha, ys)
    if na:
        assert want[0][6] == 0 and want[0][7] == 0
    if nr:
        assert want[0][-1] == 0 and want[1][-1] == 0
    m = len(ys)
    for K in sorted({1, 2, 3, max(na, nr, 1)}):               # one chunk, two, three, one chunk per entry
        for G in (1, 3, m):                                   # one lane takes every element; strided shares; one element per lane
            assert run(shim, adds, rems, alpha, ys, K, G, stress) == want, (K, G)


@pytest.mark.parametrize("stress", [0, 1])
def test_maximal_values_everywhere(shim, stress):
    """every list entry, alpha and element the largest residue or next to it"""
    adds, rems, alpha = [R - 1, R - 2, R - 1, R - 3] * 9, [R - 2, R - 4, R - 5] * 11, R - 6
    ys = [R - 1, R - 7, R - 2, 0]
    want = AM.update_factors(adds, rems, alpha, ys)
    for K in (1, 2, 36):
        assert run(shim, adds, rems, alpha, ys, K, 2, stress) == want, K


@pytest.mark.parametrize("n", [1, 2, 31])
def test_batch_inversion_share_with_a_zero_at_any_position(shim, n):
    """one lane's share of n elements (one fr_inv): an element among the removals has d_D = 0; one takes its place in Montgomery's trick and the
    others' inverses stay right"""
    rng = np.random.default_rng(n)
    alpha = rand(rng, 1)[0]
    adds, rems = rand(rng, 3), rand(rng, 4)
    base = rand(rng, n)
    patterns = [[0], [n - 1], list(range(n))] + [[k] for k in range(1, n - 1)]
    for zeros in patterns:
        ys = list(base)
        for k in zeros:
            ys[k] = rems[k % 4]
        want = AM.update_factors(adds, rems, alpha, ys)
        assert all(want[0][k] == 0 and want[1][k] == 0 for k in zeros)
        for K in (1, 2):
            assert run(shim, adds, rems, alpha, ys, K, 1, n & 1) == want, (zeros, K)


def limbs64(vals):
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in vals for k in range(4)], dtype=np.uint64)


@pytest.mark.parametrize("na,nr", [(0, 0), (1, 0), (0, 1), (5, 3), (CH + 1, 2 * CH)])
def test_host_tables_from_the_secret_key(shim, na, nr):
    """F_s, G_s, Phi as the driver builds them (prefix products, one inversion, back down) are the model's, for canonical words, canonical words that
    are not reduced, and Montgomery words; an entry equal to -alpha is refused"""
    rng = np.random.default_rng(77 + 100 * na + nr)
    alpha = rand(rng, 1)[0]
    adds, rems = rand(rng, na), rand(rng, nr)
    R2 = pow(2, 256, R)
    want = [v * R2 % R for v in AM.host_tables(adds, rems, alpha)]          # ark-ff Montgomery words
    ne = 2 * na + 2 * nr + 1
    forms = [(adds, rems, alpha, 0), ([a + R for a in adds], [r + R for r in rems], alpha + R, 0), ([a * R2 % R for a in adds], [r * R2 % R for r in rems], alpha * R2 % R, 1)]
    for a, r, al, mont in forms:
        out = np.zeros(4 * ne, np.uint64)
        assert shim.shim_acc_host_tables(p_(limbs64(a)), na, p_(limbs64(r)), nr, p_(limbs64([al])), mont, p_(out)) == 0
        got = [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in out.reshape(-1, 4)]
        assert got == want, mont
    out = np.zeros(4 * (ne + 2), np.uint64)
    assert shim.shim_acc_host_tables(p_(limbs64(adds + [R - alpha])), na + 1, p_(limbs64(rems)), nr, p_(limbs64([alpha])), 0, p_(out)) == -3
    assert shim.shim_acc_host_tables(p_(limbs64(adds)), na, p_(limbs64([R - alpha] + rems)), nr + 1, p_(limbs64([alpha])), 0, p_(out)) == -3
