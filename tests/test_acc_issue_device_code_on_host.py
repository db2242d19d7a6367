"""CPU: the per-lane routines that issue accumulator witnesses (crypto_amd/csrc/acc_kernels.hip.h: d_chunk<1>, d_chunk<4>, d_times, issue_scalar) compiled
for the host with the FP29_CHECK operand asserts (tests/native/acc_issue_dev_host_shim.cpp) and driven as k_acc_d, k_acc_d_combine, k_acc_issue_scalars and the
passes of dock_accumulator.hip drive them, against the big-integer model of tests/acc_issue_model.py: tail lanes (m no multiple of four), chunks of zero
length (K > n), passes with a short last one, a non-member equal to the first and to the last member of a chunk, y = 0 and y = r - 1, and every operand pushed
to the top of its bound.  The host's batch inversion of y + alpha (acc_host_tables.hpp issue_inverses) against the same model, share by share.  A green run
shows the values are right and that no product leaves fr_mul's operand contract."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import acc_issue_model as IM
from acc_model import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "acc_issue_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libacc_issue_dev_host_shim.so")
R2 = pow(2, 256, R)
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "acc_kernels.hip.h", "acc_host_tables.hpp", "host_field.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-mbmi2", "-madx", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz = C.c_void_p, C.c_size_t
    L.shim_d_for_batch.argtypes = [C.c_int, sz, vp, sz, vp, sz, sz, vp, vp, vp, C.c_int]
    L.shim_issue_scalars.argtypes = [sz, vp, vp, vp, C.c_int, vp, vp, C.c_int]
    L.shim_issue_inverses.argtypes = [vp, sz, vp, C.c_int, sz, vp]
    L.shim_d_for_batch.restype = L.shim_issue_scalars.restype = None
    L.shim_issue_inverses.restype = C.c_int
    return L


def words(vals):
    return np.array([(v >> (32 * k)) & 0xFFFFFFFF for v in vals for k in range(8)], dtype=np.uint32)


def ints(w):
    return [sum(int(x) << (32 * k) for k, x in enumerate(row)) for row in w.reshape(-1, 8)]


def limbs64(vals):
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in vals for k in range(4)], dtype=np.uint64)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def test_the_constants_are_the_launchers():
    hdr = open(os.path.join(CSRC, "acc_launch.hip.h")).read()
    assert re.search(r"ACC_D_PASS = \(size_t\)1 << (\d+)", hdr).group(1) == "20"
    assert re.search(r"ACC_D_UNROLL_MIN = 4 \* 64\b", hdr) and re.search(r"ACC_D_UNROLL_MIN_CHUNK = 512\b", hdr)


def run_d(shim, U, members, ys, K, npass, d_in, stress):
    m = len(ys)
    d, nz = np.zeros(8 * m, np.uint32), np.full(m, 7, np.uint8)
    shim.shim_d_for_batch(U, len(members), p_(words(members)), m, p_(words(ys)), K, npass, None if d_in is None else p_(words(d_in)), p_(d), p_(nz), stress)
    return ints(d), [int(x) for x in nz]


def case(m, n, K):
    """members and non-members with the edges the kernels can trip over: y = 0, y = r - 1, a non-member that is the first member of a chunk, one that is the
    last member of a chunk (for K <= n), a member equal to 0 and one equal to r - 1"""
    rng = np.random.default_rng(1000 * m + 10 * n + K)
    members, ys = rand(rng, n), rand(rng, m)
    if n > 2:
        members[1], members[2] = R - 1, 0
    edges = [0, R - 1]
    if n:
        edges = [members[n * (K - 1) // K], members[n - 1]] + edges      # the last chunk [n (K - 1) / K, n) is never empty: its first and its last member
    for k, e in enumerate(edges[:m]):                              # from the last non-member down: the tail lane first
        ys[m - 1 - k] = e
    return members, ys


@pytest.mark.parametrize("stress", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("n", [0, 1, 2, 33])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 9])
def test_d_against_the_model(shim, m, n, K, stress):
    members, ys = case(m, n, K)
    rng = np.random.default_rng(m + n + K)
    want = IM.d_for_batch(members, ys)
    if n:
        assert 0 in want                                           # a non-member that is a member
    d_in = rand(rng, m)
    d_in[0] = R - 1
    want_in = IM.d_for_batch(members, ys, d_in)
    for U in (1, 4):
        assert run_d(shim, U, members, ys, K, 1 << 20, None, stress) == (want, [int(d != 0) for d in want]), U
        assert run_d(shim, U, members, ys, K, 1 << 20, d_in, stress) == (want_in, [int(d != 0) for d in want_in]), U
        for npass in (7, 1):                                       # n = 33: five passes, the last one short; a member per pass
            assert run_d(shim, U, members, ys, K, npass, d_in, stress) == (want_in, [int(d != 0) for d in want_in]), (U, npass)


def test_the_partition_identity_of_the_model():
    rng = np.random.default_rng(7)
    members, ys = rand(rng, 12), rand(rng, 3)
    whole = IM.d_for_batch(members, ys)
    for cuts in ([], [0], [1], [6], [11], [12], [3, 3, 9]):
        assert IM.d_partitioned(members, ys, cuts) == whole


@pytest.mark.parametrize("stress", [0, 1])
def test_issue_scalars(shim, stress):
    rng = np.random.default_rng(99)
    alpha, f_v = rand(rng, 2)
    ys = [0, R - 1] + rand(rng, 7)
    d = rand(rng, 9)
    d[0], d[4], d[8] = 0, 0, f_v                                   # CannotBeZero at the edges of the batch; f_V - d = 0 is a zero scalar with ok = 1
    d[1], d[2] = R - 1, 1
    t = IM.membership_scalars(ys, alpha)
    want = IM.non_membership_scalars(d, ys, f_v, alpha)
    assert want[8] == (0, True)
    sc, zero = np.zeros(8 * 9, np.uint32), np.full(9, 7, np.uint8)
    shim.shim_issue_scalars(9, p_(words(d)), p_(words(t)), p_(words([f_v])), 1, p_(sc), p_(zero), stress)
    assert list(zip(ints(sc), [not z for z in zero])) == want
    for fv in (0, R - 1):                                          # f_V at the ends of the field
        shim.shim_issue_scalars(9, p_(words(d)), p_(words(t)), p_(words([fv])), 1, p_(sc), p_(zero), stress)
        assert list(zip(ints(sc), [not z for z in zero])) == IM.non_membership_scalars(d, ys, fv, alpha)
    shim.shim_issue_scalars(9, None, p_(words(t)), None, 0, p_(sc), p_(zero), stress)      # membership: t itself
    assert ints(sc) == t and not zero.any()


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("m,shares", [(1, 1), (2, 1), (9, 1), (9, 2), (9, 9), (33, 16)])
def test_host_inverses(shim, m, shares, mont):
    rng = np.random.default_rng(m * 20 + shares)
    alpha = rand(rng, 1)[0]
    ys = rand(rng, m)
    ys[0], ys[-1] = (R - alpha + 1) % R, (R - alpha - 1) % R      # next to -alpha
    form = (lambda vals: [v * R2 % R for v in vals]) if mont else (lambda vals: [v + R if k & 1 else v for k, v in enumerate(vals)])      # canonical words need not be reduced
    t = np.zeros(4 * m, np.uint64)
    assert shim.shim_issue_inverses(p_(limbs64(form(ys))), m, p_(limbs64(form([alpha]))), mont, shares, p_(t)) == 0
    got = [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in t.reshape(-1, 4)]
    assert got == [v * R2 % R for v in IM.membership_scalars(ys, alpha)]      # ark-ff Montgomery words
    for pos in (0, m - 1):                                                   # y = -alpha in the first and in the last position
        bad = list(ys)
        bad[pos] = R - alpha
        assert shim.shim_issue_inverses(p_(limbs64(form(bad))), m, p_(limbs64(form([alpha]))), mont, shares, p_(t)) == -3
