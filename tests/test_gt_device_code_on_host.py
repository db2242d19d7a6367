"""CPU: the DEVICE GT routines (crypto_amd/csrc/gt_kernels.hip.h: the lane-group Fp12 product, Granger-Scott squaring, Frobenius maps, inverse,
exp_by_x, the Miller-loop tail and the final exponentiation) compiled for the host with the FP29_CHECK bound tracker (tests/native/gt_dev_host_shim.cpp,
six threads as the six lanes of a group), checked word for word against dgpu_final_exponentiation (host code, no device), the C oracle and, on a few
elements, the big-integer model.  A green run shows the lane split computes the host's values and its lazy-limb arithmetic cannot overflow."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import bls12_381_model as M
import oracle_c as O
import util as U
from crypto_amd._native import lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "gt_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libgt_dev_host_shim.so")
P = U.P
X_ABS = 0xd201000000010000
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(HERE, "..", "crypto_amd", "csrc", f) for f in ("gt_kernels.hip.h", "pairing29.hip.h", "fp29.hip.h", "fp2_29.hip.h", "fp_safegcd.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", SO, SRC])
    return C.CDLL(SO)


def words(vals):
    """72 ABI words from 12 field residues (already in Montgomery form)"""
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in vals for k in range(6)], dtype=np.uint64)


def residues(w):
    return [sum(int(w[6 * i + k]) << (64 * k) for k in range(6)) for i in range(12)]


def rand_f12(rng):
    return words([int.from_bytes(rng.bytes(48), "little") % P for _ in range(12)])


def conj(w):
    r = residues(w)
    return words(r[:6] + [(P - v) % P for v in r[6:]])


def host_fe(f):
    out = np.zeros(72, np.uint64)
    rc = lib().dgpu_final_exponentiation(p_(np.ascontiguousarray(f)), p_(out))
    return rc, out


def dev_fe(shim, f):
    out = np.zeros(72, np.uint64)
    z = shim.shim_final_exp(p_(np.ascontiguousarray(f)), p_(out))
    return z, out


def dev_op(shim, op, a, b=None):
    out = np.zeros(72, np.uint64)
    shim.shim_op(op, p_(np.ascontiguousarray(a)), p_(None if b is None else np.ascontiguousarray(b)), p_(out))
    return out


def miller_outputs(k):
    g1 = lambda s: O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(s, 4)))[0]
    g2 = lambda s: O.G2.to_affine(O.G2.mul(O.G2.generator(), O.int_to_limbs(s, 4)))[0]
    return [np.asarray(O.multi_miller_loop(g1(3 + i).reshape(1, 12), g2(5 + 2 * i).reshape(1, 24)), dtype=np.uint64).reshape(72) for i in range(k)]


def inputs():
    rng = np.random.default_rng(2024)
    one = O.fp12_one()
    r1 = residues(one)
    minus_one = words([(P - r1[0]) % P] + r1[1:])
    pm1 = words([P - 1] * 12)
    sparse = words([0] * 12); sparse[6 * 3] = 5                         # one coefficient word set
    sparse2 = words([r1[0], 0, 0, 0, 0, 0, 0, 0, 7, 0, 0, 0])
    raw = miller_outputs(3)
    gt = [O.final_exponentiation(m) for m in raw[:2]]
    return {"one": one, "minus_one": minus_one, "p_minus_1": pm1, "sparse": sparse, "sparse2": sparse2,
            **{"random%d" % i: rand_f12(rng) for i in range(4)}, **{"miller%d" % i: m for i, m in enumerate(raw)},
            **{"gt%d" % i: g for i, g in enumerate(gt)}}


@pytest.mark.parametrize("name", sorted(inputs().keys()))
def test_final_exponentiation_matches_host_and_oracle(shim, name):
    f = inputs()[name]
    rc, want = host_fe(f)
    assert rc == 0
    z, got = dev_fe(shim, f)
    assert z == 0
    assert (got == want).all(), name
    assert (np.asarray(O.final_exponentiation(f), np.uint64) == want).all()


def test_zero_is_flagged_with_zero_words(shim):
    f = np.zeros(72, np.uint64)
    assert host_fe(f)[0] == -5                                                         # DGPU_E_ZERO
    z, got = dev_fe(shim, f)
    assert z == 1 and not got.any()


def to_model(w):
    c = [M.fp_from_mont_limbs(w[6 * i:6 * i + 6]) for i in range(12)]
    f2 = [(c[2 * k], c[2 * k + 1]) for k in range(6)]
    return (tuple(f2[:3]), tuple(f2[3:]))


def test_final_exponentiation_against_the_model(shim):
    rng = np.random.default_rng(5)
    for f in (miller_outputs(1)[0], rand_f12(rng)):
        z, got = dev_fe(shim, f)
        assert z == 0 and to_model(got) == M.final_exponentiation(to_model(f))


def test_steps_one_at_a_time(shim):
    rng = np.random.default_rng(7)
    raw = miller_outputs(2)
    cyc = [O.fp12_pow(m, (P ** 6 - 1) * (P ** 2 + 1)) for m in raw]     # cyclotomic subgroup
    for a in [rand_f12(rng), rand_f12(rng), raw[0], O.fp12_one()]:
        b = rand_f12(rng)
        assert (dev_op(shim, 0, a, b) == np.asarray(O.fp12_mul(a, b), np.uint64)).all()              # product
        assert (dev_op(shim, 0, a, a) == np.asarray(O.fp12_mul(a, a), np.uint64)).all()              # product with itself
        assert (dev_op(shim, 2, a) == np.asarray(O.fp12_pow(a, P), np.uint64)).all()                 # Frobenius p
        assert (dev_op(shim, 3, a) == np.asarray(O.fp12_pow(a, P * P), np.uint64)).all()             # Frobenius p^2
        assert (dev_op(shim, 5, a) == conj(a)).all()
        inv = dev_op(shim, 4, a)
        assert (np.asarray(O.fp12_mul(a, inv), np.uint64) == np.asarray(O.fp12_one(), np.uint64)).all()   # inverse
    for c in cyc:
        assert (dev_op(shim, 1, c) == np.asarray(O.fp12_mul(c, c), np.uint64)).all()                 # Granger-Scott on cyclotomic elements
        want = conj(np.asarray(O.fp12_pow(c, X_ABS), np.uint64))
        assert (dev_op(shim, 6, c) == want).all()                                                    # exp_by_x = c^x, x < 0
    assert not dev_op(shim, 4, np.zeros(72, np.uint64)).any()                                        # 0^-1 -> 0


def test_miller_tail_matches_the_host_tail(shim):
    rng = np.random.default_rng(11)
    for L in ([rand_f12(rng) for _ in range(68)], [O.fp12_one()] * 67 + [rand_f12(rng)]):
        f, idx = L[0], 1
        for b in range(62, -1, -1):
            if b != 62:
                f = O.fp12_mul(O.fp12_mul(f, f), L[idx]); idx += 1
            if (X_ABS >> b) & 1:
                f = O.fp12_mul(f, L[idx]); idx += 1
        assert idx == 68
        out = np.zeros(72, np.uint64)
        shim.shim_miller_tail(p_(np.ascontiguousarray(np.stack(L))), p_(out))
        assert (out == conj(np.asarray(f, np.uint64))).all()
