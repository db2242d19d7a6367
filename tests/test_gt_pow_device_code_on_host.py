"""CPU: the DEVICE GT power routines (crypto_amd/csrc/gt_kernels.hip.h: gt_signed_digits, gt_pow_table / gt_pow_cyc, gt_pow_generic, the fold level,
gt_in_cyclotomic / gt_in_gt — the group bodies k_gt_pow.hip launches) compiled for the host with the FP29_CHECK bound tracker
(tests/native/gt_pow_host_shim.cpp, six threads as the six lanes of a group), word for word against the host entry points dgpu_fp12_pow,
dgpu_fp12_multi_pow, dgpu_fp12_mul, dgpu_gt_in_subgroup and the C oracle.  A green run shows the lane split computes the host's values on every kind
of base and that its lazy-limb arithmetic cannot overflow."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import oracle_c as O
import util as U
from crypto_amd._native import lib
from test_gt_host import elements

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "gt_pow_host_shim.cpp")
SO = os.path.join(HERE, "native", "libgt_pow_host_shim.so")
R, P = U.R, U.P
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
limbs = lambda v: np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)
EDGE = [0, 1, 7, 8, 9, int("8" * 64, 16), int("8" * 63 + "9", 16), 2 ** 255, 2 ** 256 - 1, R - 1, R]


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(HERE, "..", "crypto_amd", "csrc", f) for f in ("gt_kernels.hip.h", "pairing29.hip.h", "fp29.hip.h", "fp2_29.hip.h", "fp_safegcd.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", SO, SRC])
    return C.CDLL(SO)


@pytest.fixture(scope="module")
def kinds():
    raw, gt, cyc = elements()
    return {"gt": gt, "cyc": cyc, "raw": raw, "zero": [np.zeros(72, np.uint64)], "one": [np.asarray(O.fp12_one(), np.uint64)]}


def exponents():
    rng = np.random.default_rng(77)
    return EDGE + [int.from_bytes(rng.bytes(32), "little") for _ in range(20)]


def host_pow(a, e):
    out = np.zeros(72, np.uint64)
    assert lib().dgpu_fp12_pow(p_(np.ascontiguousarray(a)), p_(limbs(e)), p_(out)) == 0
    return out


def host_multi(bases, exps):
    a = np.ascontiguousarray(np.stack(bases)); e = np.ascontiguousarray(np.stack([limbs(x) for x in exps])); out = np.zeros(72, np.uint64)
    assert lib().dgpu_fp12_multi_pow(p_(a), p_(e), len(bases), p_(out)) == 0
    return out


def dev_pow(shim, bases, exps, k=None, generic=False, out_abi=True, e_stride=4):
    a = np.ascontiguousarray(np.stack(bases)); e = np.ascontiguousarray(np.stack([limbs(x) for x in exps])); out = np.zeros(72, np.uint64)
    short = shim.shim_pow_group(p_(a), p_(e), e_stride, len(bases), k or len(bases), 1 if generic else 0, 1 if out_abi else 0, p_(out))
    return out, short


def test_signed_digits(shim):
    rng = np.random.default_rng(3)
    d = np.zeros(65, np.int8)
    for e in EDGE + [int.from_bytes(rng.bytes(32), "little") for _ in range(10000)]:
        shim.shim_signed_digits(p_(limbs(e)), p_(d))
        dl = [int(v) for v in d]
        assert sum(v * 16 ** w for w, v in enumerate(dl)) == e, hex(e)
        assert all(-7 <= v <= 8 for v in dl) and dl[64] in (0, 1), hex(e)
    shim.shim_signed_digits(p_(limbs(int("8" * 64, 16))), p_(d))
    assert [int(v) for v in d] == [8] * 64 + [0]                          # no carry anywhere
    shim.shim_signed_digits(p_(limbs(int("8" * 63 + "9", 16))), p_(d))
    assert [int(v) for v in d] == [-7] * 64 + [1]                         # a carry through all 64 digits


@pytest.mark.parametrize("kind", ["gt", "cyc", "raw", "zero", "one"])
def test_powers_on_every_kind_of_base(shim, kinds, kind):
    cyclotomic = kind in ("gt", "cyc", "one")
    for n, e in enumerate(exponents()):
        a = kinds[kind][n % len(kinds[kind])]
        want = host_pow(a, e)
        assert (np.asarray(O.fp12_pow(a, e), np.uint64) == want).all(), hex(e)
        got, short = dev_pow(shim, [a], [e], generic=True)
        assert short == 0 and (got == want).all(), (kind, "generic", hex(e))
        got, short = dev_pow(shim, [a], [e], out_abi=bool(n & 1))          # the path the kernel picks
        assert short == (1 if cyclotomic else 0) and (got == want).all(), (kind, "auto", hex(e))


def test_zero_to_the_zero_is_one_and_zero_stays_zero(shim, kinds):
    z = kinds["zero"][0]
    assert (dev_pow(shim, [z], [0])[0] == kinds["one"][0]).all()
    assert not dev_pow(shim, [z], [5])[0].any()


@pytest.mark.parametrize("k", [2, 3, 8])
def test_groups_of_k_bases(shim, kinds, k):
    ex = exponents()
    gt, cyc, raw = kinds["gt"], kinds["cyc"], kinds["raw"]
    pool = gt + cyc + [kinds["one"][0]]
    for rep in range(3):
        bases = [pool[(rep + 2 * j) % len(pool)] for j in range(k)]
        es = [ex[(5 * rep + 3 * j) % len(ex)] for j in range(k)]
        want = host_multi(bases, es)
        got, short = dev_pow(shim, bases, es, out_abi=False)
        assert short == 1 and (got == want).all(), (k, rep)
        got, short = dev_pow(shim, bases, es, generic=True)
        assert short == 0 and (got == want).all(), (k, rep, "generic")
    bases = [pool[j % len(pool)] for j in range(k - 1)] + [raw[0]]         # one raw base sends the group down the generic path
    es = [ex[(11 + j) % len(ex)] for j in range(k)]
    got, short = dev_pow(shim, bases, es)
    assert short == 0 and (got == host_multi(bases, es)).all()
    # a group with room for k bases that holds fewer: the missing ones count as one
    got, short = dev_pow(shim, bases[:k - 1], es[:k - 1], k=k)
    assert short == 1 and (got == host_multi(bases[:k - 1], es[:k - 1])).all()
    # one exponent for all (stride 0)
    got, _ = dev_pow(shim, bases[:k - 1], es[:1], k=k - 1, e_stride=0)
    assert (got == host_multi(bases[:k - 1], es[:1] * (k - 1))).all()


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 65])
def test_fold_levels(shim, kinds, n):
    pool = kinds["gt"] + kinds["raw"] + kinds["cyc"] + kinds["one"]
    cur = np.ascontiguousarray(np.stack([pool[(3 * i + 1) % len(pool)] for i in range(n)]))
    want = cur[0].copy()
    for i in range(1, n):
        t = np.zeros(72, np.uint64)
        assert lib().dgpu_fp12_mul(p_(want), p_(np.ascontiguousarray(cur[i])), p_(t)) == 0
        want = t
    level = 0
    while True:
        out = np.zeros(((len(cur) + 7) // 8, 72), np.uint64)
        assert shim.shim_fold_level(p_(cur), len(cur), level & 1, p_(out)) == len(out)
        cur, level = out, level + 1
        if len(cur) == 1:
            break
    assert (cur[0] == want).all()


def test_membership_on_every_kind(shim, kinds):
    gt, cyc, raw = kinds["gt"], kinds["cyc"], kinds["raw"]
    one = kinds["one"][0]
    h_only = O.fp12_pow(cyc[0], R)
    allv = gt + [one, O.fp12_mul(gt[0], O.fp12_pow(gt[1], 12345))] + cyc + [h_only, O.fp12_mul(gt[0], cyc[1])] + raw + kinds["zero"]
    a = np.ascontiguousarray(np.stack([np.asarray(v, np.uint64) for v in allv]))
    ok = np.zeros(len(allv), np.uint8)
    assert lib().dgpu_gt_in_subgroup(p_(a), len(allv), p_(ok)) == 0
    in_cyc = lambda f: bool(f.any()) and bool((np.asarray(O.fp12_pow(f, P ** 4 - P ** 2 + 1), np.uint64) == one).all())
    for i, f in enumerate(a):
        r = shim.shim_membership(p_(np.ascontiguousarray(f)))
        in_gt = bool(f.any()) and bool((np.asarray(O.fp12_pow(f, R), np.uint64) == one).all())
        assert bool(r & 2) == in_gt == bool(ok[i]), i
        assert bool(r & 1) == in_cyc(f), i
    assert list(ok[:5]) == [1] * 5 and not ok[5:].any()
