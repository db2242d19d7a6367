"""CPU: the key generator's device routines (crypto_amd/csrc/fr29.hip.h: fr_inv, the chunked batch inversion fr_batch_inv, the balanced column
fold fr_fold_chunk) compiled for the host with the FP29_CHECK operand asserts (tests/native/setup_dev_host_shim.cpp), checked against Python big
integers, plus the two new entry points in the header and the library's exports.  A green run shows the routines compute the field's values and
that no product of theirs leaves its operand contract, on columns of one entry, of a chunk +- 1, and of several chunks."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "setup_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libsetup_dev_host_shim.so")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CH = 64            # setupk::FOLD_CHUNK
p_ = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC, os.path.join(ROOT, "crypto_amd", "csrc", "fr29.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.shim_batch_inv.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    L.shim_fold.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int]
    L.shim_fold.restype = C.c_int
    L.shim_fr_inv.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    return L


def words(vals):
    return np.array([(v >> (32 * k)) & 0xFFFFFFFF for v in vals for k in range(8)], dtype=np.uint32)


def ints(w):
    w = w.reshape(-1, 8)
    return [sum(int(x) << (32 * k) for k, x in enumerate(row)) for row in w]


@pytest.mark.parametrize("stress", [0, 1])
def test_fr_inv(shim, stress):
    rng = np.random.default_rng(11)
    vals = [1, 2, R - 1, R - 2, (R - 1) // 2, 7] + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(10)]
    for v in vals:
        out = np.zeros(8, np.uint32)
        shim.shim_fr_inv(p_(words([v])), p_(out), stress)
        assert ints(out)[0] == pow(v, R - 2, R), v
    out = np.zeros(8, np.uint32)
    shim.shim_fr_inv(p_(words([0])), p_(out), stress)
    assert ints(out)[0] == 0                       # 0^(r-2)


@pytest.mark.parametrize("n,G", [(1, 1), (2, 1), (31, 4), (64, 2), (257, 8), (1000, 1000)])
@pytest.mark.parametrize("stress", [0, 1])
def test_batch_inversion(shim, n, G, stress):
    rng = np.random.default_rng(n * 7 + G)
    vals = [int.from_bytes(rng.bytes(32), "little") % (R - 1) + 1 for _ in range(n)]
    out = np.zeros(8 * n, np.uint32)
    shim.shim_batch_inv(n, G, p_(words(vals)), p_(out), stress)
    assert ints(out) == [pow(v, R - 2, R) for v in vals]


def fold(shim, keys, vals, nv, stress):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    out = np.zeros(8 * nv, np.uint32)
    passes = shim.shim_fold(len(keys), p_(keys), p_(words(vals)), CH, nv, p_(out), stress)
    assert passes >= 1, "a key was completed twice"
    want = [0] * nv
    for k, v in zip(keys, vals):
        want[int(k)] = (want[int(k)] + v) % R
    assert ints(out) == want
    return passes


@pytest.mark.parametrize("stress", [0, 1])
@pytest.mark.parametrize("col", [1, CH - 1, CH, CH + 1, 2 * CH - 1, 2 * CH + 1, 5 * CH + 3, 40 * CH])
def test_balanced_fold_one_long_column(shim, col, stress):
    """a column of `col` entries between short ones (the nconstraints circuit's C: variable 0 in every row)"""
    rng = np.random.default_rng(col)
    keys = [0] * 3 + [1] * col + [2] + [3] * (col // 3 + 1) + [5] * 2
    vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in keys]
    fold(shim, keys, vals, 7, stress)
    vals = [R - 1] * len(keys)                       # every entry the largest residue
    fold(shim, keys, vals, 7, stress)


def test_balanced_fold_many_passes(shim):
    """64^2 + a few entries in one column: three passes, partials of partials folded"""
    n = CH * CH * 2 + 5
    keys = [0] * n + [1, 1, 2]
    vals = list(range(1, len(keys) + 1))
    assert fold(shim, keys, vals, 3, 1) >= 3


def test_balanced_fold_random_shapes(shim):
    rng = np.random.default_rng(5)
    for trial in range(6):
        nv = int(rng.integers(1, 300))
        lens = rng.integers(0, 3 * CH, size=nv) * (rng.random(nv) < 0.5)
        keys = np.repeat(np.arange(nv), lens)
        if len(keys) == 0:
            continue
        vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in keys]
        fold(shim, keys, vals, nv, trial & 1)


def test_header_and_exports_name_the_setup_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dock_gpu.h")).read()
    for name in ("dgpu_qap_instance_map", "dgpu_legogroth16_setup"):
        assert re.search(r"int32_t %s\s*\(" % name, hdr), name
    so = os.path.join(ROOT, "crypto_amd", "libdock_gpu.so")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    for name in ("dgpu_qap_instance_map", "dgpu_legogroth16_setup"):
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
