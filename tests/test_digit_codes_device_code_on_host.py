"""CPU: the three copies of the signed radix-2^c recoding every bucket MSM starts with — crypto_amd/csrc/digit_codes.hip.h digit_codes_one (2-byte codes up to
c = 16, 4-byte codes above: the per-window sweeps of the plain pipeline), crypto_amd/csrc/ps_digits.hip.h ps_digits<0, 0> (the partition sort at a run-time
width) and ps_digits<20, 13>, <17, 16>, <16, 16> (its constant-shift forms for the shapes of the tables and of the plain pipeline at 2^17 terms and more) —
compiled for the host as they are (tests/native/digit_codes_host_shim.cpp) and compared digit for digit, code spelling included, with the big-integer model
util.signed_digits at every window width 7 .. 22, on util.edge_scalars(c): scalars that put +B, -(B - 1), a zero digit that carries and the largest top digit
into the windows, single-digit probes, the partition borders of the sort, values in [r, 2^255), and seeded random ones."""
import ctypes as C
import os
import shutil
import subprocess
import numpy as np
import pytest
import util as U

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "digit_codes_host_shim.cpp")
SO = os.path.join(HERE, "native", "libdigit_codes_host_shim.so")
WIDTHS = list(range(7, 23))
FIXED = {20: 13, 17: 16, 16: 16}            # the constant-shift shapes: width -> windows


def hip_include():
    """the directory that holds hip/hip_runtime.h: $ROCM_PATH, next to the hipcc on the PATH, or /opt/rocm"""
    cands = [os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        cands.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    cands.append("/opt/rocm")
    for d in cands:
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    raise AssertionError("hip/hip_runtime.h not found (the headers the library itself is built with)")


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("digit_codes.hip.h", "ps_digits.hip.h", "sort_launch.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + hip_include(), "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    L.shim_codes16.argtypes = L.shim_codes32.argtypes = [vp, sz, sz, vp, i32, i32, vp, vp]
    L.shim_codes16.restype = L.shim_codes32.restype = None
    L.shim_ps_digits.argtypes = [i32, vp, sz, vp, i32, i32, vp, vp]
    L.shim_ps_part_log.argtypes = [C.c_uint32]
    return L


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def words(vals):
    """integers below 2^256 -> (n, 8) little-endian 32-bit words, the layout the kernels read"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint32).reshape(-1, 8).copy()


_FAMILY = {}


def family(c):
    """(scalars, model digits) of width c as tuples, computed once and shared by the tests"""
    if c not in _FAMILY:
        sc = tuple(U.edge_scalars(c, n_random=300))
        _FAMILY[c] = (sc, tuple(tuple(U.signed_digits(s, c)) for s in sc))
    return _FAMILY[c]


def stored_codes(shim, c, sc, skip=None, n_pad=None):
    """digit_codes_one over sc -> (codes (W, n_pad), bad flag); 2-byte codes up to c = 16, 4-byte codes above, as launch_digit_codes chooses"""
    W = U.window_shape(c)[0]
    n = len(sc)
    n_pad = (n + 7) & ~7 if n_pad is None else n_pad
    skip = np.zeros(n, np.uint8) if skip is None else np.asarray(skip, np.uint8)
    dig = np.full((W, n_pad), 0x5A5A, np.uint16 if c <= 16 else np.uint32)
    bad = np.zeros(1, np.uint32)
    (shim.shim_codes16 if c <= 16 else shim.shim_codes32)(p_(words(sc)), n, n_pad, p_(skip), c, W, p_(dig), p_(bad))
    return dig, int(bad[0])


def walked_digits(shim, shape, c, sc, live=None):
    """ps_digits over sc -> (|d| - 1, negative, non-zero), each (W, n)"""
    W = U.window_shape(c)[0]
    n = len(sc)
    live = np.ones(n, np.uint8) if live is None else np.asarray(live, np.uint8)
    out = np.full((W, n, 3), 0xA5A5A5A5, np.uint32)
    calls = np.zeros(n, np.uint32)
    assert shim.shim_ps_digits(shape, p_(words(sc)), n, p_(live), c, W, p_(out), p_(calls)) == 0
    assert (calls == W).all()                                                   # every window is reported, for idle lanes too (the wave-wide counters need all lanes)
    return out[:, :, 0], out[:, :, 1], out[:, :, 2]


def model_codes(digs, bits):
    return np.array([[U.digit_code(d, bits) for d in row] for row in digs], dtype=np.uint64).T      # (W, n)


@pytest.mark.parametrize("c", WIDTHS)
def test_model_and_edge_family(c):
    """the model is a recoding (signed_digits asserts range, sum and the absent carry itself), and the named members of the family have the digits they are built for"""
    W, B, M, t = U.window_shape(c)
    e = U.edge_named(c)
    assert U.signed_digits(e["maxpos"], c) == [B] * (W - 1) + [0]
    assert U.signed_digits(e["minneg"], c) == [-(B - 1)] * (W - 1) + [1]
    assert U.signed_digits(e["topmax"], c)[W - 2:] == [-(B - 1), 1 << t]
    assert U.signed_digits(e["zero_carry"], c)[:4] == [-(B - 1), 0, 1, 0]
    assert U.signed_digits(e["all_ones"], c) == [-1] + [0] * (W - 2) + [1 << t]
    assert ((1 << t) == B) == (c in (8, 16)) and (t == 0) == (c in (15, 17))
    sc, digs = family(c)
    assert len(set(sc)) == len(sc) and {0, 1, U.R - 1, U.R, U.R + 1, 1 << 254, (1 << 255) - 2} <= set(sc)
    assert U.edge_coverage_missing(sc, c) == []
    plain = U.ps_part_log(W * B)
    assert U.edge_coverage_missing(U.edge_scalars(c, part_logs=[plain]), c, part_log=plain, per_window=True) == []


def test_partition_width_port(shim):
    """util.ps_part_log is sort_launch.hip.h's ps_part_log"""
    for NB in [1, 2, 31, 32, 33, 64] + [v + k for lg in range(7, 27) for v in (1 << lg, 3 << (lg - 1)) for k in (-1, 0, 1)] + [W * B for c in WIDTHS for W, B, _, _ in [U.window_shape(c)]]:
        assert shim.shim_ps_part_log(NB) == U.ps_part_log(NB), NB


@pytest.mark.parametrize("c", WIDTHS)
def test_stored_codes_equal_the_model(shim, c):
    """digit_codes_one: every code of every window, the padding entries, and no bad-scalar flag for values below 2^255"""
    sc, digs = family(c)
    bits = 16 if c <= 16 else 32
    got, bad = stored_codes(shim, c, sc)
    n = len(sc)
    want = model_codes(digs, bits)
    assert bad == 0
    assert (got[:, :n].astype(np.uint64) == want).all(), np.argwhere(got[:, :n].astype(np.uint64) != want)[:8]
    assert (got[:, n:] == (1 << bits) - 1).all()                                 # padding: zero digits
    if c == 16:                                                                  # the three codes next to each other at the top of the 16-bit range stay apart
        B = U.window_shape(c)[1]
        D, g = np.array(digs, dtype=np.int64).T, got[:, :n]
        for code, d in ((0x7FFF, B), (0xFFFE, -(B - 1)), (0xFFFF, 0)):
            assert (g == code).any() and ((g == code) == (D == d)).all(), hex(code)


@pytest.mark.parametrize("c", WIDTHS)
def test_walked_digits_equal_the_model(shim, c):
    """ps_digits at a run-time width, and the constant-shift form where the width has one: magnitude, sign and the non-zero mark of every window"""
    sc, digs = family(c)
    D = np.array(digs, dtype=np.int64).T                                         # (W, n)
    for shape in [0] + ([c] if c in FIXED else []):
        if shape:
            assert U.window_shape(c)[0] == FIXED[c]
        m1, neg, nz = walked_digits(shim, shape, c, sc)
        assert (nz == (D != 0)).all(), (shape, np.argwhere(nz != (D != 0))[:8])
        on = D != 0
        assert (m1[on] == (np.abs(D) - 1)[on]).all(), (shape, np.argwhere(on & (m1 != np.abs(D) - 1))[:8])
        assert (neg[on] == (D < 0)[on]).all(), (shape, np.argwhere(on & (neg != (D < 0)))[:8])
        # (a zero digit's magnitude and sign are not read by the kernels: the zero that carries reports itself negative)


@pytest.mark.parametrize("c", WIDTHS)
def test_skipped_and_idle_entries_are_zero_digits(shim, c):
    """an identity base (`skip`) or a lane without a scalar contributes the zero code in every window, its neighbours are untouched — and a skipped scalar
    still raises the bad flag"""
    sc, digs = family(c)
    sc, digs = sc[:40], digs[:40]
    bits = 16 if c <= 16 else 32
    skip = np.zeros(len(sc), np.uint8); skip[[0, 1, 7, 8, 39]] = 1
    got, bad = stored_codes(shim, c, sc, skip)
    want = model_codes(digs, bits)
    want[:, skip == 1] = (1 << bits) - 1
    assert bad == 0 and (got[:, :len(sc)].astype(np.uint64) == want).all()
    for shape in [0] + ([c] if c in FIXED else []):
        m1, neg, nz = walked_digits(shim, shape, c, sc, live=1 - skip)
        assert (nz[:, skip == 1] == 0).all()
        assert (nz[:, skip == 0] == (np.array(digs, dtype=np.int64).T != 0)[:, skip == 0]).all()
    hi = list(sc); hi[7] |= 1 << 255
    assert stored_codes(shim, c, hi, skip)[1] == 1


@pytest.mark.parametrize("c", WIDTHS)
def test_bad_flag_is_bit_255(shim, c):
    """*bad is set exactly when a scalar has bit 255 set; the digits are those of the low 255 bits either way"""
    sc, digs = family(c)
    bits = 16 if c <= 16 else 32
    for k in (0, 5, len(sc) - 1):
        one = [sc[k] | (1 << 255)]
        got, bad = stored_codes(shim, c, one)
        assert bad == 1 and (got[:, 0].astype(np.uint64) == model_codes([digs[k]], bits)[:, 0]).all()
        m1, neg, nz = walked_digits(shim, 0, c, one)
        assert (nz[:, 0] == (np.array(digs[k]) != 0)).all()
    assert stored_codes(shim, c, [(1 << 255) - 1, (1 << 255) - 2, 1 << 254, U.R])[1] == 0
    assert stored_codes(shim, c, [0, 1 << 255])[1] == 1
    mixed = list(sc[:30]); mixed[17] |= 1 << 255
    got, bad = stored_codes(shim, c, mixed)
    assert bad == 1 and (got[:, :30].astype(np.uint64) == model_codes(digs[:30], bits)).all()
