"""CPU: the DEVICE routines of the SAVER kernels (crypto_amd/csrc/saver_kernels.hip.h) compiled for the host (tests/native/saver_dev_host_shim.cpp).  The
discrete-log lookup is the ONE function k_gt_dlog_lookup calls: it is driven over synthetic tables — a hit at the first, the last and a middle entry, misses
below, above and between, runs of two and of all-equal fingerprints with the hit at either end of the run, the value one, and the compare-at-index mode with
m = 0, 2^b - 1 and 2^b.  The row verdict runs on every miss pattern for K = 1, 2, 3.  The table's group body runs under the FP29_CHECK bound tracker, six threads
as the six lanes of a group, for b = 1 .. 5 against the oracle's fp12_pow: a green run shows the doubling rounds write the powers and that the lazy limbs
cannot overflow."""
import ctypes as C
import itertools
import os
import subprocess
import numpy as np
import pytest
import oracle_c as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "saver_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libsaver_dev_host_shim.so")
p_ = lambda a: a.ctypes.data_as(C.c_void_p)
FULL = 2 ** 64 - 1
MISS = -1


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(HERE, "..", "crypto_amd", "csrc", f) for f in ("saver_kernels.hip.h", "gt_kernels.hip.h", "pairing29.hip.h", "fp29.hip.h", "fp2_29.hip.h",
                                                                                "fp_safegcd.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.shim_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32]
    L.shim_fingerprint.restype = C.c_uint64
    L.shim_fingerprint.argtypes = [C.c_void_p, C.c_uint64]
    L.shim_row_verdict.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.shim_table_from_base.argtypes = [C.c_void_p, C.c_uint32]
    return L


ONE = np.asarray(O.fp12_one(), np.uint64)


class Table:
    """E synthetic entries: entry m (1-based) has the fingerprint fps[m - 1] in its first word and a body that names m, so that entries with equal
    fingerprints still differ — in their LAST word only, which a compare that stopped early would miss"""
    def __init__(self, fps, mask=FULL):
        self.E, self.mask = len(fps), mask
        self.tab = np.full((self.E, 72), 0x1111111111111111, np.uint64)
        self.tab[:, 0] = np.array(fps, np.uint64)
        self.tab[:, 71] = np.arange(1, self.E + 1, dtype=np.uint64)
        order = sorted(range(self.E), key=lambda k: (fps[k] & mask, k))
        self.fps = np.array([fps[k] & mask for k in order], np.uint64)
        self.ms = np.array([k + 1 for k in order], np.uint16)

    def lookup(self, shim, p, at_index=False, m=0):
        p = np.ascontiguousarray(p, np.uint64)
        return shim.shim_lookup(p_(p), p_(ONE), p_(self.tab), p_(self.fps), p_(self.ms), self.E, self.mask, 1 if at_index else 0, m)

    def value(self, fp, tag):
        v = np.full(72, 0x1111111111111111, np.uint64); v[0] = fp; v[71] = tag
        return v


def test_hits_and_misses_over_distinct_fingerprints(shim):
    fps = [50, 10, 40, 20, 30, 70, 60]                                     # entry m has fingerprint fps[m - 1]: the index is not the table's order
    t = Table(fps)
    for m in range(1, 8):
        assert t.lookup(shim, t.tab[m - 1]) == m
    assert t.lookup(shim, t.tab[1]) == 2 and t.lookup(shim, t.tab[5]) == 6      # the first and the last of the index
    for fp in (5, 75, 35, 2 ** 64 - 1, 0):                                 # below, above, between
        assert t.lookup(shim, t.value(fp, 1)) == MISS
    assert t.lookup(shim, t.value(40, 99)) == MISS                        # the fingerprint of entry 3 with another body: the full compare decides
    v = t.tab[2].copy(); v[35] ^= 1
    assert t.lookup(shim, v) == MISS
    assert shim.shim_fingerprint(p_(t.tab[0]), FULL) == 50 and shim.shim_fingerprint(p_(t.tab[0]), 7) == 2
    # the high half of the fingerprint is the second 32-bit word
    hi = Table([1 << 32, 1, (1 << 32) + 1])
    assert [hi.lookup(shim, hi.tab[k]) for k in range(3)] == [1, 2, 3]


def test_runs_of_equal_fingerprints(shim):
    t = Table([10, 20, 20, 30, 30, 30, 40])                               # runs of 2 and 3 inside
    for m in range(1, 8):
        assert t.lookup(shim, t.tab[m - 1]) == m
    assert t.lookup(shim, t.value(20, 4)) == MISS and t.lookup(shim, t.value(30, 2)) == MISS      # in a run's fingerprint, no member of the run
    ends = Table([20, 20, 30, 40, 40])                                    # runs at both ends of the index
    assert [ends.lookup(shim, ends.tab[k]) for k in range(5)] == [1, 2, 3, 4, 5]
    assert ends.lookup(shim, ends.value(40, 9)) == MISS                   # the scan stops at the end of the column
    for E in (1, 2, 15):                                                  # all-equal: by a mask of no bits, and by equal words
        for t in (Table(list(range(100, 100 + E)), mask=0), Table([7] * E)):
            assert [t.lookup(shim, t.tab[k]) for k in range(E)] == list(range(1, E + 1))
            assert t.lookup(shim, t.value(100, 77)) == MISS
    t = Table(list(range(8, 23)), mask=7)                                  # 3 bits over fifteen entries: runs by pigeonhole
    assert [t.lookup(shim, t.tab[k]) for k in range(15)] == list(range(1, 16))
    assert len(set(t.fps.tolist())) == 8


def test_one_and_compare_at_index(shim):
    b = 4
    E = (1 << b) - 1
    t = Table(list(range(1000, 1000 + E)))
    assert t.lookup(shim, ONE) == 0
    withone = Table([int(ONE[0])] * 3); withone.tab[1] = ONE              # an entry that IS one (a base of one): zero comes first, as in the reference
    assert withone.lookup(shim, ONE) == 0
    # compare-at-index: entry m and nothing else
    assert t.lookup(shim, ONE, True, 0) == 0 and t.lookup(shim, t.tab[0], True, 0) == MISS
    assert t.lookup(shim, t.tab[E - 1], True, E) == E and t.lookup(shim, t.tab[E - 2], True, E) == MISS
    assert t.lookup(shim, t.tab[E - 1], True, E + 1) == MISS and t.lookup(shim, ONE, True, E + 1) == MISS and t.lookup(shim, t.tab[0], True, 65535) == MISS
    assert t.lookup(shim, t.tab[6], True, 7) == 7 and t.lookup(shim, t.tab[6], True, 8) == MISS and t.lookup(shim, ONE, True, 7) == MISS


@pytest.mark.parametrize("K", [1, 2, 3])
def test_row_verdict_on_every_miss_pattern(shim, K):
    for pattern in itertools.product((0, 1), repeat=K):
        miss = np.array(pattern, np.uint8)
        chunks = np.arange(5, 5 + K, dtype=np.uint16)
        st = shim.shim_row_verdict(p_(miss), K, p_(chunks))
        assert st == (1 if any(pattern) else 0)
        assert chunks.tolist() == ([0] * K if any(pattern) else list(range(5, 5 + K)))


@pytest.mark.parametrize("b", [1, 2, 3, 4, 5])
def test_table_rounds_write_the_powers(shim, b):
    E = (1 << b) - 1
    base = np.asarray(O.final_exponentiation(O.multi_miller_loop(O.G1.generator().reshape(1, 12), O.G2.generator().reshape(1, 24))), np.uint64)
    base = np.asarray(O.fp12_pow(base, 0xC0FFEE + b), np.uint64)
    tab = np.zeros((E, 72), np.uint64)
    tab[0] = base
    shim.shim_table_from_base(p_(tab), E)
    for m in range(1, E + 1):
        assert (tab[m - 1] == np.asarray(O.fp12_pow(base, m), np.uint64)).all(), m
