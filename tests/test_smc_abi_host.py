"""CPU: the host-side contract of the two dgpu_smc_* calls (include/dock_gpu_smc.h, served by libdock_gpu_smc.so and its development build, NOT by the product or
the SAVER libraries) — what can be decided without a device: the header, crypto_amd/_native.py and the libraries' exports agree, the product, its twin and both
SAVER images export none of the names, n = 0 is DGPU_OK with every pointer NULL and the empty batch verifies, every DGPU_E_BADARG case of the header answers so
before the device is looked at (NULL pointers with n > 0, sides outside {1, 2}, l = 65, n = 2^31, a zero random or rho in either form), l = 0 needs no digit
arrays, and a well-formed call is stopped by the missing device only."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
slib = lambda: _native.smc_lib(bring_up=False)                   # libdock_gpu_smc.so, not brought up on a device
sdev = lambda: _native._load(_native._SMC_DEV_SO)                # its development build

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
PREPARED_WORDS = 68 * 36
vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
HEAD = [vp] * 5 + [i32, sz] + [vp] * 8 + [sz, i32]
SIGNATURES = {"dgpu_smc_range_proofs_verify_each_g1": HEAD + [vp, vp, vp],
              "dgpu_smc_range_proofs_verify_batch_g1": HEAD + [vp, C.POINTER(i32)]}
S, L_, N = 2, 3, 2
NAMES = ["g1", "g", "h", "pk", "g2", "sides", "l", "w", "consts", "C", "dpts", "dresp", "spts", "sresp", "c", "n", "mont"]


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(v):
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], np.uint64)


def test_symbols_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "dock_gpu_smc.h")).read()
    assert sorted(set(re.findall(r"\b(dgpu_smc_[a-z0-9_]+)\s*\(", hdr))) == sorted(SIGNATURES) == sorted(_native.SMC_SYMBOLS)
    saver, saver_dev = _native.saver_lib(bring_up=False), _native._load(_native._SAVER_DEV_SO)
    for name, args in SIGNATURES.items():
        assert name not in _native.SYMBOLS + _native.DEV_SYMBOLS + _native.SAVER_SYMBOLS
        for other in (lib(), dev_lib(), saver, saver_dev):
            assert not hasattr(other, name)
        for L in (slib(), sdev()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args, name
    exported = lambda so: sorted(l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "crypto_amd", so)], text=True).splitlines() if " T dgpu_" in l)
    assert exported("libdock_gpu_smc.so") == sorted(_native.SYMBOLS + _native.SMC_SYMBOLS)
    assert exported("libdock_gpu_smc_dev.so") == sorted(_native.SYMBOLS + _native.SMC_SYMBOLS + _native.DEV_SYMBOLS)
    for so in ("libdock_gpu.so", "libdock_gpu_dev.so", "libdock_gpu_saver.so", "libdock_gpu_saver_dev.so"):
        assert not [s for s in exported(so) if "smc" in s], so
    assert hasattr(sdev(), "dgpu_set_many_chunk_rows") and not hasattr(slib(), "dgpu_set_many_chunk_rows")      # the knob that cuts the chunks: the development build alone


class Args:
    def __init__(self, sides=S, l=L_, n=N):
        one = lambda *shape: np.ones(shape, np.uint64)
        self.v = dict(g1=one(12), g=one(12), h=one(12), pk=one(PREPARED_WORDS), g2=one(PREPARED_WORDS), sides=sides, l=l, w=one(max(l, 1), 4), consts=one(sides * 3, 4),
                      C=one(n, 12), dpts=one(max(n * sides * l, 1), 3, 12), dresp=one(max(n * sides * l, 1), 2, 4), spts=one(n * sides, 12), sresp=one(n * sides, 4), c=one(n, 4),
                      n=n, mont=0)
        self.random, self.rho = one(n, 4), limbs(5)
        self.status, self.detail, self.ok = np.full(n, 9, np.uint8), np.full(n, -9, np.int32), C.c_int32(-7)

    def head(self, **kw):
        v = dict(self.v, **kw)
        return [p_(v[k]) if isinstance(v[k], np.ndarray) else v[k] for k in NAMES]

    def each(self, L, random=None, status=True, detail=True, **kw):
        return L.dgpu_smc_range_proofs_verify_each_g1(*self.head(**kw), random, p_(self.status) if status else None, p_(self.detail) if detail else None)

    def batch(self, L, rho=True, ok=True, **kw):
        return L.dgpu_smc_range_proofs_verify_batch_g1(*self.head(**kw), (p_(self.rho) if rho is True else rho), C.byref(self.ok) if ok else None)


@pytest.mark.parametrize("L", [slib, sdev], ids=["smc", "smc-dev"])
def test_n_zero_needs_nothing(L):
    L = L()
    ok = C.c_int32(-7)
    nulls = [None] * 5 + [0, 0] + [None] * 8 + [0, 0]
    assert L.dgpu_smc_range_proofs_verify_each_g1(*nulls, None, None, None) == OK
    assert L.dgpu_smc_range_proofs_verify_batch_g1(*nulls, None, C.byref(ok)) == OK and ok.value == 1      # an empty batch verifies
    assert L.dgpu_smc_range_proofs_verify_batch_g1(*nulls, None, None) == OK
    nulls[5], nulls[6] = 7, 1000                                                                            # ... before sides and l are looked at
    assert L.dgpu_smc_range_proofs_verify_each_g1(*nulls, None, None, None) == OK


@pytest.mark.parametrize("L", [slib, sdev], ids=["smc", "smc-dev"])
def test_bad_arguments_are_refused_before_the_device(L):
    L, a = L(), Args()
    for k in NAMES:
        if isinstance(a.v[k], np.ndarray):
            assert a.each(L, **{k: None}) == BADARG and a.batch(L, **{k: None}) == BADARG, k
    assert a.each(L, status=False) == BADARG and a.batch(L, rho=None) == BADARG and a.batch(L, ok=False) == BADARG
    for sides in (0, 3, -1):
        assert a.each(L, sides=sides) == BADARG and a.batch(L, sides=sides) == BADARG
    assert a.each(L, l=65) == BADARG and a.batch(L, l=65) == BADARG
    assert a.each(L, n=2 ** 31) == BADARG and a.batch(L, n=2 ** 31) == BADARG
    # rho = 0 mod r, and a random_i that is: canonical zero, r itself, and in the Montgomery form zero
    for zero, mont in ((0, 0), (R, 0), (0, 1)):
        a.rho = limbs(zero)
        assert a.batch(L, mont=mont) == BADARG
        rnd = np.ones((N, 4), np.uint64); rnd[N - 1] = limbs(zero)
        assert a.each(L, random=p_(rnd), mont=mont) == BADARG
    assert (a.status == 9).all() and (a.detail == -9).all() and a.ok.value == -7


@pytest.mark.parametrize("L", [slib, sdev], ids=["smc", "smc-dev"])
def test_a_well_formed_call_stops_at_the_missing_device(L):
    L = L()
    if L.dgpu_context_count() != 0:                                         # (the suite's CPU half never initialises a device; with one these calls would run)
        pytest.skip("this library is up on a device in this process: DGPU_E_NODEVICE cannot be observed")
    for sides, l in ((1, 0), (2, 0), (1, 1), (2, 3), (1, 64), (2, 64)):
        a = Args(sides, l)
        assert a.each(L) == NODEVICE and a.each(L, detail=False) == NODEVICE and a.each(L, random=p_(a.random)) == NODEVICE and a.batch(L) == NODEVICE, (sides, l)
        assert a.each(L, mont=1) == NODEVICE and a.batch(L, mont=1) == NODEVICE
        if l == 0:                                                          # no digits: their arrays and the weights may be NULL
            assert a.each(L, w=None, dpts=None, dresp=None) == NODEVICE and a.batch(L, w=None, dpts=None, dresp=None) == NODEVICE
    assert (a.status == 9).all() and a.ok.value == -7
