"""CPU: the host-side contract of the four dgpu_accumulator_gt_* calls (include/dock_gpu_acc_gt.h, served by libdock_gpu_acc_gt.so and its development build,
NOT by the product or its other siblings) — what can be decided without a device: the header, crypto_amd/_native.py and the libraries' exports agree, the
product, its twin and the SAVER, SMC and BPP images export none of the names, n = 0 is DGPU_OK with every pointer NULL and the empty batch verifies, every
DGPU_E_BADARG case of the header answers so before the device is looked at (NULL pointers with n > 0, n = 2^31, a zero rho in either form), and a well-formed call
is stopped by the missing device only."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
glib = lambda: _native.acc_gt_lib(bring_up=False)                # libdock_gpu_acc_gt.so, not brought up on a device
gdev = lambda: _native._load(_native._ACC_GT_DEV_SO)             # its development build

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
PREPARED_WORDS = 68 * 36
vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
MEM, NM = "membership", "non_membership"
NAME = lambda kind, form: "dgpu_accumulator_gt_%s_proofs_verify_%s_g1" % (kind, form)
SIGNATURES = {NAME(MEM, "each"): [vp] * 8 + [sz, i32, vp], NAME(MEM, "batch"): [vp] * 8 + [sz, i32, vp, C.POINTER(i32)],
              NAME(NM, "each"): [vp] * 9 + [sz, i32, vp], NAME(NM, "batch"): [vp] * 9 + [sz, i32, vp, C.POINTER(i32)]}
N = 3


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(v):
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], np.uint64)


def test_symbols_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "dock_gpu_acc_gt.h")).read()
    assert sorted(set(re.findall(r"\b(dgpu_accumulator_gt_[a-z0-9_]+)\s*\(", hdr))) == sorted(SIGNATURES) == sorted(_native.ACC_GT_SYMBOLS)
    others = [lib(), dev_lib(), _native.saver_lib(bring_up=False), _native._load(_native._SAVER_DEV_SO), _native.smc_lib(bring_up=False), _native._load(_native._SMC_DEV_SO),
              _native.bpp_lib(bring_up=False), _native._load(_native._BPP_DEV_SO)]
    for name, args in SIGNATURES.items():
        assert name not in _native.SYMBOLS + _native.DEV_SYMBOLS + _native.SAVER_SYMBOLS + _native.SMC_SYMBOLS + _native.BPP_SYMBOLS
        for other in others:
            assert not hasattr(other, name)
        for L in (glib(), gdev()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args, name
    exported = lambda so: sorted(l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "crypto_amd", so)], text=True).splitlines() if " T dgpu_" in l)
    assert exported("libdock_gpu_acc_gt.so") == sorted(_native.SYMBOLS + _native.ACC_GT_SYMBOLS)
    assert exported("libdock_gpu_acc_gt_dev.so") == sorted(_native.SYMBOLS + _native.ACC_GT_SYMBOLS + _native.DEV_SYMBOLS)
    for so in ("libdock_gpu.so", "libdock_gpu_dev.so", "libdock_gpu_saver.so", "libdock_gpu_saver_dev.so", "libdock_gpu_smc.so", "libdock_gpu_smc_dev.so", "libdock_gpu_bpp.so",
               "libdock_gpu_bpp_dev.so"):
        assert not [s for s in exported(so) if "accumulator_gt" in s], so
    assert hasattr(gdev(), "dgpu_set_many_chunk_rows") and not hasattr(glib(), "dgpu_set_many_chunk_rows")      # the knob that cuts the chunks: the development build alone
    # the header states what the calls take on trust, the soundness bound and what rho = 1 does
    for phrase in ("dgpu_gt_in_subgroup_device", "dgpu_g1_validate_batch", "J n / r", "rho = 1 adds the rows up unweighted", "Nothing secret passes through"):
        assert phrase in hdr, phrase


class Args:
    """well-formed arguments of a kind (any words: nothing is computed without a device); head(): in the order of the header"""

    def __init__(self, kind, n=N):
        one = lambda *shape: np.ones(shape, np.uint64)
        npts, nresp = (7, 5) if kind == MEM else (11, 8)
        self.kind, self.n = kind, n
        self.v = dict(V=one(12), P=one(12), prk=one(3 if kind == MEM else 4, 12), pk=one(PREPARED_WORDS), pt=one(PREPARED_WORDS), points=one(n, npts, 12), r_e=one(n, 72),
                      resp=one(n, nresp, 4), c=one(n, 4))
        self.names = ["V"] + (["P"] if kind == NM else []) + ["prk", "pk", "pt", "points", "r_e", "resp", "c"]
        self.rho, self.status, self.ok = limbs(5), np.full(n, 9, np.uint8), C.c_int32(-7)

    def head(self, n=None, mont=0, **kw):
        v = dict(self.v, **kw)
        return [None if v[k] is None else p_(v[k]) for k in self.names] + [self.n if n is None else n, mont]

    def each(self, L, status=True, **kw):
        return getattr(L, NAME(self.kind, "each"))(*self.head(**kw), p_(self.status) if status else None)

    def batch(self, L, rho=True, ok=True, **kw):
        return getattr(L, NAME(self.kind, "batch"))(*self.head(**kw), (p_(self.rho) if rho is True else rho), C.byref(self.ok) if ok else None)


@pytest.mark.parametrize("kind", [MEM, NM])
@pytest.mark.parametrize("L", [glib, gdev], ids=["acc-gt", "acc-gt-dev"])
def test_n_zero_needs_nothing(L, kind):
    L = L()
    ok = C.c_int32(-7)
    nulls = [None] * (8 if kind == MEM else 9) + [0, 0]
    assert getattr(L, NAME(kind, "each"))(*nulls, None) == OK
    assert getattr(L, NAME(kind, "batch"))(*nulls, None, C.byref(ok)) == OK and ok.value == 1      # an empty batch verifies
    assert getattr(L, NAME(kind, "batch"))(*nulls, None, None) == OK


@pytest.mark.parametrize("kind", [MEM, NM])
@pytest.mark.parametrize("L", [glib, gdev], ids=["acc-gt", "acc-gt-dev"])
def test_bad_arguments_are_refused_before_the_device(L, kind):
    L, a = L(), Args(kind)
    for k in a.names:
        assert a.each(L, **{k: None}) == BADARG and a.batch(L, **{k: None}) == BADARG, k
    assert a.each(L, status=False) == BADARG and a.batch(L, rho=None) == BADARG and a.batch(L, ok=False) == BADARG
    assert a.each(L, n=2 ** 31) == BADARG and a.batch(L, n=2 ** 31) == BADARG
    # rho = 0 mod r: canonical zero, r itself, and in the Montgomery form zero
    for zero, mont in ((0, 0), (R, 0), (0, 1)):
        a.rho = limbs(zero)
        assert a.batch(L, mont=mont) == BADARG
    assert (a.status == 9).all() and a.ok.value == -7


@pytest.mark.parametrize("kind", [MEM, NM])
@pytest.mark.parametrize("L", [glib, gdev], ids=["acc-gt", "acc-gt-dev"])
def test_a_well_formed_call_stops_at_the_missing_device(L, kind):
    L = L()
    if L.dgpu_context_count() != 0:          # (the suite's CPU half never initialises a device; where this image is up on one, the refusal cannot be observed)
        return
    for n in (1, N, 4097):
        a = Args(kind, n)
        assert a.each(L) == NODEVICE and a.batch(L) == NODEVICE and a.each(L, mont=1) == NODEVICE and a.batch(L, mont=1) == NODEVICE, n
        assert (a.status == 9).all() and a.ok.value == -7
