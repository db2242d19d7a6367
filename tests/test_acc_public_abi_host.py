"""CPU: the host-side contract of dgpu_accumulator_omega_g1 / dgpu_accumulator_update_witnesses_public_g1 (include/dock_gpu.h) — what can be decided
without a device: both symbols are exported by the product and its twin and declared in crypto_amd/_native.py, m = 0 is DGPU_OK whatever the pointers,
two empty lists give DGPU_OK and omega_len = 0 without a device, and every DGPU_E_BADARG case of the header answers so before the device is looked at —
a list above the cap and an entry equal to -alpha included."""
import ctypes as C
import os
import numpy as np
import pytest
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R2 = pow(2, 256, R)
CAP = 1 << 18                                  # DGPU_ACC_OMEGA_MAX
vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def test_symbols_exported_and_declared():
    want = {"dgpu_accumulator_omega_g1": [vp, sz, vp, sz, vp, vp, i32, vp, vp, C.POINTER(sz)],
            "dgpu_accumulator_update_witnesses_public_g1": [vp, sz, vp, sz, vp, vp, sz, vp, vp, sz, i32, vp, vp, vp, vp]}
    for name, args in want.items():
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dock_gpu.h")).read()
    assert "#define DGPU_ACC_OMEGA_MAX ((size_t)1 << 18)" in hdr                                # the cap is stated in the header


class Args:
    """a well-formed pair of calls: two additions, one removal, an omega of two entries, three holders"""
    def __init__(self):
        self.alpha = limbs([7])
        self.adds, self.rems, self.elems = limbs([11, 12]), limbs([13]), limbs([21, 22, 23])
        self.wit, self.acc = np.ones((3, 12), np.uint64), np.ones(12, np.uint64)
        self.om, self.om_inf, self.length = np.zeros((2, 12), np.uint64), np.zeros(2, np.uint8), sz(99)
        self.d, self.out, self.inf, self.ok = np.zeros((3, 4), np.uint64), np.zeros((3, 12), np.uint64), np.zeros(3, np.uint8), np.zeros(3, np.uint8)

    def omega(self, L, mont=0, **kw):
        a = dict(adds=p_(self.adds), na=2, rems=p_(self.rems), nr=1, alpha=p_(self.alpha), acc=p_(self.acc), om=p_(self.om), om_inf=p_(self.om_inf), length=C.byref(self.length)); a.update(kw)
        return L.dgpu_accumulator_omega_g1(a["adds"], a["na"], a["rems"], a["nr"], a["alpha"], a["acc"], mont, a["om"], a["om_inf"], a["length"])

    def public(self, L, mont=0, **kw):
        a = dict(adds=p_(self.adds), na=2, rems=p_(self.rems), nr=1, om=p_(self.om), om_inf=p_(self.om_inf), n=2, elems=p_(self.elems), wit=p_(self.wit), m=3, d=p_(self.d),
                 out=p_(self.out), inf=p_(self.inf), ok=p_(self.ok)); a.update(kw)
        return L.dgpu_accumulator_update_witnesses_public_g1(a["adds"], a["na"], a["rems"], a["nr"], a["om"], a["om_inf"], a["n"], a["elems"], a["wit"], a["m"], mont,
                                                             a["d"], a["out"], a["inf"], a["ok"])


def test_no_holders_and_no_lists_need_no_device():
    L = lib()
    assert L.dgpu_accumulator_update_witnesses_public_g1(None, 0, None, 0, None, None, 0, None, None, 0, 0, None, None, None, None) == OK
    assert L.dgpu_accumulator_update_witnesses_public_g1(None, 3, None, 1 << 40, None, None, 9, None, None, 0, 1, None, None, None, None) == OK
    A = Args()
    for mont in (0, 1):
        A.length.value = 99
        assert A.omega(L, mont, adds=None, na=0, rems=None, nr=0, om=None, om_inf=None) == OK      # two empty lists: the empty Omega
        assert A.length.value == 0


def test_a_well_formed_call_is_stopped_by_the_missing_device_only():
    L = lib()
    want = (NODEVICE,) if L.dgpu_context_count() == 0 else (OK,)      # (the suite's CPU half never initialises a device)
    A = Args()
    assert A.omega(L) in want and A.public(L) in want
    assert A.omega(L, adds=None, na=0) in want and A.public(L, rems=None, nr=0) in want          # an empty list needs no pointer
    assert A.public(L, om=None, om_inf=None, n=0) in want and A.public(L, om_inf=None) in want   # no omega at all; no flag array
    if want == (NODEVICE,):
        assert not A.om.any() and not A.out.any()


def test_omega_bad_arguments():
    L = lib()
    A = Args()
    for kw in (dict(adds=None), dict(rems=None), dict(alpha=None), dict(acc=None), dict(om=None), dict(om_inf=None), dict(length=None)):
        assert A.omega(L, **kw) == BADARG, kw
    assert A.omega(L, na=1 << 31) == BADARG and A.omega(L, nr=1 << 31) == BADARG
    assert A.omega(L, na=CAP + 1) == BADARG and A.omega(L, nr=CAP + 1) == BADARG                 # above the cap (decided before the lists are read)
    minus = R - 7
    for bad in (limbs([11, minus]), limbs([minus + R, 12])):
        assert A.omega(L, adds=p_(bad)) == BADARG
    assert A.omega(L, rems=p_(limbs([minus]))) == BADARG
    mont = lambda vals: limbs([v * R2 % R for v in vals])
    M = Args()
    M.alpha, M.adds, M.rems = mont([7]), mont([11, minus]), mont([13])
    assert M.omega(L, mont=1) == BADARG
    M.adds, M.rems = mont([11, 12]), mont([minus])
    assert M.omega(L, mont=1) == BADARG


def test_public_update_bad_arguments():
    L = lib()
    A = Args()
    for kw in (dict(adds=None), dict(rems=None), dict(om=None), dict(elems=None), dict(wit=None), dict(d=None), dict(out=None), dict(inf=None), dict(ok=None)):
        assert A.public(L, **kw) == BADARG, kw
    assert A.public(L, m=1 << 31) == BADARG and A.public(L, n=1 << 31) == BADARG
    assert A.public(L, na=1 << 31) == BADARG and A.public(L, nr=1 << 31) == BADARG
    assert A.public(L, na=1 << 30, nr=1 << 30) == BADARG
