"""CPU: the host-side contract of dgpu_accumulator_update_factors / dgpu_accumulator_update_witnesses_g1 (include/dock_gpu.h) — what can be decided
without a device: both symbols are exported by the product and its twin and declared in crypto_amd/_native.py, the development knob is on the twin
only, m = 0 is DGPU_OK whatever the pointers, and every DGPU_E_BADARG case of the header answers so before the device is looked at — an addition or
a removal equal to -alpha included, which the host finds while it builds its tables."""
import ctypes as C
import numpy as np
import pytest
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R2 = pow(2, 256, R)
vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def test_symbols_exported_and_declared():
    want = {"dgpu_accumulator_update_factors": [vp, sz, vp, sz, vp, vp, sz, i32, vp, vp],
            "dgpu_accumulator_update_witnesses_g1": [vp, sz, vp, sz, vp, vp, vp, sz, vp, i32, vp, vp, vp]}
    for name, args in want.items():
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args
    for knob in ("dgpu_dev_set_acc_split", "dgpu_dev_get_acc_split"):
        assert knob in _native.DEV_SYMBOLS and hasattr(dev_lib(), knob)
        with pytest.raises(AttributeError):
            getattr(lib(), knob)                                 # not part of the product
    T = dev_lib()
    assert T.dgpu_dev_set_acc_split(-1) == BADARG and T.dgpu_dev_set_acc_split(4097) == BADARG
    assert T.dgpu_dev_set_acc_split(5) == OK and T.dgpu_dev_set_acc_split(0) == OK


class Args:
    """a well-formed call of two additions, one removal and three holders"""
    def __init__(self):
        self.alpha = limbs([7])
        self.adds, self.rems, self.elems = limbs([11, 12]), limbs([13]), limbs([21, 22, 23])
        self.wit, self.acc = np.ones((3, 12), np.uint64), np.ones(12, np.uint64)
        self.f, self.g = np.zeros((3, 4), np.uint64), np.zeros((3, 4), np.uint64)
        self.out, self.inf = np.zeros((3, 12), np.uint64), np.zeros(3, np.uint8)

    def factors(self, L, mont=0, **kw):
        a = dict(adds=p_(self.adds), na=2, rems=p_(self.rems), nr=1, alpha=p_(self.alpha), elems=p_(self.elems), m=3, f=p_(self.f), g=p_(self.g)); a.update(kw)
        return L.dgpu_accumulator_update_factors(a["adds"], a["na"], a["rems"], a["nr"], a["alpha"], a["elems"], a["m"], mont, a["f"], a["g"])

    def witnesses(self, L, mont=0, **kw):
        a = dict(adds=p_(self.adds), na=2, rems=p_(self.rems), nr=1, alpha=p_(self.alpha), elems=p_(self.elems), wit=p_(self.wit), m=3, acc=p_(self.acc), d=p_(self.f),
                 out=p_(self.out), inf=p_(self.inf)); a.update(kw)
        return L.dgpu_accumulator_update_witnesses_g1(a["adds"], a["na"], a["rems"], a["nr"], a["alpha"], a["elems"], a["wit"], a["m"], a["acc"], mont, a["d"], a["out"], a["inf"])


def test_an_empty_batch_is_ok_whatever_the_pointers():
    L = lib()
    assert L.dgpu_accumulator_update_factors(None, 0, None, 0, None, None, 0, 0, None, None) == OK
    assert L.dgpu_accumulator_update_factors(None, 5, None, 1 << 40, None, None, 0, 1, None, None) == OK
    assert L.dgpu_accumulator_update_witnesses_g1(None, 0, None, 0, None, None, None, 0, None, 0, None, None, None) == OK
    assert L.dgpu_accumulator_update_witnesses_g1(None, 3, None, 9, None, None, None, 0, None, 1, None, None, None) == OK


def test_a_well_formed_call_is_stopped_by_the_missing_device_only():
    L = lib()
    want = (NODEVICE,) if L.dgpu_context_count() == 0 else (OK,)      # (the suite's CPU half never initialises a device)
    A = Args()
    assert A.factors(L) in want and A.witnesses(L) in want
    assert A.factors(L, adds=None, na=0) in want and A.witnesses(L, rems=None, nr=0) in want      # an empty list needs no pointer
    if want == (NODEVICE,):
        assert not A.f.any() and not A.out.any()


@pytest.mark.parametrize("which", ["factors", "witnesses"])
def test_bad_arguments(which):
    L = lib()
    A = Args()
    call = getattr(A, which)
    # NULL pointers with a non-zero count
    for kw in (dict(adds=None), dict(rems=None), dict(alpha=None), dict(elems=None)):
        assert call(L, **kw) == BADARG, kw
    outs = (dict(f=None), dict(g=None)) if which == "factors" else (dict(wit=None), dict(acc=None), dict(d=None), dict(out=None), dict(inf=None))
    for kw in outs:
        assert call(L, **kw) == BADARG, kw
    # sizes
    assert call(L, m=1 << 31) == BADARG
    assert call(L, na=1 << 31) == BADARG and call(L, nr=1 << 31) == BADARG
    assert call(L, na=1 << 30, nr=1 << 30) == BADARG
    # an addition / a removal equal to -alpha, canonical (also given as a value >= r) and Montgomery words: found on the host
    minus = R - 7
    for bad in (limbs([11, minus]), limbs([minus + R, 12])):
        assert call(L, adds=p_(bad)) == BADARG
    assert call(L, rems=p_(limbs([minus]))) == BADARG
    mont = lambda vals: limbs([v * R2 % R for v in vals])
    M = Args()
    M.alpha, M.adds, M.rems, M.elems = mont([7]), mont([11, minus]), mont([13]), mont([21, 22, 23])
    assert getattr(M, which)(L, mont=1) == BADARG
    M.adds, M.rems = mont([11, 12]), mont([minus])
    assert getattr(M, which)(L, mont=1) == BADARG
