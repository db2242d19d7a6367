"""CPU: the host-side contract of dgpu_accumulator_d_for_batch[_resident], dgpu_accumulator_non_membership_witnesses_g1 and
dgpu_accumulator_membership_witnesses_g1 (include/dock_gpu.h) — what can be decided without a device: the four symbols are exported by the product and
its twin and declared in crypto_amd/_native.py, m = 0 is DGPU_OK whatever the other arguments, every DGPU_E_BADARG case of the header — a y_i equal to
-alpha in the first and in the last position included — answers so before the device is looked at, and a well-formed call is stopped by the missing device
only."""
import ctypes as C
import numpy as np
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R2 = pow(2, 256, R)
vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def test_symbols_exported_and_declared():
    want = {"dgpu_accumulator_d_for_batch": [vp, sz, vp, sz, i32, vp, vp, vp],
            "dgpu_accumulator_d_for_batch_resident": [u64, sz, sz, vp, sz, i32, vp, vp, vp],
            "dgpu_accumulator_non_membership_witnesses_g1": [vp, vp, sz, vp, vp, vp, i32, vp, vp, vp],
            "dgpu_accumulator_membership_witnesses_g1": [vp, sz, vp, vp, i32, vp, vp]}
    for name, args in want.items():
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args
    for name in ("dgpu_dev_set_acc_d_pass", "dgpu_dev_set_acc_d_unroll", "dgpu_dev_get_acc_d_unroll"):      # the twin's knobs, and only the twin's
        assert name in _native.DEV_SYMBOLS and hasattr(dev_lib(), name) and not hasattr(lib(), name)


class Args:
    """well-formed calls: three members, four non-members"""
    def __init__(self, mont=False):
        f = (lambda vals: limbs([v * R2 % R for v in vals])) if mont else limbs
        self.mont = 1 if mont else 0
        self.alpha, self.fv = f([7]), f([99])
        self.members, self.ys, self.d_in = f([11, 12, 13]), f([21, 22, 23, 24]), f([1, 2, 3, 4])
        self.base = np.ones(12, np.uint64)
        self.d, self.nz = np.zeros((4, 4), np.uint64), np.zeros(4, np.uint8)
        self.out, self.inf, self.ok = np.zeros((4, 12), np.uint64), np.zeros(4, np.uint8), np.zeros(4, np.uint8)

    def d_call(self, L, **kw):
        a = dict(members=p_(self.members), n=3, ys=p_(self.ys), m=4, d_in=p_(self.d_in), d=p_(self.d), nz=p_(self.nz)); a.update(kw)
        return L.dgpu_accumulator_d_for_batch(a["members"], a["n"], a["ys"], a["m"], self.mont, a["d_in"], a["d"], a["nz"])

    def resident(self, L, **kw):
        a = dict(handle=0, offset=0, n=3, ys=p_(self.ys), m=4, d_in=p_(self.d_in), d=p_(self.d), nz=p_(self.nz)); a.update(kw)
        return L.dgpu_accumulator_d_for_batch_resident(a["handle"], a["offset"], a["n"], a["ys"], a["m"], self.mont, a["d_in"], a["d"], a["nz"])

    def non_membership(self, L, **kw):
        a = dict(d=p_(self.d_in), ys=p_(self.ys), m=4, fv=p_(self.fv), alpha=p_(self.alpha), base=p_(self.base), out=p_(self.out), inf=p_(self.inf), ok=p_(self.ok)); a.update(kw)
        return L.dgpu_accumulator_non_membership_witnesses_g1(a["d"], a["ys"], a["m"], a["fv"], a["alpha"], a["base"], self.mont, a["out"], a["inf"], a["ok"])

    def membership(self, L, **kw):
        a = dict(ys=p_(self.ys), m=4, alpha=p_(self.alpha), base=p_(self.base), out=p_(self.out), inf=p_(self.inf)); a.update(kw)
        return L.dgpu_accumulator_membership_witnesses_g1(a["ys"], a["m"], a["alpha"], a["base"], self.mont, a["out"], a["inf"])


def test_no_elements_need_no_device_and_read_nothing():
    L = lib()
    assert L.dgpu_accumulator_d_for_batch(None, 0, None, 0, 0, None, None, None) == OK
    assert L.dgpu_accumulator_d_for_batch(None, 1 << 40, None, 0, 1, None, None, None) == OK
    assert L.dgpu_accumulator_d_for_batch_resident(12345, 7, 1 << 40, None, 0, 0, None, None, None) == OK
    assert L.dgpu_accumulator_non_membership_witnesses_g1(None, None, 0, None, None, None, 0, None, None, None) == OK
    assert L.dgpu_accumulator_membership_witnesses_g1(None, 0, None, None, 1, None, None) == OK


def test_a_well_formed_call_is_stopped_by_the_missing_device_only():
    L = lib()
    want = (NODEVICE,) if L.dgpu_context_count() == 0 else (OK,)      # (the suite's CPU half never initialises a device)
    for mont in (False, True):
        A = Args(mont)
        assert A.d_call(L) in want and A.d_call(L, d_in=None) in want
        assert A.d_call(L, members=None, n=0) in want                                              # no members at all need no pointer
        assert A.non_membership(L) in want and A.membership(L) in want
        if want == (NODEVICE,):
            assert not A.d.any() and not A.out.any()


def test_d_for_batch_bad_arguments():
    L = lib()
    A = Args()
    for kw in (dict(members=None), dict(ys=None), dict(d=None), dict(nz=None)):
        assert A.d_call(L, **kw) == BADARG, kw
    assert A.d_call(L, m=1 << 31) == BADARG and A.d_call(L, n=1 << 31) == BADARG
    for kw in (dict(ys=None), dict(d=None), dict(nz=None), dict(m=1 << 31), dict(n=1 << 31)):
        assert A.resident(L, **kw) == BADARG, kw
    assert A.resident(L) == BADARG and A.resident(L, handle=987654321) == BADARG                      # no such handle
    assert A.resident(L, handle=987654321, n=0) == BADARG                                            # ... even for an empty range


def test_witness_calls_bad_arguments():
    L = lib()
    A = Args()
    for kw in (dict(d=None), dict(ys=None), dict(fv=None), dict(alpha=None), dict(base=None), dict(out=None), dict(inf=None), dict(ok=None), dict(m=1 << 31)):
        assert A.non_membership(L, **kw) == BADARG, kw
    for kw in (dict(ys=None), dict(alpha=None), dict(base=None), dict(out=None), dict(inf=None), dict(m=1 << 31)):
        assert A.membership(L, **kw) == BADARG, kw


def test_an_element_equal_to_minus_alpha_is_refused_before_the_device():
    L = lib()
    minus = R - 7
    for mont in (False, True):
        A = Args(mont)
        f = (lambda vals: limbs([v * R2 % R for v in vals])) if mont else limbs
        for bad in (f([minus, 22, 23, 24]), f([21, 22, 23, minus])):                                 # the first and the last position
            assert A.non_membership(L, ys=p_(bad)) == BADARG
            assert A.membership(L, ys=p_(bad)) == BADARG
    A = Args()
    assert A.membership(L, ys=p_(limbs([21, 22, 23, minus + R]))) == BADARG                          # canonical words are taken mod r
    # 5000 elements: several shares of the host threads, the offender in the last one
    ys = limbs(list(range(100, 5100)))
    ys[-1] = limbs([minus])[0]
    out, inf = np.zeros((5000, 12), np.uint64), np.zeros(5000, np.uint8)
    assert A.membership(L, ys=p_(ys), m=5000, out=p_(out), inf=p_(inf)) == BADARG
