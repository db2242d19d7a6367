"""CPU: the host-side contract of dgpu_bbs_plus_sign_many_g1, dgpu_bbs_plus_verify_each_g1 and dgpu_bbs_plus_verify_batch_g1 (include/dock_gpu.h) — what can be
decided without a device: the three symbols are exported by the product and its twin and declared in crypto_amd/_native.py, n = 0 is DGPU_OK with every pointer
NULL, every DGPU_E_BADARG case of the header that needs no handle answers so before the device is looked at (rho = 0 as 0 and as r, L = 0, row_stride < L, NULL
pointers, sizes of 2^31), and a well-formed call is stopped by the missing device only."""
import ctypes as C
import numpy as np
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R2 = pow(2, 256, R)
PREPARED_WORDS = 68 * 36
vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def test_symbols_exported_and_declared():
    want = {"dgpu_bbs_plus_sign_many_g1": [u64, sz, vp, vp, sz, vp, vp, sz, i32, vp, vp],
            "dgpu_bbs_plus_verify_each_g1": [u64, sz, vp, vp, vp, vp, vp, vp, sz, sz, i32, vp],
            "dgpu_bbs_plus_verify_batch_g1": [u64, sz, vp, vp, vp, vp, vp, vp, sz, sz, i32, vp, C.POINTER(i32)]}
    for name, args in want.items():
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args


class Args:
    """well-formed calls: three rows of two messages, a row stride of three"""
    def __init__(self, mont=False):
        self.f = (lambda vals: limbs([v * R2 % R for v in vals])) if mont else limbs
        self.mont = 1 if mont else 0
        self.sk, self.rho = self.f([7]), self.f([5])
        self.msgs, self.e, self.s = self.f(list(range(100, 109))), self.f([11, 12, 13]), self.f([21, 22, 23])
        self.pk, self.g2 = np.ones(PREPARED_WORDS, np.uint64), np.ones(PREPARED_WORDS, np.uint64)
        self.a = np.ones((3, 12), np.uint64)
        self.out, self.bad, self.ok, self.ok1 = np.zeros((3, 12), np.uint64), np.zeros(3, np.uint8), np.zeros(3, np.uint8), C.c_int32(-7)

    def base(self, kw):
        a = dict(params=0, L=2, sk=p_(self.sk), msgs=p_(self.msgs), stride=3, e=p_(self.e), s=p_(self.s), n=3, out=p_(self.out), bad=p_(self.bad), pk=p_(self.pk),
                 g2=p_(self.g2), a=p_(self.a), ok=p_(self.ok), rho=p_(self.rho), ok1=C.byref(self.ok1))
        a.update(kw)
        return a

    def sign(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_bbs_plus_sign_many_g1(a["params"], a["L"], a["sk"], a["msgs"], a["stride"], a["e"], a["s"], a["n"], self.mont, a["out"], a["bad"])

    def each(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_bbs_plus_verify_each_g1(a["params"], a["L"], a["pk"], a["g2"], a["a"], a["e"], a["s"], a["msgs"], a["stride"], a["n"], self.mont, a["ok"])

    def batch(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_bbs_plus_verify_batch_g1(a["params"], a["L"], a["pk"], a["g2"], a["a"], a["e"], a["s"], a["msgs"], a["stride"], a["n"], self.mont, a["rho"], a["ok1"])


def test_no_rows_need_no_device_and_read_nothing():
    L = lib()
    assert L.dgpu_bbs_plus_sign_many_g1(0, 0, None, None, 0, None, None, 0, 0, None, None) == OK
    assert L.dgpu_bbs_plus_sign_many_g1(12345, 1 << 40, None, None, 0, None, None, 0, 1, None, None) == OK
    assert L.dgpu_bbs_plus_verify_each_g1(0, 0, None, None, None, None, None, None, 0, 0, 0, None) == OK
    assert L.dgpu_bbs_plus_verify_batch_g1(0, 0, None, None, None, None, None, None, 0, 0, 0, None, None) == OK
    ok = C.c_int32(-7)
    assert L.dgpu_bbs_plus_verify_batch_g1(0, 3, None, None, None, None, None, None, 0, 0, 1, None, C.byref(ok)) == OK and ok.value == 1      # the empty batch verifies


def test_a_well_formed_call_is_stopped_by_the_missing_device_only():
    L = lib()
    if L.dgpu_context_count() != 0:      # (the suite's CPU half never initialises a device; with one, handle 0 is what stops these calls)
        want = BADARG
    else:
        want = NODEVICE
    for mont in (False, True):
        A = Args(mont)
        assert A.sign(L) == want and A.each(L) == want and A.batch(L) == want
        assert A.sign(L, stride=2) == want and A.each(L, stride=1 << 20) == want                    # packed rows; a long stride is only a stride
        assert A.sign(L, e=p_(A.f([R - 7, 12, 13]))) == want                                       # sk + e_0 = 0 is a flagged row, not a refusal
        assert not A.out.any() and not A.ok.any() and A.ok1.value == -7


def test_bad_arguments_answer_before_the_device():
    L = lib()
    A = Args()
    for kw in (dict(L=0), dict(stride=1), dict(msgs=None), dict(e=None), dict(s=None), dict(n=1 << 31), dict(stride=1 << 31), dict(L=(1 << 31) - 2, stride=1 << 31)):
        assert A.sign(L, **kw) == BADARG, kw
        assert A.each(L, **kw) == BADARG, kw
        assert A.batch(L, **kw) == BADARG, kw
    for kw in (dict(sk=None), dict(out=None), dict(bad=None)):
        assert A.sign(L, **kw) == BADARG, kw
    for kw in (dict(pk=None), dict(g2=None), dict(a=None)):
        assert A.each(L, **kw) == BADARG, kw
        assert A.batch(L, **kw) == BADARG, kw
    assert A.each(L, ok=None) == BADARG
    assert A.batch(L, ok1=None) == BADARG and A.batch(L, rho=None) == BADARG


def test_a_zero_batching_scalar_is_refused_before_the_device():
    L = lib()
    A = Args()
    assert A.batch(L, rho=p_(limbs([0]))) == BADARG
    assert A.batch(L, rho=p_(limbs([R]))) == BADARG                                                 # canonical words are taken mod r
    assert A.batch(L, rho=p_(limbs([2 * R]))) == BADARG
    assert Args(True).batch(L, rho=p_(limbs([0]))) == BADARG
    assert A.ok1.value == -7
