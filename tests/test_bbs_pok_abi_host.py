"""CPU: the host-side contract of dgpu_bbs_plus_pok_verify_each_g1 and dgpu_bbs_plus_pok_verify_batch_g1 (include/dock_gpu.h) — what can be decided without a
device: the two symbols are exported by the product and its twin and declared in crypto_amd/_native.py, n = 0 is DGPU_OK with every pointer NULL and the empty
batch verifies, every DGPU_E_BADARG case of the header that needs no handle answers so before the device is looked at (rho = 0 as 0 and as r, L = 0, row_stride < L,
NULL pointers, sizes of 2^31), and a well-formed call is stopped by the missing device only.  crypto_amd.bbs_plus.challenge_contribution byte for byte against a
layout built here from the oracle's field conversion and the Zcash flags."""
import ctypes as C
import numpy as np
import pytest
import oracle_c as O
from crypto_amd import _native
from crypto_amd import bbs_plus as BBS
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R2 = pow(2, 256, R)
PREPARED_WORDS = 68 * 36
vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def test_symbols_exported_and_declared():
    want = {"dgpu_bbs_plus_pok_verify_each_g1": [u64, sz, vp, vp, vp, vp, vp, vp, sz, vp, vp, sz, i32, vp],
            "dgpu_bbs_plus_pok_verify_batch_g1": [u64, sz, vp, vp, vp, vp, vp, vp, sz, vp, vp, sz, i32, vp, C.POINTER(i32)]}
    for name, args in want.items():
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args


class Args:
    """well-formed calls: three proofs over two messages, a row stride of three"""
    def __init__(self, mont=False):
        self.f = (lambda vals: limbs([v * R2 % R for v in vals])) if mont else limbs
        self.mont = 1 if mont else 0
        self.rho = self.f([5])
        self.h0, self.points = np.ones(12, np.uint64), np.ones((3, 5, 12), np.uint64)
        self.fixed, self.values, self.chal = self.f(list(range(30, 42))), self.f(list(range(100, 109))), self.f([11, 12, 13])
        self.rev = np.array([1, 0, 0, 1, 1, 1], np.uint8)
        self.pk, self.g2 = np.ones(PREPARED_WORDS, np.uint64), np.ones(PREPARED_WORDS, np.uint64)
        self.status, self.ok1 = np.full(3, 9, np.uint8), C.c_int32(-7)

    def base(self, kw):
        a = dict(params=0, L=2, h0=p_(self.h0), pk=p_(self.pk), g2=p_(self.g2), points=p_(self.points), fixed=p_(self.fixed), values=p_(self.values), stride=3, rev=p_(self.rev),
                 chal=p_(self.chal), n=3, status=p_(self.status), rho=p_(self.rho), ok1=C.byref(self.ok1))
        a.update(kw)
        return a

    def each(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_bbs_plus_pok_verify_each_g1(a["params"], a["L"], a["h0"], a["pk"], a["g2"], a["points"], a["fixed"], a["values"], a["stride"], a["rev"], a["chal"], a["n"],
                                                   self.mont, a["status"])

    def batch(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_bbs_plus_pok_verify_batch_g1(a["params"], a["L"], a["h0"], a["pk"], a["g2"], a["points"], a["fixed"], a["values"], a["stride"], a["rev"], a["chal"], a["n"],
                                                    self.mont, a["rho"], a["ok1"])


def test_no_rows_need_no_device_and_read_nothing():
    L = lib()
    assert L.dgpu_bbs_plus_pok_verify_each_g1(0, 0, None, None, None, None, None, None, 0, None, None, 0, 0, None) == OK
    assert L.dgpu_bbs_plus_pok_verify_each_g1(12345, 1 << 40, None, None, None, None, None, None, 0, None, None, 0, 1, None) == OK
    assert L.dgpu_bbs_plus_pok_verify_batch_g1(0, 0, None, None, None, None, None, None, 0, None, None, 0, 0, None, None) == OK
    ok = C.c_int32(-7)
    assert L.dgpu_bbs_plus_pok_verify_batch_g1(0, 3, None, None, None, None, None, None, 0, None, None, 0, 1, None, C.byref(ok)) == OK and ok.value == 1      # the empty batch verifies


def test_a_well_formed_call_is_stopped_by_the_missing_device_only():
    L = lib()
    want = BADARG if L.dgpu_context_count() != 0 else NODEVICE      # (the suite's CPU half never initialises a device; with one, handle 0 is what stops these calls)
    for mont in (False, True):
        A = Args(mont)
        assert A.each(L) == want and A.batch(L) == want
        assert A.each(L, stride=2) == want and A.batch(L, stride=1 << 20) == want                    # packed rows; a long stride is only a stride
        assert (A.status == 9).all() and A.ok1.value == -7


def test_bad_arguments_answer_before_the_device():
    L = lib()
    A = Args()
    for kw in (dict(L=0), dict(stride=1), dict(h0=None), dict(pk=None), dict(g2=None), dict(points=None), dict(fixed=None), dict(values=None), dict(rev=None), dict(chal=None),
               dict(n=1 << 31), dict(stride=1 << 31), dict(L=(1 << 31) - 2, stride=1 << 31)):
        assert A.each(L, **kw) == BADARG, kw
        assert A.batch(L, **kw) == BADARG, kw
    assert A.each(L, status=None) == BADARG
    assert A.batch(L, ok1=None) == BADARG and A.batch(L, rho=None) == BADARG
    assert (A.status == 9).all() and A.ok1.value == -7


def test_a_zero_batching_scalar_is_refused_before_the_device():
    L = lib()
    A = Args()
    assert A.batch(L, rho=p_(limbs([0]))) == BADARG
    assert A.batch(L, rho=p_(limbs([R]))) == BADARG                                                 # canonical words are taken mod r
    assert A.batch(L, rho=p_(limbs([2 * R]))) == BADARG
    assert Args(True).batch(L, rho=p_(limbs([0]))) == BADARG
    assert A.ok1.value == -7


def test_the_python_wrappers_count_their_rows():
    class Q:
        handle, L, h_0, pk_pc, g2_pc = 0, 2, np.ones(12, np.uint64), np.ones(PREPARED_WORDS, np.uint64), np.ones(PREPARED_WORDS, np.uint64)
    with pytest.raises(ValueError):
        BBS._proofs(Q, np.ones((2, 5, 12), np.uint64), [[1, 2, 3, 4]] * 3, [[1, 2]] * 3, [[0, 1]] * 3, [5, 6, 7])
    with pytest.raises(ValueError):
        BBS._proofs(Q, np.ones((3, 5, 12), np.uint64), [[1, 2, 3, 4]] * 3, [[1, 2, 3]] * 3, [[0, 1]] * 3, [5, 6, 7])
    v, stride, n, pts, fixed, rev, c = BBS._proofs(Q, np.ones((3, 5, 12), np.uint64), [[1, 2, 3, 4]] * 3, [[1, 2]] * 3, [[0, 7]] * 3, [5, 6, 7])
    assert (stride, n) == (2, 3) and fixed.shape == (3, 4, 4) and rev.tolist() == [[0, 1]] * 3 and c.shape == (3, 4) and fixed[1, 2, 0] == 3


def compressed(pt):
    """ark-serialize's compressed G1 (Zcash flags) from affine Montgomery words, through the oracle's field conversion"""
    if not pt.any():
        return bytes([0xC0]) + bytes(47)
    x, y = [sum(int(w) << (64 * k) for k, w in enumerate(O.fp_from_mont(pt[6 * h:6 * h + 6]))) for h in (0, 1)]
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if y > (P - 1) // 2 else 0)
    return bytes(b)


def test_challenge_contribution_byte_for_byte():
    """A', Abar, d, h_0, g1, T1, T2, then every h_j followed by m_j where it is revealed (proof.rs:328-352)"""
    G = O.G1
    L = 4
    pts = G.gen_seq(O.rand_scalars(1, 1)[0], O.rand_scalars(2, 1)[0], L + 2 + 5, threads=1)
    params, proof = pts[:L + 2], pts[L + 2:].copy()
    proof[4] = 0                                                              # an identity T2 has a byte layout too
    vals = [3, R - 1, 0, 1 << 200]
    for mask in ([0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 0, 1], [0, 1, 1, 0]):
        want = b"".join(compressed(q) for q in (proof[0], proof[1], proof[2], params[1], params[0], proof[3], proof[4]))
        for j in range(L):
            want += compressed(params[2 + j]) + (vals[j].to_bytes(32, "little") if mask[j] else b"")
        got = BBS.challenge_contribution(params, proof, mask, vals)
        assert got == want and len(got) == 48 * (7 + L) + 32 * sum(mask), mask
    assert {compressed(q)[0] & 0x20 for q in pts} == {0, 0x20}                # both signs of y among the points
    with pytest.raises(ValueError):
        BBS.challenge_contribution(params, proof, [0, 0, 0], vals)
