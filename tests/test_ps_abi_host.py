"""CPU: the host-side contract of the four dgpu_ps_* calls (include/dock_gpu.h) — what can be decided without a device: the symbols are exported by the product
and its twin and declared in crypto_amd/_native.py, n = 0 is DGPU_OK with every pointer NULL and the empty batch verifies, every DGPU_E_BADARG case of the header
that needs no handle answers so before the device is looked at (rho = 0 as 0 and as r, L = 0, row_stride < L, NULL pointers, sizes of 2^31), and a well-formed call
is stopped by the missing device only.  crypto_amd.ps.challenge_contribution byte for byte against a layout built here from the oracle's field conversion and the
Zcash flags."""
import ctypes as C
import numpy as np
import pytest
import oracle_c as O
from crypto_amd import _native
from crypto_amd import ps as PS
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R2 = pow(2, 256, R)
PREPARED_WORDS = 68 * 36
vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64
SIGNATURES = {"dgpu_ps_sign_many_g1": [u64, sz, vp, vp, sz, vp, sz, i32, vp, vp],
              "dgpu_ps_verify_each": [u64, sz, vp, vp, vp, sz, sz, i32, vp],
              "dgpu_ps_verify_batch": [u64, sz, vp, vp, vp, sz, sz, i32, vp, C.POINTER(i32)],
              "dgpu_ps_pok_verify_each": [u64, sz, vp, vp, vp, vp, vp, sz, vp, vp, sz, i32, vp]}


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def test_symbols_exported_and_declared():
    assert len(SIGNATURES) == 4
    for name, args in SIGNATURES.items():
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args, name
    assert len(_native.SYMBOLS) == 165


class Calls:
    """well-formed calls: three rows of two messages, a row stride of three"""
    def __init__(self, mont=False):
        self.f = (lambda vals: limbs([v * R2 % R for v in vals])) if mont else limbs
        self.mont = 1 if mont else 0
        self.sk, self.rho = self.f([77, 78, 79]), self.f([5])
        self.msgs, self.r, self.z, self.chal = self.f(list(range(100, 109))), self.f([11, 12, 13]), self.f([21, 22, 23]), self.f([31, 32, 33])
        self.sig, self.g2pts = np.ones((3, 2, 12), np.uint64), np.ones((3, 2, 24), np.uint64)
        self.rev = np.array([1, 0, 0, 1, 1, 1], np.uint8)
        self.pc, self.all_pc = np.ones(PREPARED_WORDS, np.uint64), np.ones(4 * PREPARED_WORDS, np.uint64)
        self.out, self.bad, self.ok, self.status, self.ok1 = np.full((3, 2, 12), 9, np.uint64), np.full(3, 9, np.uint8), np.full(3, 9, np.uint8), np.full(3, 9, np.uint8), C.c_int32(-7)

    def base(self, kw):
        a = dict(h=0, L=2, sk=p_(self.sk), pc=p_(self.pc), all_pc=p_(self.all_pc), sig=p_(self.sig), msgs=p_(self.msgs), stride=3, r=p_(self.r), n=3, out=p_(self.out),
                 bad=p_(self.bad), ok=p_(self.ok), rho=p_(self.rho), ok1=C.byref(self.ok1), g2pts=p_(self.g2pts), z=p_(self.z), rev=p_(self.rev), chal=p_(self.chal),
                 status=p_(self.status))
        a.update(kw)
        return a

    def sign(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_ps_sign_many_g1(a["h"], a["L"], a["sk"], a["msgs"], a["stride"], a["r"], a["n"], self.mont, a["out"], a["bad"])

    def each(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_ps_verify_each(a["h"], a["L"], a["pc"], a["sig"], a["msgs"], a["stride"], a["n"], self.mont, a["ok"])

    def batch(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_ps_verify_batch(a["h"], a["L"], a["all_pc"], a["sig"], a["msgs"], a["stride"], a["n"], self.mont, a["rho"], a["ok1"])

    def pok(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_ps_pok_verify_each(a["h"], a["L"], a["pc"], a["sig"], a["g2pts"], a["z"], a["msgs"], a["stride"], a["rev"], a["chal"], a["n"], self.mont, a["status"])

    def all(self, lb, **kw):
        return [self.sign(lb, **kw), self.each(lb, **kw), self.batch(lb, **kw), self.pok(lb, **kw)]

    def untouched(self):
        return (self.out == 9).all() and (self.bad == 9).all() and (self.ok == 9).all() and (self.status == 9).all() and self.ok1.value == -7


def test_no_rows_need_no_device_and_read_nothing():
    L = lib()
    assert L.dgpu_ps_sign_many_g1(0, 0, None, None, 0, None, 0, 0, None, None) == OK
    assert L.dgpu_ps_sign_many_g1(12345, 1 << 40, None, None, 0, None, 0, 1, None, None) == OK
    assert L.dgpu_ps_verify_each(0, 0, None, None, None, 0, 0, 0, None) == OK
    assert L.dgpu_ps_verify_each(12345, 1 << 40, None, None, None, 0, 0, 1, None) == OK
    assert L.dgpu_ps_verify_batch(0, 0, None, None, None, 0, 0, 0, None, None) == OK
    ok = C.c_int32(-7)
    assert L.dgpu_ps_verify_batch(0, 3, None, None, None, 0, 0, 1, None, C.byref(ok)) == OK and ok.value == 1          # the empty batch verifies
    assert L.dgpu_ps_pok_verify_each(0, 0, None, None, None, None, None, 0, None, None, 0, 0, None) == OK
    assert L.dgpu_ps_pok_verify_each(12345, 1 << 40, None, None, None, None, None, 0, None, None, 0, 1, None) == OK


def test_a_well_formed_call_is_stopped_by_the_missing_device_only():
    L = lib()
    want = BADARG if L.dgpu_context_count() != 0 else NODEVICE      # (the suite's CPU half never initialises a device; with one, handle 0 is what stops these calls)
    for mont in (False, True):
        A = Calls(mont)
        assert A.all(L) == [want] * 4
        assert A.all(L, stride=2) == [want] * 4 and A.all(L, stride=1 << 20) == [want] * 4      # packed rows; a long stride is only a stride
        assert A.untouched()


def test_bad_arguments_answer_before_the_device():
    L = lib()
    A = Calls()
    for kw in (dict(L=0), dict(stride=1), dict(msgs=None), dict(n=1 << 31), dict(stride=1 << 31), dict(L=(1 << 31) - 2, stride=1 << 31)):
        assert A.all(L, **kw) == [BADARG] * 4, kw
    for kw in (dict(sk=None), dict(r=None), dict(out=None), dict(bad=None)):
        assert A.sign(L, **kw) == BADARG, kw
    assert A.each(L, sig=None) == BADARG and A.batch(L, sig=None) == BADARG and A.pok(L, sig=None) == BADARG
    assert A.each(L, pc=None) == BADARG and A.pok(L, pc=None) == BADARG and A.batch(L, all_pc=None) == BADARG
    assert A.each(L, ok=None) == BADARG and A.batch(L, ok1=None) == BADARG and A.batch(L, rho=None) == BADARG
    for kw in (dict(g2pts=None), dict(z=None), dict(rev=None), dict(chal=None), dict(status=None)):
        assert A.pok(L, **kw) == BADARG, kw
    assert A.untouched()


def test_a_zero_batching_scalar_is_refused_before_the_device():
    L = lib()
    A, M = Calls(), Calls(True)
    assert A.batch(L, rho=p_(limbs([0]))) == BADARG
    assert A.batch(L, rho=p_(limbs([R]))) == BADARG                                             # canonical words are taken mod r
    assert A.batch(L, rho=p_(limbs([2 * R]))) == BADARG
    assert M.batch(L, rho=p_(limbs([0]))) == BADARG
    assert A.ok1.value == -7 and M.ok1.value == -7


def test_the_python_wrappers_count_their_rows():
    class Q:
        handle, L, g_tilde_pc, all_pc = 0, 2, np.ones(PREPARED_WORDS, np.uint64), np.ones(4 * PREPARED_WORDS, np.uint64)
    with pytest.raises(ValueError):
        PS._sigs(np.ones((2, 2, 12), np.uint64), 3)
    with pytest.raises(ValueError):
        PS._proofs(Q, np.ones((3, 2, 12), np.uint64), np.ones((2, 2, 24), np.uint64), [1, 2, 3], [[1, 2]] * 3, [[0, 1]] * 3, [5, 6, 7])
    with pytest.raises(ValueError):
        PS._proofs(Q, np.ones((3, 2, 12), np.uint64), np.ones((3, 2, 24), np.uint64), [1, 2, 3], [[1, 2, 3]] * 3, [[0, 1]] * 3, [5, 6, 7])
    with pytest.raises(ValueError):
        PS._proofs(Q, np.ones((3, 2, 12), np.uint64), np.ones((3, 2, 24), np.uint64), [1, 2], [[1, 2]] * 3, [[0, 1]] * 3, [5, 6, 7])
    v, stride, n, a, pts, z, rev, c = PS._proofs(Q, np.ones((3, 2, 12), np.uint64), np.ones((3, 2, 24), np.uint64), [1, 2, 3], [[1, 2]] * 3, [[0, 7]] * 3, [5, 6, 7])
    assert (stride, n) == (2, 3) and a.shape == (3, 2, 12) and pts.shape == (3, 2, 24) and rev.tolist() == [[0, 1]] * 3 and c.shape == (3, 4) and z[2, 0] == 3
    assert PS.STATUS[1] == "ZeroSignature" and PS.STATUS[4] == "PairingCheckFailed"


def coord(words):
    return sum(int(w) << (64 * k) for k, w in enumerate(O.fp_from_mont(words)))


def compressed_g1(pt):
    """ark-serialize's compressed G1 (Zcash flags) from affine Montgomery words, through the oracle's field conversion"""
    if not pt.any():
        return bytes([0xC0]) + bytes(47)
    x, y = coord(pt[:6]), coord(pt[6:])
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if y > (P - 1) // 2 else 0)
    return bytes(b)


def compressed_g2(pt):
    """compressed G2: x.c1 then x.c0, 48 big-endian bytes each; the sign flag compares y lexicographically, c1 first"""
    if not pt.any():
        return bytes([0xC0]) + bytes(95)
    x0, x1, y0, y1 = (coord(pt[6 * h:6 * h + 6]) for h in range(4))
    greatest = y1 > (P - 1) // 2 if y1 else y0 > (P - 1) // 2
    b = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if greatest else 0)
    return bytes(b)


def test_challenge_contribution_byte_for_byte():
    """beta_tilde as a compressed vector with its length prefix, g, k, t (proof.rs:59-72, with_schnorr_response.rs:106-113)"""
    L = 4
    g2s = O.G2.gen_seq(O.rand_scalars(1, 1)[0], O.rand_scalars(2, 1)[0], L + 2 + 8, threads=1)
    g = O.G1.gen_seq(O.rand_scalars(3, 1)[0], O.rand_scalars(4, 1)[0], 1, threads=1)[0]

    class Q:
        pass
    q = Q(); q.points, q.g, q.L = g2s[:L + 2], g, L
    signs = set()
    for i in range(4):
        k, t = g2s[L + 2 + 2 * i], g2s[L + 3 + 2 * i].copy()
        if i == 3:
            t[:] = 0                                                          # an identity commitment has a byte layout too
        want = (L).to_bytes(8, "little") + b"".join(compressed_g2(b) for b in g2s[1:L + 1]) + compressed_g1(g) + compressed_g2(k) + compressed_g2(t)
        got = PS.challenge_contribution(q, k, t)
        assert got == want and len(got) == 8 + 96 * L + 48 + 192, i
        signs |= {compressed_g2(k)[0] & 0x20, compressed_g2(t)[0] & 0x20}
    assert {compressed_g2(b)[0] & 0x20 for b in g2s} == {0, 0x20}             # both signs of y among the points
