"""CPU: the host-side contract of the seven dgpu_bbs23_* calls (include/dock_gpu.h) — what can be decided without a device: the symbols are exported by the
product and its twin and declared in crypto_amd/_native.py, n = 0 is DGPU_OK with every pointer NULL and the empty batch verifies, every DGPU_E_BADARG case of the
header that needs no handle answers so before the device is looked at (rho = 0 as 0 and as r, L = 0, row_stride < L, NULL pointers, sizes of 2^31), and a
well-formed call is stopped by the missing device only.  Both challenge contributions of crypto_amd.bbs_23 byte for byte against a layout built here from the
oracle's field conversion and the Zcash flags."""
import ctypes as C
import numpy as np
import pytest
import oracle_c as O
from crypto_amd import _native
from crypto_amd import bbs_23 as B23
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R2 = pow(2, 256, R)
PREPARED_WORDS = 68 * 36
vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64
POK_EACH = [u64, sz, vp, vp, vp, vp, vp, sz, vp, vp, sz, i32, vp]
POK_BATCH = POK_EACH + [C.POINTER(i32)]
SIGNATURES = {"dgpu_bbs23_sign_many_g1": [u64, sz, vp, vp, sz, vp, sz, i32, vp, vp],
              "dgpu_bbs23_verify_each_g1": [u64, sz, vp, vp, vp, vp, vp, sz, sz, i32, vp],
              "dgpu_bbs23_verify_batch_g1": [u64, sz, vp, vp, vp, vp, vp, sz, sz, i32, vp, C.POINTER(i32)],
              "dgpu_bbs23_pok_verify_each_g1": POK_EACH, "dgpu_bbs23_pok_verify_batch_g1": POK_BATCH,
              "dgpu_bbs23_pok_ietf_verify_each_g1": POK_EACH, "dgpu_bbs23_pok_ietf_verify_batch_g1": POK_BATCH}
KINDS = {"cdl": ("dgpu_bbs23_pok_verify_each_g1", "dgpu_bbs23_pok_verify_batch_g1", 5, 3),
         "ietf": ("dgpu_bbs23_pok_ietf_verify_each_g1", "dgpu_bbs23_pok_ietf_verify_batch_g1", 3, 2)}


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def test_symbols_exported_and_declared():
    assert len(SIGNATURES) == 7
    for name, args in SIGNATURES.items():
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args, name


class Rows:
    """well-formed signature calls: three rows of two messages, a row stride of three"""
    def __init__(self, mont=False):
        self.f = (lambda vals: limbs([v * R2 % R for v in vals])) if mont else limbs
        self.mont = 1 if mont else 0
        self.sk, self.rho = self.f([77]), self.f([5])
        self.msgs, self.e = self.f(list(range(100, 109))), self.f([11, 12, 13])
        self.sig = np.ones((3, 12), np.uint64)
        self.pk, self.g2 = np.ones(PREPARED_WORDS, np.uint64), np.ones(PREPARED_WORDS, np.uint64)
        self.out, self.bad, self.ok, self.ok1 = np.full((3, 12), 9, np.uint64), np.full(3, 9, np.uint8), np.full(3, 9, np.uint8), C.c_int32(-7)

    def base(self, kw):
        a = dict(params=0, L=2, sk=p_(self.sk), pk=p_(self.pk), g2=p_(self.g2), sig=p_(self.sig), msgs=p_(self.msgs), stride=3, e=p_(self.e), n=3, out=p_(self.out), bad=p_(self.bad),
                 ok=p_(self.ok), rho=p_(self.rho), ok1=C.byref(self.ok1))
        a.update(kw)
        return a

    def sign(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_bbs23_sign_many_g1(a["params"], a["L"], a["sk"], a["msgs"], a["stride"], a["e"], a["n"], self.mont, a["out"], a["bad"])

    def each(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_bbs23_verify_each_g1(a["params"], a["L"], a["pk"], a["g2"], a["sig"], a["e"], a["msgs"], a["stride"], a["n"], self.mont, a["ok"])

    def batch(self, lb, **kw):
        a = self.base(kw)
        return lb.dgpu_bbs23_verify_batch_g1(a["params"], a["L"], a["pk"], a["g2"], a["sig"], a["e"], a["msgs"], a["stride"], a["n"], self.mont, a["rho"], a["ok1"])

    def untouched(self):
        return (self.out == 9).all() and (self.bad == 9).all() and (self.ok == 9).all() and self.ok1.value == -7


class Proofs:
    """well-formed proof calls of one kind: three proofs over two messages, a row stride of three"""
    def __init__(self, kind, mont=False):
        self.name_each, self.name_batch, npts, nresp = KINDS[kind]
        self.f = (lambda vals: limbs([v * R2 % R for v in vals])) if mont else limbs
        self.mont = 1 if mont else 0
        self.rho = self.f([5])
        self.points = np.ones((3, npts, 12), np.uint64)
        self.fixed, self.values, self.chal = self.f(list(range(30, 30 + 3 * nresp))), self.f(list(range(100, 109))), self.f([11, 12, 13])
        self.rev = np.array([1, 0, 0, 1, 1, 1], np.uint8)
        self.pk, self.g2 = np.ones(PREPARED_WORDS, np.uint64), np.ones(PREPARED_WORDS, np.uint64)
        self.status, self.ok1 = np.full(3, 9, np.uint8), C.c_int32(-7)

    def base(self, kw):
        a = dict(params=0, L=2, pk=p_(self.pk), g2=p_(self.g2), points=p_(self.points), fixed=p_(self.fixed), values=p_(self.values), stride=3, rev=p_(self.rev),
                 chal=p_(self.chal), n=3, status=p_(self.status), rho=p_(self.rho), ok1=C.byref(self.ok1))
        a.update(kw)
        return a

    def each(self, lb, **kw):
        a = self.base(kw)
        return getattr(lb, self.name_each)(a["params"], a["L"], a["pk"], a["g2"], a["points"], a["fixed"], a["values"], a["stride"], a["rev"], a["chal"], a["n"], self.mont, a["status"])

    def batch(self, lb, **kw):
        a = self.base(kw)
        return getattr(lb, self.name_batch)(a["params"], a["L"], a["pk"], a["g2"], a["points"], a["fixed"], a["values"], a["stride"], a["rev"], a["chal"], a["n"], self.mont, a["rho"],
                                            a["ok1"])

    def untouched(self):
        return (self.status == 9).all() and self.ok1.value == -7


def test_no_rows_need_no_device_and_read_nothing():
    L = lib()
    assert L.dgpu_bbs23_sign_many_g1(0, 0, None, None, 0, None, 0, 0, None, None) == OK
    assert L.dgpu_bbs23_sign_many_g1(12345, 1 << 40, None, None, 0, None, 0, 1, None, None) == OK
    assert L.dgpu_bbs23_verify_each_g1(0, 0, None, None, None, None, None, 0, 0, 0, None) == OK
    ok = C.c_int32(-7)
    assert L.dgpu_bbs23_verify_batch_g1(0, 0, None, None, None, None, None, 0, 0, 0, None, None) == OK
    assert L.dgpu_bbs23_verify_batch_g1(0, 3, None, None, None, None, None, 0, 0, 1, None, C.byref(ok)) == OK and ok.value == 1          # the empty batch verifies
    for name_each, name_batch, _, _ in KINDS.values():
        assert getattr(L, name_each)(0, 0, None, None, None, None, None, 0, None, None, 0, 0, None) == OK
        assert getattr(L, name_each)(12345, 1 << 40, None, None, None, None, None, 0, None, None, 0, 1, None) == OK
        assert getattr(L, name_batch)(0, 0, None, None, None, None, None, 0, None, None, 0, 0, None, None) == OK
        ok = C.c_int32(-7)
        assert getattr(L, name_batch)(0, 3, None, None, None, None, None, 0, None, None, 0, 1, None, C.byref(ok)) == OK and ok.value == 1


def test_a_well_formed_call_is_stopped_by_the_missing_device_only():
    L = lib()
    want = BADARG if L.dgpu_context_count() != 0 else NODEVICE      # (the suite's CPU half never initialises a device; with one, handle 0 is what stops these calls)
    for mont in (False, True):
        A = Rows(mont)
        assert A.sign(L) == want and A.each(L) == want and A.batch(L) == want
        assert A.sign(L, stride=2) == want and A.each(L, stride=2) == want and A.batch(L, stride=1 << 20) == want      # packed rows; a long stride is only a stride
        assert A.untouched()
        for kind in KINDS:
            A = Proofs(kind, mont)
            assert A.each(L) == want and A.batch(L) == want
            assert A.each(L, stride=2) == want and A.batch(L, stride=1 << 20) == want
            assert A.untouched()


def test_bad_arguments_answer_before_the_device():
    L = lib()
    A = Rows()
    for kw in (dict(L=0), dict(stride=1), dict(msgs=None), dict(e=None), dict(n=1 << 31), dict(stride=1 << 31), dict(L=(1 << 31) - 2, stride=1 << 31)):
        assert A.sign(L, **kw) == BADARG and A.each(L, **kw) == BADARG and A.batch(L, **kw) == BADARG, kw
    for kw in (dict(sk=None), dict(out=None), dict(bad=None)):
        assert A.sign(L, **kw) == BADARG, kw
    for kw in (dict(pk=None), dict(g2=None), dict(sig=None)):
        assert A.each(L, **kw) == BADARG and A.batch(L, **kw) == BADARG, kw
    assert A.each(L, ok=None) == BADARG and A.batch(L, ok1=None) == BADARG and A.batch(L, rho=None) == BADARG
    assert A.untouched()
    for kind in KINDS:
        A = Proofs(kind)
        for kw in (dict(L=0), dict(stride=1), dict(pk=None), dict(g2=None), dict(points=None), dict(fixed=None), dict(values=None), dict(rev=None), dict(chal=None),
                   dict(n=1 << 31), dict(stride=1 << 31), dict(L=(1 << 31) - 2, stride=1 << 31)):
            assert A.each(L, **kw) == BADARG, (kind, kw)
            assert A.batch(L, **kw) == BADARG, (kind, kw)
        assert A.each(L, status=None) == BADARG
        assert A.batch(L, ok1=None) == BADARG and A.batch(L, rho=None) == BADARG
        assert A.untouched()


def test_a_zero_batching_scalar_is_refused_before_the_device():
    L = lib()
    for A, M in [(Rows(), Rows(True))] + [(Proofs(kind), Proofs(kind, True)) for kind in KINDS]:
        assert A.batch(L, rho=p_(limbs([0]))) == BADARG
        assert A.batch(L, rho=p_(limbs([R]))) == BADARG                                             # canonical words are taken mod r
        assert A.batch(L, rho=p_(limbs([2 * R]))) == BADARG
        assert M.batch(L, rho=p_(limbs([0]))) == BADARG
        assert A.ok1.value == -7 and M.ok1.value == -7


def test_the_python_wrappers_count_their_rows():
    class Q:
        handle, L, pk_pc, g2_pc = 0, 2, np.ones(PREPARED_WORDS, np.uint64), np.ones(PREPARED_WORDS, np.uint64)
    with pytest.raises(ValueError):
        B23._rows(Q, [1, 2], [[1, 2]] * 3)
    with pytest.raises(ValueError):
        B23._rows(Q, [1, 2, 3], [[1, 2, 3]] * 3)
    for npts, nresp in ((5, 3), (3, 2)):
        fixed_rows = [list(range(1, nresp + 1))] * 3
        with pytest.raises(ValueError):
            B23._proofs(Q, npts, nresp, np.ones((2, npts, 12), np.uint64), fixed_rows, [[1, 2]] * 3, [[0, 1]] * 3, [5, 6, 7])
        with pytest.raises(ValueError):
            B23._proofs(Q, npts, nresp, np.ones((3, npts, 12), np.uint64), fixed_rows, [[1, 2, 3]] * 3, [[0, 1]] * 3, [5, 6, 7])
        v, stride, n, pts, fixed, rev, c = B23._proofs(Q, npts, nresp, np.ones((3, npts, 12), np.uint64), fixed_rows, [[1, 2]] * 3, [[0, 7]] * 3, [5, 6, 7])
        assert (stride, n) == (2, 3) and fixed.shape == (3, nresp, 4) and rev.tolist() == [[0, 1]] * 3 and c.shape == (3, 4) and fixed[1, nresp - 1, 0] == nresp
    assert B23.STATUS[3] == "SecondSchnorrVerificationFailed" and B23.STATUS[1] == "ZeroSignature"


def compressed(pt):
    """ark-serialize's compressed G1 (Zcash flags) from affine Montgomery words, through the oracle's field conversion"""
    if not pt.any():
        return bytes([0xC0]) + bytes(47)
    x, y = [sum(int(w) << (64 * k) for k, w in enumerate(O.fp_from_mont(pt[6 * h:6 * h + 6]))) for h in (0, 1)]
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if y > (P - 1) // 2 else 0)
    return bytes(b)


def test_challenge_contributions_byte_for_byte():
    """CDL: Abar, Bbar, d, g1, T1, T2 (proof_23_cdl.rs:272-296); IETF: Abar, Bbar, g1, T (proof_23_ietf.rs:218-238); then every h_j followed by m_j where it is
    revealed"""
    G = O.G1
    L = 4
    pts = G.gen_seq(O.rand_scalars(1, 1)[0], O.rand_scalars(2, 1)[0], L + 1 + 5, threads=1)
    params, proof = pts[:L + 1], pts[L + 1:].copy()
    proof[4] = 0                                                              # an identity T2 has a byte layout too
    vals = [3, R - 1, 0, 1 << 200]
    for mask in ([0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 0, 1], [0, 1, 1, 0]):
        tail = b""
        for j in range(L):
            tail += compressed(params[1 + j]) + (vals[j].to_bytes(32, "little") if mask[j] else b"")
        want = b"".join(compressed(q) for q in (proof[0], proof[1], proof[2], params[0], proof[3], proof[4])) + tail
        got = B23.challenge_contribution(params, proof, mask, vals)
        assert got == want and len(got) == 48 * (6 + L) + 32 * sum(mask), mask
        want = b"".join(compressed(q) for q in (proof[0], proof[1], params[0], proof[2])) + tail
        got = B23.challenge_contribution_ietf(params, proof[:3], mask, vals)
        assert got == want and len(got) == 48 * (4 + L) + 32 * sum(mask), mask
    assert {compressed(q)[0] & 0x20 for q in pts} == {0, 0x20}                # both signs of y among the points
    with pytest.raises(ValueError):
        B23.challenge_contribution(params, proof, [0, 0, 0], vals)
    with pytest.raises(ValueError):
        B23.challenge_contribution_ietf(params, proof[:3], [0, 0, 0], vals)
