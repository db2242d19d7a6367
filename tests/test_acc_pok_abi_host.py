"""CPU: the host-side contract of the four accumulator proof calls (include/dock_gpu.h: dgpu_accumulator_membership_proofs_verify_each_g1 / _verify_batch_g1,
dgpu_accumulator_non_membership_proofs_verify_each_g1 / _verify_batch_g1) — what can be decided without a device: the symbols are exported by the product and
its twin and declared in crypto_amd/_native.py, n = 0 is DGPU_OK with every pointer NULL and the empty batch verifies, every DGPU_E_BADARG case that needs no
device answers so before the device is looked at (NULL pointers, n = 2^31, rho = 0 as 0 and as r), and a well-formed call is stopped by the missing device
only.  The two challenge-contribution functions of crypto_amd.accumulator byte for byte against a layout built here from the oracle's field conversion and the
Zcash flags."""
import ctypes as C
import numpy as np
import pytest
import oracle_c as O
from crypto_amd import _native
from crypto_amd import accumulator as ACC
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R2 = pow(2, 256, R)
PREPARED_WORDS = 68 * 36
vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
MEM_EACH, MEM_BATCH = "dgpu_accumulator_membership_proofs_verify_each_g1", "dgpu_accumulator_membership_proofs_verify_batch_g1"
NM_EACH, NM_BATCH = "dgpu_accumulator_non_membership_proofs_verify_each_g1", "dgpu_accumulator_non_membership_proofs_verify_batch_g1"


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def test_symbols_exported_and_declared():
    want = {MEM_EACH: [vp] * 6 + [sz, i32, vp], MEM_BATCH: [vp] * 6 + [sz, i32, vp, C.POINTER(i32)],
            NM_EACH: [vp] * 8 + [sz, i32, vp], NM_BATCH: [vp] * 8 + [sz, i32, vp, C.POINTER(i32)]}
    for name, args in want.items():
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args
    hdr = open(_native.__file__.replace("crypto_amd/_native.py", "include/dock_gpu.h")).read()
    for name in want:
        assert "int32_t %s(" % name in hdr


class Args:
    """well-formed calls: three proofs of either kind"""
    def __init__(self, mont=False):
        self.f = (lambda vals: limbs([v * R2 % R for v in vals])) if mont else limbs
        self.mont = 1 if mont else 0
        self.rho = self.f([5])
        self.v, self.p, self.q = np.ones(12, np.uint64), np.ones(12, np.uint64) * 2, np.ones(12, np.uint64) * 3
        self.points = {0: np.ones((3, 3, 12), np.uint64), 1: np.ones((3, 5, 12), np.uint64)}
        self.resp = {0: self.f(list(range(30, 36))), 1: self.f(list(range(30, 39)))}
        self.chal = self.f([11, 12, 13])
        self.pk, self.pt = np.ones(PREPARED_WORDS, np.uint64), np.ones(PREPARED_WORDS, np.uint64)
        self.status, self.ok1 = np.full(3, 9, np.uint8), C.c_int32(-7)

    def base(self, kind, kw):
        a = dict(v=p_(self.v), p=p_(self.p), q=p_(self.q), pk=p_(self.pk), pt=p_(self.pt), points=p_(self.points[kind]), resp=p_(self.resp[kind]), chal=p_(self.chal), n=3,
                 status=p_(self.status), rho=p_(self.rho), ok1=C.byref(self.ok1))
        a.update(kw)
        head = [a["v"]] + ([a["p"], a["q"]] if kind else []) + [a["pk"], a["pt"], a["points"], a["resp"], a["chal"], a["n"], self.mont]
        return a, head

    def each(self, lb, kind, **kw):
        a, head = self.base(kind, kw)
        return getattr(lb, NM_EACH if kind else MEM_EACH)(*head, a["status"])

    def batch(self, lb, kind, **kw):
        a, head = self.base(kind, kw)
        return getattr(lb, NM_BATCH if kind else MEM_BATCH)(*head, a["rho"], a["ok1"])


def test_no_rows_need_no_device_and_read_nothing():
    L = lib()
    assert getattr(L, MEM_EACH)(None, None, None, None, None, None, 0, 0, None) == OK
    assert getattr(L, NM_EACH)(None, None, None, None, None, None, None, None, 0, 1, None) == OK
    assert getattr(L, MEM_BATCH)(None, None, None, None, None, None, 0, 0, None, None) == OK
    assert getattr(L, NM_BATCH)(None, None, None, None, None, None, None, None, 0, 0, None, None) == OK
    for name, nhead in ((MEM_BATCH, 6), (NM_BATCH, 8)):
        ok = C.c_int32(-7)
        assert getattr(L, name)(*([None] * nhead), 0, 1, None, C.byref(ok)) == OK and ok.value == 1      # the empty batch verifies


def test_a_well_formed_call_is_stopped_by_the_missing_device_only():
    L = lib()
    no_device = L.dgpu_context_count() == 0      # (the suite's CPU half never initialises a device; with one, nothing stops these calls: they run and answer)
    want = NODEVICE if no_device else OK
    for mont in (False, True):
        A = Args(mont)
        for kind in (0, 1):
            assert A.each(L, kind) == want and A.batch(L, kind) == want
            assert A.batch(L, kind, rho=p_(A.f([R - 1]))) == want
        assert not no_device or ((A.status == 9).all() and A.ok1.value == -7)


def test_bad_arguments_answer_before_the_device():
    L = lib()
    A = Args()
    for kind in (0, 1):
        nulls = ["v", "pk", "pt", "points", "resp", "chal"] + (["p", "q"] if kind else [])
        for kw in [{k: None} for k in nulls] + [dict(n=1 << 31), dict(n=(1 << 40) + 3)]:
            assert A.each(L, kind, **kw) == BADARG, (kind, kw)
            assert A.batch(L, kind, **kw) == BADARG, (kind, kw)
        assert A.each(L, kind, status=None) == BADARG
        assert A.batch(L, kind, ok1=None) == BADARG and A.batch(L, kind, rho=None) == BADARG
    assert (A.status == 9).all() and A.ok1.value == -7


def test_a_zero_batching_scalar_is_refused_before_the_device():
    L = lib()
    A = Args()
    for kind in (0, 1):
        assert A.batch(L, kind, rho=p_(limbs([0]))) == BADARG
        assert A.batch(L, kind, rho=p_(limbs([R]))) == BADARG                                       # canonical words are taken mod r
        assert A.batch(L, kind, rho=p_(limbs([2 * R]))) == BADARG
        assert Args(True).batch(L, kind, rho=p_(limbs([0]))) == BADARG
    assert A.ok1.value == -7


def test_the_python_wrappers_count_their_rows():
    with pytest.raises(ValueError):
        ACC._acc_proofs(np.ones((3, 3, 12), np.uint64), 3, [[1, 2]] * 2, 2, [5, 6, 7])
    with pytest.raises(ValueError):
        ACC._acc_proofs(np.ones((3, 5, 12), np.uint64), 5, [[1, 2, 3]] * 3, 3, [5, 6])
    n, pts, resp, c = ACC._acc_proofs(np.ones((3, 5, 12), np.uint64), 5, [[1, 2, 3]] * 3, 3, [5, 6, 7])
    assert n == 3 and pts.shape == (3, 5, 12) and resp.shape == (3, 3, 4) and resp[1, 2, 0] == 3 and c.shape == (3, 4)
    n, pts, resp, c = ACC._acc_proofs(np.zeros((0, 3, 12), np.uint64), 3, [], 2, [])
    assert n == 0 and resp.shape == (0, 2, 4)


def compressed(pt):
    """ark-serialize's compressed G1 (Zcash flags) from affine Montgomery words, through the oracle's field conversion"""
    if not pt.any():
        return bytes([0xC0]) + bytes(47)
    x, y = [sum(int(w) << (64 * k) for k, w in enumerate(O.fp_from_mont(pt[6 * h:6 * h + 6]))) for h in (0, 1)]
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if y > (P - 1) // 2 else 0)
    return bytes(b)


def test_challenge_contributions_byte_for_byte():
    """Abar, A', V, T (weak_bb_sig_pok_cdh.rs:129-141), respectively Cbar, C', J, V, P, Q, T1, T2 (proofs_cdh.rs:326-346), all compressed"""
    pts = O.G1.gen_seq(O.rand_scalars(1, 1)[0], O.rand_scalars(2, 1)[0], 11, threads=1)
    V, Pp, Q = pts[0], pts[1], pts[2]
    mem, nm = pts[3:6].copy(), pts[6:11].copy()
    got = ACC.membership_challenge_contribution(V, mem)
    assert got == b"".join(compressed(q) for q in (mem[1], mem[0], V, mem[2])) and len(got) == 4 * 48
    mem[2] = 0                                                                # an identity T has a byte layout too
    assert ACC.membership_challenge_contribution(V, mem) == b"".join(compressed(q) for q in (mem[1], mem[0], V, mem[2]))
    got = ACC.non_membership_challenge_contribution(V, Pp, Q, nm)
    assert got == b"".join(compressed(q) for q in (nm[1], nm[0], nm[2], V, Pp, Q, nm[3], nm[4])) and len(got) == 8 * 48
    nm[3] = nm[4] = 0
    assert ACC.non_membership_challenge_contribution(V, Pp, Q, nm) == b"".join(compressed(q) for q in (nm[1], nm[0], nm[2], V, Pp, Q, nm[3], nm[4]))
    assert {compressed(q)[0] & 0x20 for q in pts} == {0, 0x20}                # both signs of y among the points
    with pytest.raises(ValueError):
        ACC.membership_challenge_contribution(V, nm)
