"""CPU: the host-side contract of the seven dgpu_saver_* calls (include/dock_gpu_saver.h, served by libdock_gpu_saver.so and its development build, NOT by the
product) — what can be decided without a device: the header, crypto_amd/_native.py and the libraries' exports agree, the product and its twin export none of them,
the development knob lives in the development builds alone, n = 0 is DGPU_OK with every pointer NULL and the empty batch
verifies, every DGPU_E_BADARG case of the header answers so before the device is looked at (NULL pointers with n > 0, chunk_bit_size 0 and 17, K = 0 and 256, a
handle that was never issued), and a well-formed call is stopped by the missing device only.  A LIVE handle of another kind and one that was freed need a device
to exist: tests/test_gpu_saver.py holds those two cases."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
slib = lambda: _native.saver_lib(bring_up=False)                 # libdock_gpu_saver.so, not brought up on a device
sdev = lambda: _native._load(_native._SAVER_DEV_SO)              # its development build

OK, NODEVICE, BADARG = 0, -1, -3
PREPARED_WORDS = 68 * 36
vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64
SIGNATURES = {"dgpu_saver_dk_create": [vp, vp, vp, vp, vp, i32, sz, C.POINTER(u64)],
              "dgpu_saver_dk_free": [u64],
              "dgpu_saver_dk_powers": [u64, sz, sz, sz, vp],
              "dgpu_saver_decrypt_many": [u64, vp, sz, vp, i32, vp, vp, vp],
              "dgpu_saver_verify_decryption_each": [u64, vp, sz, vp, vp, vp],
              "dgpu_saver_verify_commitment_each": [vp, sz, vp, sz, vp],
              "dgpu_saver_verify_commitments_batch": [vp, sz, vp, sz, vp, i32, C.POINTER(i32)]}
K, N = 3, 2


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_exported_and_declared():
    assert len(SIGNATURES) == 7
    hdr = open(os.path.join(ROOT, "include", "dock_gpu_saver.h")).read()
    assert sorted(set(re.findall(r"\b(dgpu_[a-z0-9_]+)\s*\(", hdr))) == sorted(SIGNATURES) == sorted(_native.SAVER_SYMBOLS)
    for name, args in SIGNATURES.items():
        assert name not in _native.SYMBOLS and not hasattr(lib(), name) and not hasattr(dev_lib(), name)      # the product exports exactly include/dock_gpu.h
        for L in (slib(), sdev()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args, name
    exported = lambda so: sorted(l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "crypto_amd", so)], text=True).splitlines() if " T dgpu_" in l)
    assert exported("libdock_gpu_saver.so") == sorted(_native.SYMBOLS + _native.SAVER_SYMBOLS)
    assert exported("libdock_gpu_saver_dev.so") == sorted(_native.SYMBOLS + _native.SAVER_SYMBOLS + _native.DEV_SYMBOLS)
    assert "dgpu_dev_set_saver_fp_bits" in _native.DEV_SYMBOLS and hasattr(sdev(), "dgpu_dev_set_saver_fp_bits") and not hasattr(slib(), "dgpu_dev_set_saver_fp_bits")


def test_the_fingerprint_knob_takes_minus_one_to_63():
    T = sdev()
    for bits in (-2, 64, 1000):
        assert T.dgpu_dev_set_saver_fp_bits(bits) == BADARG
    for bits in (-1, 3, 63, 0):
        assert T.dgpu_dev_set_saver_fp_bits(bits) == OK


class Args:
    def __init__(self):
        self.g, self.H, self.V0 = np.ones((K, 12), np.uint64), np.ones(24, np.uint64), np.ones(24, np.uint64)
        self.V1, self.V2 = np.ones((K, 24), np.uint64), np.ones((K, 24), np.uint64)
        self.ct, self.sk = np.ones((N, K + 2, 12), np.uint64), np.array([5, 0, 0, 0], np.uint64)
        self.chunks, self.nu = np.full((N, K), 9, np.uint16), np.ones((N, 12), np.uint64)
        self.status, self.ok1, self.h = np.full(N, 9, np.uint8), C.c_int32(-7), C.c_uint64(0)
        self.all_pc, self.w = np.ones((K + 2) * PREPARED_WORDS, np.uint64), np.ones((N, 4), np.uint64)
        self.out = np.zeros((2, 72), np.uint64)


@pytest.mark.parametrize("L", [slib, sdev], ids=["saver", "saver-dev"])
def test_n_zero_needs_nothing(L):
    L = L()
    ok1 = C.c_int32(-7)
    assert L.dgpu_saver_decrypt_many(0, None, 0, None, 0, None, None, None) == OK
    assert L.dgpu_saver_verify_decryption_each(0, None, 0, None, None, None) == OK
    assert L.dgpu_saver_verify_commitment_each(None, 0, None, 0, None) == OK
    assert L.dgpu_saver_verify_commitments_batch(None, 0, None, 0, None, 0, C.byref(ok1)) == OK and ok1.value == 1      # an empty batch verifies
    assert L.dgpu_saver_verify_commitments_batch(None, 0, None, 0, None, 0, None) == OK


def test_create_refuses_bad_shapes_and_nulls_before_the_device():
    L, a = slib(), Args()
    call = lambda g, H, V0, V1, V2, b, k, h: L.dgpu_saver_dk_create(g, H, V0, V1, V2, b, k, h)
    good = [p_(a.g), p_(a.H), p_(a.V0), p_(a.V1), p_(a.V2), 4, K, C.byref(a.h)]
    for b in (0, 17, -1):
        assert call(*(good[:5] + [b] + good[6:])) == BADARG
    for k in (0, 256):
        assert call(*(good[:6] + [k] + good[7:])) == BADARG
    for i in (0, 1, 2, 3, 4, 7):
        args = list(good); args[i] = None
        assert call(*args) == BADARG, i
    if L.dgpu_context_count() == 0:                                         # (the suite's CPU half never initialises a device; with one these calls would run)
        assert call(*good) == NODEVICE and a.h.value == 0
        for b, k in ((1, 1), (16, 255)):                                    # the corners of the range pass the argument checks
            assert call(*(good[:5] + [b, k] + good[7:])) == NODEVICE


def test_calls_refuse_nulls_and_foreign_handles_before_the_device():
    L, a = slib(), Args()
    dec = lambda h=12345, ct=p_(a.ct), sk=p_(a.sk), ch=p_(a.chunks), nu=p_(a.nu), st=p_(a.status): L.dgpu_saver_decrypt_many(h, ct, N, sk, 0, ch, nu, st)
    ver = lambda h=12345, ct=p_(a.ct), ch=p_(a.chunks), nu=p_(a.nu), ok=p_(a.status): L.dgpu_saver_verify_decryption_each(h, ct, N, ch, nu, ok)
    for kw in ({"ct": None}, {"sk": None}, {"ch": None}, {"nu": None}, {"st": None}):
        assert dec(**kw) == BADARG, kw
    for kw in ({"ct": None}, {"ch": None}, {"nu": None}, {"ok": None}):
        assert ver(**kw) == BADARG, kw
    # a handle nobody issued (0, a stale number): not a live SAVER key
    for h in (0, 12345, 2 ** 63):
        assert dec(h=h) == BADARG and ver(h=h) == BADARG
        assert L.dgpu_saver_dk_free(h) == BADARG
        assert L.dgpu_saver_dk_powers(h, 0, 1, 1, p_(a.out)) == BADARG
    assert (a.status == 9).all() and (a.chunks == 9).all()
    each = lambda pc=p_(a.all_pc), k=K, ct=p_(a.ct), ok=p_(a.status): L.dgpu_saver_verify_commitment_each(pc, k, ct, N, ok)
    batch = lambda pc=p_(a.all_pc), k=K, ct=p_(a.ct), w=p_(a.w), ok=C.byref(a.ok1): L.dgpu_saver_verify_commitments_batch(pc, k, ct, N, w, 0, ok)
    for kw in ({"pc": None}, {"ct": None}, {"ok": None}, {"k": 0}, {"k": 256}):
        assert each(**kw) == BADARG and batch(**kw) == BADARG, kw
    assert batch(w=None) == BADARG
    if L.dgpu_context_count() == 0:
        assert each() == NODEVICE and batch() == NODEVICE and a.ok1.value == -7
