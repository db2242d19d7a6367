"""CPU: the C ABI of the batched GT entry points without a device (dgpu_final_exponentiation_batch, dgpu_legogroth16_verify_each): exported,
n = 0 answers DGPU_OK at once, bad arguments DGPU_E_BADARG before the device check, valid arguments DGPU_E_NODEVICE when no device was initialised."""
import ctypes as C
import numpy as np
from crypto_amd._native import lib, SYMBOLS

OK, NODEVICE, BADARG = 0, -1, -3
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def test_exported():
    for name in ("dgpu_final_exponentiation_batch", "dgpu_legogroth16_verify_each"):
        assert name in SYMBOLS and hasattr(lib(), name)


def test_final_exponentiation_batch_arguments():
    f, out, z = np.zeros((2, 72), np.uint64), np.zeros((2, 72), np.uint64), np.zeros(2, np.uint8)
    L = lib()
    assert L.dgpu_final_exponentiation_batch(None, 0, None, None) == OK
    assert L.dgpu_final_exponentiation_batch(None, 2, p_(out), p_(z)) == BADARG
    assert L.dgpu_final_exponentiation_batch(p_(f), 2, None, p_(z)) == BADARG
    assert L.dgpu_final_exponentiation_batch(p_(f), 2, p_(out), None) == BADARG
    assert L.dgpu_final_exponentiation_batch(p_(f), 2, p_(out), p_(z)) == NODEVICE


def test_verify_each_arguments():
    gt, pc, g1, g2 = np.zeros(72, np.uint64), np.zeros(68 * 36, np.uint64), np.zeros(3 * 12, np.uint64), np.zeros(24, np.uint64)
    pub, ok = np.zeros(8, np.uint64), np.zeros(1, np.uint8)
    L = lib()
    call = lambda gt_, gabc_len, a, b, c, d, n, pubs, n_pub, okv: L.dgpu_legogroth16_verify_each(p_(gt_), p_(pc), p_(pc), p_(g1), gabc_len, p_(a), p_(b), p_(c), p_(d), n,
                                                                                                  p_(pubs), n_pub, 0, p_(okv))
    assert call(gt, 3, None, None, None, None, 0, None, 0, None) == OK
    assert call(gt, 3, None, None, None, None, 0, None, 2, None) == OK
    assert call(None, 3, g1, g2, g1, g1, 1, pub, 2, ok) == BADARG
    assert call(gt, 3, None, g2, g1, g1, 1, pub, 2, ok) == BADARG
    assert call(gt, 3, g1, g2, g1, g1, 1, pub, 2, None) == BADARG
    assert call(gt, 3, g1, g2, g1, g1, 1, None, 2, ok) == BADARG
    assert call(gt, 2, g1, g2, g1, g1, 1, pub, 2, ok) == BADARG                      # n_pub + 1 > gamma_abc_len: MalformedVerifyingKey
    assert call(gt, 3, g1, g2, g1, g1, 1, pub, 2, ok) == NODEVICE
