"""CPU: the C ABI of the device GT entry points without a device (dgpu_fp12_pow_batch, dgpu_fp12_multi_pow_device, dgpu_gt_in_subgroup_device):
exported by the product library, their knob dgpu_set_gt_pow by the development twin only; n = 0 answers DGPU_OK at once (the product of no powers is
the element one), bad arguments DGPU_E_BADARG before the device check, valid arguments DGPU_E_NODEVICE when no device was initialised."""
import ctypes as C
import numpy as np
import pytest
import torch
import oracle_c as O
from crypto_amd._native import lib, dev_lib, SYMBOLS, DEV_SYMBOLS

OK, NODEVICE, BADARG = 0, -1, -3
NAMES = ("dgpu_fp12_pow_batch", "dgpu_fp12_multi_pow_device", "dgpu_gt_in_subgroup_device")
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def test_exported_by_the_product_and_the_knob_by_the_twin_only():
    for name in NAMES:
        assert name in SYMBOLS and hasattr(lib(), name) and hasattr(dev_lib(), name)
    assert "dgpu_set_gt_pow" in DEV_SYMBOLS and hasattr(dev_lib(), "dgpu_set_gt_pow") and not hasattr(lib(), "dgpu_set_gt_pow")
    T = dev_lib()
    assert T.dgpu_set_gt_pow(11, 0, 0) == BADARG and T.dgpu_set_gt_pow(0, 9, 0) == BADARG and T.dgpu_set_gt_pow(0, 0, -1) == BADARG
    assert T.dgpu_set_gt_pow(10, 8, 16) == OK and T.dgpu_set_gt_pow(0, 0, 0) == OK


def test_nothing_to_do_needs_no_device():
    L = lib()
    assert L.dgpu_fp12_pow_batch(None, None, 4, 0, None) == OK
    assert L.dgpu_gt_in_subgroup_device(None, 0, None) == OK
    out = np.zeros(72, np.uint64)
    assert L.dgpu_fp12_multi_pow_device(None, None, 0, p_(out)) == OK
    assert (out == np.asarray(O.fp12_one(), np.uint64)).all()


def test_bad_arguments_come_before_the_device_check():
    L = lib()
    a, e, out, ok = np.zeros((2, 72), np.uint64), np.ones((2, 4), np.uint64), np.zeros((2, 72), np.uint64), np.zeros(2, np.uint8)
    assert L.dgpu_fp12_pow_batch(None, p_(e), 4, 2, p_(out)) == BADARG
    assert L.dgpu_fp12_pow_batch(p_(a), None, 4, 2, p_(out)) == BADARG
    assert L.dgpu_fp12_pow_batch(p_(a), p_(e), 4, 2, None) == BADARG
    assert L.dgpu_fp12_pow_batch(p_(a), p_(e), 3, 2, p_(out)) == BADARG
    assert L.dgpu_fp12_pow_batch(p_(a), p_(e), 3, 0, p_(out)) == BADARG
    assert L.dgpu_fp12_multi_pow_device(None, p_(e), 2, p_(out)) == BADARG
    assert L.dgpu_fp12_multi_pow_device(p_(a), None, 2, p_(out)) == BADARG
    assert L.dgpu_fp12_multi_pow_device(p_(a), p_(e), 2, None) == BADARG
    assert L.dgpu_fp12_multi_pow_device(None, None, 0, None) == BADARG
    assert L.dgpu_gt_in_subgroup_device(None, 2, p_(ok)) == BADARG
    assert L.dgpu_gt_in_subgroup_device(p_(a), 2, None) == BADARG


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device behaviour")
def test_one_element_without_a_device():
    L = lib()
    a, e, out, ok = np.zeros((1, 72), np.uint64), np.ones((1, 4), np.uint64), np.zeros((1, 72), np.uint64), np.zeros(1, np.uint8)
    assert L.dgpu_fp12_pow_batch(p_(a), p_(e), 4, 1, p_(out)) == NODEVICE
    assert L.dgpu_fp12_pow_batch(p_(a), p_(e), 0, 1, p_(out)) == NODEVICE
    assert L.dgpu_fp12_multi_pow_device(p_(a), p_(e), 1, p_(out)) == NODEVICE
    assert L.dgpu_gt_in_subgroup_device(p_(a), 1, p_(ok)) == NODEVICE
