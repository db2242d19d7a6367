"""CPU: the host-side contract of dgpu_msm_g1_handle_many / dgpu_msm_g2_handle_many (include/dock_gpu.h) — what can be decided without a device: the
symbols are exported by the product and its twin and declared in crypto_amd/_native.py, an empty batch is DGPU_OK whatever the pointers, argument
errors are DGPU_E_BADARG, and a batch with work in it answers DGPU_E_NODEVICE (never "too small") when no device was initialised."""
import ctypes as C
import numpy as np
import pytest
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG, TOO_SMALL = 0, -1, -3, -6
NAMES = ("dgpu_msm_g1_handle_many", "dgpu_msm_g2_handle_many")


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_exported_and_declared():
    for name in NAMES:
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32
            assert fn.argtypes == [C.c_uint64, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p]
    assert "dgpu_set_many_chunk_rows" in _native.DEV_SYMBOLS
    assert hasattr(dev_lib(), "dgpu_set_many_chunk_rows")
    with pytest.raises(AttributeError):
        lib().dgpu_set_many_chunk_rows                       # the knob is not part of the product


def test_codes_are_the_header_s():
    assert (NODEVICE, BADARG, TOO_SMALL) == (-1, -3, -6)
    assert lib().dgpu_strerror(BADARG) and lib().dgpu_strerror(NODEVICE)


@pytest.mark.parametrize("name,jw", [(NAMES[0], 18), (NAMES[1], 36)])
def test_refusals_without_a_device(name, jw):
    L = lib()
    no_device = L.dgpu_context_count() == 0                  # (the suite's CPU half never initialises one)
    fn = getattr(L, name)
    m, n = 5, 12
    sc = np.ones((m, n, 4), np.uint64)
    out = np.zeros((m, jw), np.uint64)
    inf = np.zeros(m, np.uint8)
    # m = 0: DGPU_OK with NULL pointers and no device, whatever the other arguments say
    assert fn(0, 0, None, 0, 0, 0, 0, None, None) == OK
    assert fn(12345, 7, None, 1, n, 0, 1, None, None) == OK
    # m, n > 0 without a device: DGPU_E_NODEVICE — answered before any size threshold (m * n = 1 is below every threshold)
    if no_device:
        assert fn(1, 0, p_(sc), n, n, m, 0, p_(out), p_(inf)) == NODEVICE
        assert fn(1, 0, p_(sc), n, 1, 1, 0, p_(out), None) == NODEVICE
    # NULL pointers with m, n > 0, and row_stride < n: DGPU_E_BADARG (decided before the device is looked at)
    assert fn(1, 0, None, n, n, m, 0, p_(out), p_(inf)) == BADARG
    assert fn(1, 0, p_(sc), n, n, m, 0, None, p_(inf)) == BADARG
    assert fn(1, 0, p_(sc), n - 1, n, m, 0, p_(out), p_(inf)) == BADARG
    assert fn(1, 0, p_(sc), 0, n, m, 0, p_(out), None) == BADARG
    assert not out.any()
    # n = 0, m > 0: no scalars are needed (NULL is fine); without a device the single call's answer for n = 0
    if no_device:
        assert fn(1, 0, None, 0, 0, m, 0, p_(out), None) == NODEVICE
    assert fn(1, 0, None, 0, 0, m, 0, None, None) == BADARG
