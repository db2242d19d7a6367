"""CPU: the host-side contract of dgpu_msm_g1_segments / dgpu_msm_g2_segments (include/dock_gpu.h) — what can be decided without a device: the symbols
are exported by the product and its twin and declared in crypto_amd/_native.py, the development knob is on the twin only, an empty batch is DGPU_OK
whatever the pointers, argument errors are DGPU_E_BADARG (decided before the device is looked at, `out` untouched), and a batch with work in it answers
DGPU_E_NODEVICE (never "too small") when no device was initialised."""
import ctypes as C
import numpy as np
import pytest
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

OK, NODEVICE, BADARG, TOO_SMALL = 0, -1, -3, -6
NAMES = ("dgpu_msm_g1_segments", "dgpu_msm_g2_segments")


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_exported_and_declared():
    for name in NAMES:
        assert name in _native.SYMBOLS
        for L in (lib(), dev_lib()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32
            assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p]
    assert "dgpu_set_msm_segments" in _native.DEV_SYMBOLS
    assert hasattr(dev_lib(), "dgpu_set_msm_segments")
    with pytest.raises(AttributeError):
        lib().dgpu_set_msm_segments                          # the knob is not part of the product


def test_knob_refuses_what_it_cannot_set():
    T = dev_lib()
    assert T.dgpu_set_msm_segments(3, 0) == BADARG and T.dgpu_set_msm_segments(-1, 0) == BADARG
    assert T.dgpu_set_msm_segments(0, -1) == BADARG and T.dgpu_set_msm_segments(0, (1 << 20) + 1) == BADARG
    assert T.dgpu_set_msm_segments(2, 100) == OK and T.dgpu_set_msm_segments(0, 0) == OK


@pytest.mark.parametrize("name,aw", [(NAMES[0], 12), (NAMES[1], 24)])
def test_refusals_without_a_device(name, aw):
    L = lib()
    fn = getattr(L, name)
    jw = aw * 3 // 2
    N, nseg = 12, 4
    bases = np.ones((N, aw), np.uint64)
    sc = np.ones((N, 4), np.uint64)
    inf = np.zeros(N, np.uint8)
    se = np.array([3, 3, 7, 12], np.uint64)
    out = np.zeros((nseg, jw), np.uint64)
    oinf = np.zeros(nseg, np.uint8)
    # nseg = 0: DGPU_OK with NULL pointers and no device, whatever the other arguments say
    assert fn(None, None, None, 0, None, 0, 0, None, None) == OK
    assert fn(None, None, None, 12345, None, 0, 1, None, None) == OK
    # a NULL pointer among bases / scalars / out / seg_end: DGPU_E_BADARG
    assert fn(None, p_(inf), p_(sc), N, p_(se), nseg, 0, p_(out), p_(oinf)) == BADARG
    assert fn(p_(bases), p_(inf), None, N, p_(se), nseg, 0, p_(out), p_(oinf)) == BADARG
    assert fn(p_(bases), p_(inf), p_(sc), N, p_(se), nseg, 0, None, p_(oinf)) == BADARG
    assert fn(p_(bases), p_(inf), p_(sc), N, None, nseg, 0, p_(out), p_(oinf)) == BADARG
    # a descending seg_end; a last seg_end that is not N (short and long); N >= 2^31
    bad = np.array([3, 2, 7, 12], np.uint64)
    assert fn(p_(bases), p_(inf), p_(sc), N, p_(bad), nseg, 0, p_(out), p_(oinf)) == BADARG
    assert fn(p_(bases), p_(inf), p_(sc), N - 1, p_(se), nseg, 0, p_(out), p_(oinf)) == BADARG
    assert fn(p_(bases), p_(inf), p_(sc), N + 1, p_(se), nseg, 0, p_(out), p_(oinf)) == BADARG
    assert fn(p_(bases), p_(inf), p_(sc), N, p_(se), nseg - 1, 0, p_(out), p_(oinf)) == BADARG
    huge = np.array([1 << 31], np.uint64)
    assert fn(p_(bases), None, p_(sc), 1 << 31, p_(huge), 1, 0, p_(out), None) == BADARG
    assert not out.any() and not oinf.any()


@pytest.mark.parametrize("name,aw", [(NAMES[0], 12), (NAMES[1], 24)])
def test_no_device_is_answered_before_any_size_threshold(name, aw):
    """work without a device: DGPU_E_NODEVICE, never "too small" (a one-term batch is below every threshold), `out` untouched"""
    L = lib()
    if L.dgpu_context_count() != 0:
        pytest.skip("a device context exists in this process (a GPU test ran before): the refusal needs a process without one")
    fn = getattr(L, name)
    jw = aw * 3 // 2
    N, nseg = 12, 4
    bases, sc, inf = np.ones((N, aw), np.uint64), np.ones((N, 4), np.uint64), np.zeros(N, np.uint8)
    se = np.array([3, 3, 7, 12], np.uint64)
    out, oinf = np.zeros((nseg, jw), np.uint64), np.zeros(nseg, np.uint8)
    assert fn(p_(bases), p_(inf), p_(sc), N, p_(se), nseg, 0, p_(out), p_(oinf)) == NODEVICE
    one = np.array([1], np.uint64)
    assert fn(p_(bases), None, p_(sc), 1, p_(one), 1, 0, p_(out), None) == NODEVICE
    assert not out.any() and not oinf.any()
