"""CPU: dgpu_witness_map_r1cs_many is declared, exported by the product library and its development twin, and answers what it can decide without a
device before it looks at one: m = 0 is DGPU_OK with NULL pointers, every malformed call is DGPU_E_BADARG.  dgpu_set_wm_many lives in the twin only."""
import ctypes as C
import os
import re
import numpy as np
from crypto_amd._native import lib, dev_lib, SYMBOLS, DEV_SYMBOLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p_ = lambda a: a.ctypes.data_as(C.c_void_p)
OK, BADARG = 0, -3


def test_the_symbol_exists_in_the_header_the_library_and_the_twin():
    hdr = open(os.path.join(ROOT, "include", "dock_gpu.h")).read()
    assert re.search(r"int32_t dgpu_witness_map_r1cs_many\s*\(", hdr)
    assert "dgpu_witness_map_r1cs_many" in SYMBOLS and hasattr(lib(), "dgpu_witness_map_r1cs_many") and hasattr(dev_lib(), "dgpu_witness_map_r1cs_many")
    dev = open(os.path.join(ROOT, "include", "dock_gpu_dev.h")).read()
    assert re.search(r"int32_t dgpu_set_wm_many\s*\(", dev) and "dgpu_set_wm_many" in DEV_SYMBOLS
    assert hasattr(dev_lib(), "dgpu_set_wm_many") and not hasattr(lib(), "dgpu_set_wm_many")


def test_no_rows_is_ok_without_touching_anything():
    for L in (lib(), dev_lib()):
        assert L.dgpu_witness_map_r1cs_many(0, None, 0, 0, 0, 0, None, None, None) == OK
        assert L.dgpu_witness_map_r1cs_many(12345, None, 1, 5, 0, 3, None, None, None) == OK


def test_malformed_calls_are_refused_before_a_device_is_looked_at():
    L = lib()
    z = np.zeros((3, 8, 4), dtype=np.uint64)
    out = np.zeros((3, 16, 4), dtype=np.uint64)
    h, n = C.c_uint64(77), C.c_size_t(99)
    # NULL assignments; both outputs NULL; rows closer together than their length; a handle that does not exist; a handle of zero
    assert L.dgpu_witness_map_r1cs_many(1, None, 8, 8, 3, 0, p_(out), None, C.byref(n)) == BADARG
    assert L.dgpu_witness_map_r1cs_many(1, p_(z), 8, 8, 3, 0, None, None, C.byref(n)) == BADARG
    assert L.dgpu_witness_map_r1cs_many(1, p_(z), 7, 8, 3, 0, p_(out), C.byref(h), C.byref(n)) == BADARG
    assert L.dgpu_witness_map_r1cs_many(0xDEADBEEF, p_(z), 8, 8, 3, 0, p_(out), C.byref(h), C.byref(n)) == BADARG
    assert L.dgpu_witness_map_r1cs_many(0, p_(z), 8, 8, 3, 1, p_(out), None, None) == BADARG
    assert h.value == 77 and n.value == 99 and not out.any(), "a refused call writes nothing"


def test_the_knob_refuses_what_it_cannot_mean():
    T = dev_lib()
    for bad in ((-1, 0), (0, -1), (4097, 0), (0, 513)):
        assert T.dgpu_set_wm_many(*bad) == BADARG
    assert T.dgpu_set_wm_many(4, 2) == OK and T.dgpu_set_wm_many(0, 0) == OK
