"""arkworks `CanonicalSerialize` / `CanonicalDeserialize` for BLS12-381 group elements (Zcash format) over the C ABI:
what the reference's keys and proofs look like on disk (legogroth16/src/data_structures.rs:7-186, utils/src/serde_utils.rs:8-33)."""
import ctypes as C
import numpy as np
from ._native import lib, DockGpuError

_SZ = {("g1", True): 48, ("g1", False): 96, ("g2", True): 96, ("g2", False): 192}


def serialize(curve, points, is_inf=None, compressed=True):
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, curve.AW)
    inf = None if is_inf is None else np.ascontiguousarray(is_inf, dtype=np.uint8)
    out = np.zeros(len(pts) * _SZ[(curve.tag, compressed)], dtype=np.uint8)
    fn = lib().dgpu_g1_serialize if curve.tag == "g1" else lib().dgpu_g2_serialize
    rc = fn(pts.ctypes.data_as(C.c_void_p), None if inf is None else inf.ctypes.data_as(C.c_void_p), len(pts), int(compressed), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise DockGpuError(rc, "serialize")
    return out.tobytes()


def serialize_device(curve, points, is_inf=None, compressed=True):
    """serialize() on the device (dgpu_*_serialize_device): the same bytes"""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, curve.AW)
    inf = None if is_inf is None else np.ascontiguousarray(is_inf, dtype=np.uint8)
    out = np.zeros(len(pts) * _SZ[(curve.tag, compressed)], dtype=np.uint8)
    fn = lib().dgpu_g1_serialize_device if curve.tag == "g1" else lib().dgpu_g2_serialize_device
    rc = fn(pts.ctypes.data_as(C.c_void_p), None if inf is None else inf.ctypes.data_as(C.c_void_p), len(pts), int(compressed), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise DockGpuError(rc, "serialize_device")
    return out.tobytes()


def read_handle(curve, handle, offset, n):
    """dgpu_bases_read_*: (words, is_inf) of points [offset, offset + n) of a resident bases handle"""
    pts = np.zeros((n, curve.AW), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    rc = getattr(lib(), "dgpu_bases_read_%s" % curve.tag)(handle, offset, n, pts.ctypes.data_as(C.c_void_p), inf.ctypes.data_as(C.c_void_p))
    if rc:
        raise DockGpuError(rc, "dgpu_bases_read")
    return pts, inf


def serialize_handle(curve, handle, offset, n, compressed=True):
    """dgpu_bases_serialize_*: the encoded points [offset, offset + n) of a resident bases handle"""
    out = np.zeros(n * _SZ[(curve.tag, compressed)], dtype=np.uint8)
    rc = getattr(lib(), "dgpu_bases_serialize_%s" % curve.tag)(handle, offset, n, int(compressed), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise DockGpuError(rc, "dgpu_bases_serialize")
    return out.tobytes()


def deserialize(curve, data, compressed=True, validate=True):
    """CanonicalDeserialize: validate=True is Validate::Yes (curve + prime-order subgroup), False is Validate::No (curve only)"""
    sz = _SZ[(curve.tag, compressed)]
    if len(data) % sz:
        raise ValueError("length is not a multiple of %d" % sz)
    n = len(data) // sz
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    pts = np.zeros((n, curve.AW), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    fn = lib().dgpu_g1_deserialize if curve.tag == "g1" else lib().dgpu_g2_deserialize
    rc = fn(buf.ctypes.data_as(C.c_void_p), n, int(compressed) | (0 if validate else 2), pts.ctypes.data_as(C.c_void_p), inf.ctypes.data_as(C.c_void_p))
    if rc:
        raise DockGpuError(rc, "deserialize")
    return pts, inf


def _refused(rc, what, first_bad):
    err = DockGpuError(rc, what)
    err.index = first_bad if rc == -3 else None          # the lowest refused point (DGPU_E_BADARG)
    return err


def deserialize_device(curve, data, compressed=True, validate=True):
    """deserialize() on the device (dgpu_*_deserialize_device): the same verdict, words and flags.  A refused input raises DockGpuError whose
    `index` is the lowest refused point."""
    sz = _SZ[(curve.tag, compressed)]
    if len(data) % sz:
        raise ValueError("length is not a multiple of %d" % sz)
    n = len(data) // sz
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    pts = np.zeros((n, curve.AW), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    bad = C.c_size_t(0)
    fn = lib().dgpu_g1_deserialize_device if curve.tag == "g1" else lib().dgpu_g2_deserialize_device
    rc = fn(buf.ctypes.data_as(C.c_void_p), n, int(compressed) | (0 if validate else 2), pts.ctypes.data_as(C.c_void_p), inf.ctypes.data_as(C.c_void_p), C.byref(bad))
    if rc:
        raise _refused(rc, "deserialize_device", bad.value)
    return pts, inf


def validate(curve, points, is_inf=None):
    """Validate::Yes of affine ABI words on the device (dgpu_*_validate_batch): a bool per point — the identity, or reduced, on the curve and in
    the prime-order subgroup"""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, curve.AW)
    inf = None if is_inf is None else np.ascontiguousarray(is_inf, dtype=np.uint8)
    ok = np.zeros(len(pts), dtype=np.uint8)
    fn = lib().dgpu_g1_validate_batch if curve.tag == "g1" else lib().dgpu_g2_validate_batch
    rc = fn(pts.ctypes.data_as(C.c_void_p), None if inf is None else inf.ctypes.data_as(C.c_void_p), len(pts), ok.ctypes.data_as(C.c_void_p))
    if rc:
        raise DockGpuError(rc, "validate")
    return ok.astype(bool)
