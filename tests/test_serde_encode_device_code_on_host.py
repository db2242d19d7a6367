"""CPU: the DEVICE point encoding routines (crypto_amd/csrc/serde_kernels.hip.h: encode_point, record_to_abi) compiled for the host with the
FP29_CHECK bound tracker (tests/native/serde_enc_host_shim.cpp), checked byte for byte against the host encoders dgpu_g1_serialize /
dgpu_g2_serialize.  A green run shows the encoding is right and its lazy-limb arithmetic cannot overflow.  Also the C ABI of the device encoders
and of the handle readers without a device: exported, declared, DGPU_E_BADARG for bad arguments first, then DGPU_E_NODEVICE."""
import ctypes as C
import os
import random
import re
import subprocess
import numpy as np
import pytest
import bls12_381_model as M
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd import serde
from crypto_amd._native import lib, SYMBOLS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "serde_enc_host_shim.cpp")
SO = os.path.join(HERE, "native", "libserde_enc_host_shim.so")
HEADER = os.path.join(HERE, "..", "include", "dock_gpu.h")
P = M.P
NEW = ["dgpu_g1_serialize_device", "dgpu_g2_serialize_device", "dgpu_bases_read_g1", "dgpu_bases_read_g2", "dgpu_bases_serialize_g1", "dgpu_bases_serialize_g2"]


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(HERE, "..", "crypto_amd", "csrc", f) for f in ("serde_kernels.hip.h", "fp29.hip.h", "fp2_29.hip.h", "ec29.hip.h", "fp30s.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    return C.CDLL(SO)


def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def nfp(curve):
    return 1 if curve.tag == "g1" else 2


def limbs_int(w):
    return sum(int(x) << (64 * i) for i, x in enumerate(w))


def int_limbs(v):
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(6)], np.uint64)


def neg_words(curve, pts):
    """-P for every row: each y component c becomes p - c (Montgomery limbs; a zero component stays zero)"""
    out = pts.copy()
    for row in out:
        for k in range(nfp(curve), 2 * nfp(curve)):
            v = limbs_int(row[6 * k:6 * k + 6])
            row[6 * k:6 * k + 6] = int_limbs((P - v) % P)
    return out


def dev_encode(shim, curve, pts, inf, compressed):
    pts = np.ascontiguousarray(pts, np.uint64)
    out = np.zeros(len(pts) * (48 if compressed else 96) * nfp(curve), np.uint8)
    shim.shim_encode(nfp(curve), p_(pts), p_(inf), len(pts), int(compressed), p_(out))
    return out.tobytes()


def dev_record(shim, curve, pts, inf, compressed):
    pts = np.ascontiguousarray(pts, np.uint64)
    back, binf = np.zeros_like(pts), np.zeros(len(pts), np.uint8)
    out = np.zeros(len(pts) * (48 if compressed else 96) * nfp(curve), np.uint8)
    shim.shim_record(nfp(curve), p_(pts), p_(inf), len(pts), int(compressed), p_(back), p_(binf), p_(out))
    return back, binf, out.tobytes()


def check(shim, curve, pts, inf):
    """device routines == dgpu_g*_serialize in both compressions, direct and through a base record; the words a record reads back"""
    pts = np.ascontiguousarray(pts, np.uint64)
    ident = (inf.astype(bool) if inf is not None else np.zeros(len(pts), bool)) | ~pts.any(axis=1)
    for compressed in (True, False):
        want = serde.serialize(curve, pts, inf, compressed)
        assert dev_encode(shim, curve, pts, inf, compressed) == want, (curve.tag, compressed)
        back, binf, enc = dev_record(shim, curve, pts, inf, compressed)
        assert enc == want, (curve.tag, compressed)
        assert (binf.astype(bool) == ident).all() and not back[ident].any() and (back[~ident] == pts[~ident]).all()


def flags(curve, data, compressed=True):
    sz = (48 if compressed else 96) * nfp(curve)
    return [data[i] & 0xe0 for i in range(0, len(data), sz)]


def twist_points_with_real_y(k, seed):
    """k points on the twist y^2 = x^3 + 4 (1 + u) whose y has c1 = 0, as model pairs ((x0, x1), (y0, 0)): x = x0 + x1 u with
    3 x0^2 x1 - x1^3 + 4 = 0 makes x^3 + 4 (1 + u) real.  They lie outside G2 (the encoder does not care: it never validates)."""
    rnd, out = random.Random(seed), []
    while len(out) < k:
        x1 = rnd.randrange(1, P)
        x0 = U.fp_sqrt((x1 ** 3 - 4) * pow(3 * x1, P - 2, P) % P)
        if x0 is None:
            continue
        y0 = U.fp_sqrt((x0 ** 3 - 3 * x0 * x1 * x1 + 4) % P)
        if y0 is None or y0 == 0:
            continue
        x, y = (x0, x1), (y0, 0)
        assert M.f2_sqr(y) == M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.B_TWIST)
        out.append((x, y))
    return out


def test_random_points_and_their_negatives(shim):
    """P and -P of random points (both values of the "largest" flag occur), plus the small multiples of the generator"""
    for curve, G in ((ca.G1, O.G1), (ca.G2, O.G2)):
        pts = G.gen_seq(O.rand_scalars(11, 1)[0], O.rand_scalars(12, 1)[0], 48, threads=4)
        pts = np.concatenate([pts, neg_words(curve, pts), G.gen_seq(1, 1, 4, threads=1)])
        check(shim, curve, pts, None)
        fl = flags(curve, serde.serialize(curve, pts, None, True))
        assert {0x80, 0xa0} <= set(fl), curve.tag


def test_g2_points_whose_y_has_no_c1(shim):
    """y.c1 = 0: the flag follows y.c0 (dock_serde.cpp is_high2); the points and their negatives give both values"""
    pts = np.stack([U.g2_abi(pt)[0] for pt in twist_points_with_real_y(12, 3)])
    pts = np.concatenate([pts, neg_words(ca.G2, pts)])
    assert not pts[:, 18:24].any()
    check(shim, ca.G2, pts, None)
    assert set(flags(ca.G2, serde.serialize(ca.G2, pts, None, True))) == {0x80, 0xa0}


def test_identities_given_either_way(shim):
    """is_inf = 1 over non-zero words, all-zero words with is_inf = 0, and no flag array at all: the flag byte followed by zeros"""
    for curve, G in ((ca.G1, O.G1), (ca.G2, O.G2)):
        pts = G.gen_seq(O.rand_scalars(21, 1)[0], O.rand_scalars(22, 1)[0], 10, threads=2)
        pts[[2, 7]] = 0
        inf = np.zeros(len(pts), np.uint8); inf[[0, 5, 7]] = 1
        check(shim, curve, pts, inf)
        check(shim, curve, pts, None)
        for compressed in (True, False):
            data = serde.serialize(curve, pts, inf, compressed)
            fl = flags(curve, data, compressed)
            assert [fl[i] for i in (0, 2, 5, 7)] == [(0x80 if compressed else 0) | 0x40] * 4


def test_ranges_of_the_coordinates(shim):
    """coordinates 0, 1, p - 1 and (p - 1) / 2, (p + 1) / 2 (the boundary of the flag) as words: the same bytes as the host (the encoder takes
    any reduced words, on the curve or not)"""
    vals = [0, 1, 2, P - 1, (P - 1) // 2, (P + 1) // 2, P - 2]
    rows1 = [np.concatenate([U.fp_abi(x), U.fp_abi(y)]) for x in vals for y in vals if x or y]
    check(shim, ca.G1, np.stack(rows1), None)
    rnd = random.Random(5)
    rows2 = [np.concatenate([U.fp_abi(rnd.choice(vals)) for _ in range(4)]) for _ in range(60)]
    rows2 = [r for r in rows2 if r.any()]
    check(shim, ca.G2, np.stack(rows2), None)


def test_new_symbols_exported_and_declared():
    L = lib()
    decl = open(HEADER).read()
    for s in NEW:
        assert s in SYMBOLS and hasattr(L, s) and getattr(L, s).restype is not None
        assert re.search(r"\bint32_t %s\(" % s, decl), s


def test_argument_checks_then_no_device():
    """DGPU_E_BADARG for NULL arguments, unknown handles or ranges before the device check; n = 0 is DGPU_OK; without a device n >= 1 is
    DGPU_E_NODEVICE for the encoders (never a host result).  Without a device no handle exists, so every handle call is DGPU_E_BADARG."""
    L = lib()
    if L.dgpu_device_count() > 0:
        pytest.skip("checks the no-device behaviour")
    out = np.zeros(192, np.uint8)
    inf = np.zeros(1, np.uint8)
    for fn, G in ((L.dgpu_g1_serialize_device, O.G1), (L.dgpu_g2_serialize_device, O.G2)):
        g = np.ascontiguousarray(G.generator()[None, :])
        assert fn(None, None, 1, 1, p_(out)) == -3
        assert fn(p_(g), None, 1, 1, None) == -3
        assert fn(p_(g), None, 1 << 31, 1, p_(out)) == -3
        assert fn(None, None, 0, 1, None) == 0
        assert fn(p_(g), None, 1, 1, p_(out)) == -1
        assert fn(p_(g), p_(inf), 1, 0, p_(out)) == -1
    xy = np.zeros(24, np.uint64)
    for rd in (L.dgpu_bases_read_g1, L.dgpu_bases_read_g2):
        assert rd(12345, 0, 1, p_(xy), p_(inf)) == -3
        assert rd(12345, 0, 1, None, None) == -3
        assert rd(0, 0, 0, None, None) == -3
    for se in (L.dgpu_bases_serialize_g1, L.dgpu_bases_serialize_g2):
        assert se(12345, 0, 1, 1, p_(out)) == -3
        assert se(12345, 0, 1, 0, None) == -3
    with pytest.raises(ca.DockGpuError):
        serde.serialize_device(ca.G1, O.G1.generator()[None, :])
