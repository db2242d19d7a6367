"""CPU: the DEVICE point decoding / validation routines (crypto_amd/csrc/serde_kernels.hip.h) compiled for the host with the FP29_CHECK bound
tracker (tests/native/serde_dev_host_shim.cpp), checked point by point against the host deserialisers (dock_serde.cpp) and the big-integer model
([r]P == O as the independent subgroup verdict).  A green run shows the decoding is right and its lazy-limb arithmetic cannot overflow.  Also the
C ABI of the device forms without a device: exported, DGPU_E_BADARG for bad arguments first, then DGPU_E_NODEVICE."""
import ctypes as C
import os
import random
import subprocess
import numpy as np
import pytest
import bls12_381_model as M
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd import serde
from crypto_amd._native import lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "serde_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libserde_dev_host_shim.so")
P, R = M.P, M.R
SZ = {("g1", True): 48, ("g1", False): 96, ("g2", True): 96, ("g2", False): 192}
NEW = ["dgpu_g1_deserialize_device", "dgpu_g2_deserialize_device", "dgpu_bases_upload_g1_serialized", "dgpu_bases_upload_g2_serialized",
       "dgpu_g1_validate_batch", "dgpu_g2_validate_batch"]


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(HERE, "..", "crypto_amd", "csrc", f) for f in ("serde_kernels.hip.h", "fp29.hip.h", "fp2_29.hip.h", "ec29.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    return C.CDLL(SO)


def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def nfp(curve):
    return 1 if curve.tag == "g1" else 2


def dev_decode(shim, curve, data, mode):
    """the device routine on every record: (ok, words, is_inf) per point"""
    sz = SZ[(curve.tag, bool(mode & 1))]
    n = len(data) // sz
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    xy, inf, ok = np.zeros((n, curve.AW), np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    shim.shim_decode(nfp(curve), p_(buf), n, mode, p_(xy), p_(inf), p_(ok))
    return ok.astype(bool), xy, inf


def host_decode(curve, data, mode):
    """dgpu_g*_deserialize one point at a time: the host verdict of every point"""
    sz = SZ[(curve.tag, bool(mode & 1))]
    fn = lib().dgpu_g1_deserialize if curve.tag == "g1" else lib().dgpu_g2_deserialize
    n = len(data) // sz
    oks, xy, inf = np.zeros(n, bool), np.zeros((n, curve.AW), np.uint64), np.zeros(n, np.uint8)
    for i in range(n):
        b = np.frombuffer(bytes(data[i * sz:(i + 1) * sz]), np.uint8).copy()
        w, f = np.zeros(curve.AW, np.uint64), np.zeros(1, np.uint8)
        rc = fn(p_(b), 1, mode, p_(w), p_(f))
        assert rc in (0, -3)
        oks[i] = rc == 0
        if rc == 0:
            xy[i], inf[i] = w, f[0]
    return oks, xy, inf


def check_same(shim, curve, data, modes):
    for mode in modes:
        dok, dxy, dinf = dev_decode(shim, curve, data, mode)
        hok, hxy, hinf = host_decode(curve, data, mode)
        assert (dok == hok).all(), (curve.tag, mode, np.nonzero(dok != hok)[0])
        assert (dxy[hok] == hxy[hok]).all() and (dinf[hok] == hinf[hok]).all(), (curve.tag, mode)
        yield mode, hok


def encode(curve, pts, inf=None, compressed=True):
    return serde.serialize(curve, np.asarray(pts, np.uint64).reshape(-1, curve.AW), inf, compressed)


def be48(v):
    return v.to_bytes(48, "big")


def test_generator_multiples_and_random_points(shim):
    for curve, G in ((ca.G1, O.G1), (ca.G2, O.G2)):
        pts = G.gen_seq(O.rand_scalars(5, 1)[0], O.rand_scalars(6, 1)[0], 40, threads=4)
        pts = np.concatenate([pts, G.gen_seq(1, 1, 6, threads=1)])          # G, 2G, ..., 6G
        inf = np.zeros(len(pts), np.uint8); inf[[3, 17]] = 1
        for compressed in (True, False):
            data = encode(curve, pts, inf, compressed)
            for mode, ok in check_same(shim, curve, data, (int(compressed), int(compressed) | 2)):
                assert ok.all()
            dok, dxy, dinf = dev_decode(shim, curve, data, int(compressed))
            live = inf == 0
            assert (dxy[live] == pts[live]).all() and (dinf == inf).all() and not dxy[~live].any()


def test_points_outside_the_subgroups(shim):
    """on the curve / twist, outside G1 / G2 (the order-3 points with x = 0 among them): refused with validation, accepted without, as on the host;
    the verdict is also the model's [r]P == O"""
    off = U.off_subgroup_points()
    for curve, names, mul in ((ca.G1, ("S", "-S", "T", "S11"), M.g1_mul), (ca.G2, ("T2", "S2"), M.g2_mul)):
        abi = U.g1_abi if curve is ca.G1 else U.g2_abi
        pts = np.stack([abi(off[k][0])[0] for k in names])
        for k in names:
            assert mul(off[k][0], R) is not None
        for compressed in (True, False):
            data = encode(curve, pts, None, compressed)
            res = dict(check_same(shim, curve, data, (int(compressed), int(compressed) | 2)))
            assert not res[int(compressed)].any() and res[int(compressed) | 2].all()
            dok, dxy, _ = dev_decode(shim, curve, data, int(compressed) | 2)
            assert (dxy == pts).all()


def test_malformed_encodings(shim):
    """x without a root, x >= p, every flag combination, canonical and non-canonical infinity, a y >= p: the same verdict as the host"""
    random.seed(7)
    g1 = O.G1.gen_seq(3, 5, 4, threads=1)
    recs = []
    xs_noroot = [x for x in range(1, 60) if U.g1_lift(x) is None][:4]
    for x in xs_noroot:
        recs.append(bytes([0x80 | be48(x)[0]]) + be48(x)[1:])
    for x in (P, P + 1, 2 ** 381 - 1, P - 1):
        b = be48(x); recs.append(bytes([0x80 | b[0]]) + b[1:])
    base = encode(ca.G1, g1[:1], None, True)
    for flags in range(8):
        recs.append(bytes([(base[0] & 0x1f) | (flags << 5)]) + base[1:])
    recs.append(bytes([0xc0]) + bytes(47))                                   # canonical infinity
    recs.append(bytes([0xe0]) + bytes(47))                                   # with "largest"
    recs.append(bytes([0xc0]) + bytes(46) + b"\x01")                         # with a payload bit
    recs.append(bytes([0xc1]) + bytes(47))
    data = b"".join(recs)
    res = dict(check_same(shim, ca.G1, data, (1, 3)))
    assert res[1].any() and not res[1].all()
    # uncompressed: flags, y >= p, a y off the curve
    un = encode(ca.G1, g1[:2], None, False)
    recs = [un[:96], un[96:]]
    for flags in range(8):
        recs.append(bytes([(un[0] & 0x1f) | (flags << 5)]) + un[1:96])
    recs.append(un[:48] + be48(P))
    recs.append(un[:48] + be48(U.fp_int(g1[0][6:]) ^ 1))
    recs.append(bytes([0x40]) + bytes(95)); recs.append(bytes([0x40]) + bytes(94) + b"\x01")
    res = dict(check_same(shim, ca.G1, b"".join(recs), (0, 2)))
    assert res[0][:2].all()
    # G2: the same classes; c1 and c0 >= p each
    g2 = O.G2.gen_seq(3, 5, 2, threads=1)
    c2 = encode(ca.G2, g2, None, True)
    recs = [c2[:96], c2[96:]]
    for flags in range(8):
        recs.append(bytes([(c2[0] & 0x1f) | (flags << 5)]) + c2[1:96])
    b = be48(P); recs.append(bytes([0x80 | b[0]]) + b[1:] + c2[48:96])
    recs.append(c2[:48] + be48(P))
    for a in range(12):
        x = (a, 1)
        if U.g2_lift(x) is None:
            recs.append(bytes([0x80]) + be48(1)[1:] + be48(a))
    recs.append(bytes([0xc0]) + bytes(95)); recs.append(bytes([0xc0]) + bytes(94) + b"\x02")
    res = dict(check_same(shim, ca.G2, b"".join(recs), (1, 3)))
    assert res[1][:2].all() and not res[1].all()
    u2 = encode(ca.G2, g2, None, False)
    recs = [u2[:192], u2[192:], u2[:144] + be48(P), u2[:96] + be48(P) + u2[144:192], bytes([0x20 | u2[0]]) + u2[1:192]]
    res = dict(check_same(shim, ca.G2, b"".join(recs), (0, 2)))
    assert res[0][:2].all() and not res[0][2:].any()


def test_fq2_roots_with_c1_zero(shim):
    """the Fq2 square root on c1 = 0 (the branch of sqrt(a0) and sqrt(-a0) u), on zero, and on a non-square; the G2 sign order (c1 first) is covered
    by the points above, whose y has c1 != 0, and here by decoding both signs of a point whose y has c1 = 0 if one turns up"""
    random.seed(3)
    out = np.zeros(24, np.uint64)
    for a0 in [0, 1, 4, P - 1, P - 4] + [random.randrange(P) for _ in range(20)]:
        a = (a0, 0)
        A = np.concatenate([U.fp_abi(a0), U.fp_abi(0)])
        ok = shim.shim_fq2_sqrt(p_(A), p_(out))
        r = (U.fp_int(out[:6]), U.fp_int(out[6:]))
        assert ok == 1 and M.f2_sqr(r) == a
    nonsq = next(((a, 1) for a in range(2, 200) if U.fp2_sqrt((a, 1)) is None))
    A = np.concatenate([U.fp_abi(nonsq[0]), U.fp_abi(nonsq[1])])
    assert shim.shim_fq2_sqrt(p_(A), p_(out)) == 0
    for a in [random.randrange(P) for _ in range(20)]:
        A = U.fp_abi(a)
        ok = shim.shim_fq_sqrt(p_(A), p_(out[:6]))
        assert bool(ok) == (U.fp_sqrt(a) is not None)
        if ok:
            assert U.fp_int(out[:6]) ** 2 % P == a


def test_validate_words(shim):
    """Validate::Yes of ABI words: subgroup points, outside the subgroups, off the curve, unreduced limbs, identities — against the model"""
    off = U.off_subgroup_points()
    for curve, G, names, mul, on in ((ca.G1, O.G1, ("S", "-S", "T", "S11"), M.g1_mul, M.g1_on_curve), (ca.G2, O.G2, ("T2", "S2"), M.g2_mul, M.g2_on_curve)):
        abi = U.g1_abi if curve is ca.G1 else U.g2_abi
        good = G.gen_seq(9, 11, 5, threads=1)
        rows, want, inf = list(good), [True] * 5, [0] * 5
        for k in names:
            rows.append(abi(off[k][0])[0]); want.append(mul(off[k][0], R) is None); inf.append(0)
        bad = good[0].copy(); bad[-6:] = U.fp_abi((U.fp_int(bad[-6:]) + 1) % P); rows.append(bad); want.append(False); inf.append(0)
        unr = good[1].copy(); v = O.limbs_to_int(unr[:6]) + P
        if v < 2 ** 384:
            unr[:6] = O.int_to_limbs(v, 6); rows.append(unr); want.append(False); inf.append(0)
        rows.append(np.zeros(curve.AW, np.uint64)); want.append(True); inf.append(0)
        rows.append(bad.copy()); want.append(True); inf.append(1)                 # the flag wins, as in the ABI
        pts = np.ascontiguousarray(np.stack(rows), np.uint64)
        ok = np.zeros(len(pts), np.uint8)
        shim.shim_validate(nfp(curve), p_(pts), p_(np.array(inf, np.uint8)), len(pts), p_(ok))
        assert ok.astype(bool).tolist() == want, curve.tag


def test_new_symbols_exported_and_bind():
    L = lib()
    for s in NEW:
        assert hasattr(L, s) and getattr(L, s).restype is not None


def test_argument_checks_then_no_device():
    """DGPU_E_BADARG for NULL / inconsistent arguments before the device check; n = 0 is DGPU_OK; without a device n >= 1 is DGPU_E_NODEVICE"""
    L = lib()
    if L.dgpu_device_count() > 0:
        pytest.skip("checks the no-device behaviour")
    data = np.frombuffer(encode(ca.G1, O.G1.generator()[None, :]), np.uint8).copy()
    data2 = np.frombuffer(encode(ca.G2, O.G2.generator()[None, :]), np.uint8).copy()
    xy, inf, ok = np.zeros(24, np.uint64), np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    bad, h = C.c_size_t(7), C.c_uint64(0)
    for dev, d in ((L.dgpu_g1_deserialize_device, data), (L.dgpu_g2_deserialize_device, data2)):
        assert dev(None, 1, 1, p_(xy), p_(inf), C.byref(bad)) == -3
        assert dev(p_(d), 1, 1, None, p_(inf), C.byref(bad)) == -3
        assert dev(p_(d), 1, 1, p_(xy), None, None) == -3
        assert dev(p_(d), 1 << 31, 1, p_(xy), p_(inf), None) == -3
        assert dev(None, 0, 1, None, None, C.byref(bad)) == 0 and bad.value == 0
        assert dev(p_(d), 1, 1, p_(xy), p_(inf), C.byref(bad)) == -1
    for up, d in ((L.dgpu_bases_upload_g1_serialized, data), (L.dgpu_bases_upload_g2_serialized, data2)):
        assert up(p_(d), 1, 1, None, None, None, None) == -3
        assert up(None, 1, 1, None, None, C.byref(h), None) == -3
        assert up(p_(d), 1, 1, None, None, C.byref(h), C.byref(bad)) == -1
        assert up(p_(d), 0, 1, None, None, C.byref(h), None) == L.dgpu_bases_upload_g1(None, None, 0, C.byref(h))
    for val in (L.dgpu_g1_validate_batch, L.dgpu_g2_validate_batch):
        assert val(None, None, 1, p_(ok)) == -3
        assert val(p_(xy), None, 1, None) == -3
        assert val(None, None, 0, None) == 0
        assert val(p_(xy), None, 1, p_(ok)) == -1
    with pytest.raises(ca.DockGpuError):
        serde.deserialize_device(ca.G1, data.tobytes())
    with pytest.raises(ca.DockGpuError):
        serde.validate(ca.G1, O.G1.generator()[None, :])
