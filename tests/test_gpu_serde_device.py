"""GPU: point decoding and validation on the device (dgpu_g*_deserialize_device, dgpu_bases_upload_g*_serialized, dgpu_g*_validate_batch) against the
host forms of dock_serde.cpp, the big-integer model and the MSM pipeline: the same words and flags byte for byte, the same refusals with the lowest
refused index, resident bases from bytes that behave like dgpu_bases_upload_*, and a refused key that leaves nothing on the device."""
import ctypes as C
import numpy as np
import pytest
import bls12_381_model as M
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd import serde
from crypto_amd._native import lib, DockGpuError
from crypto_amd.fixed_base import WindowTable

pytestmark = pytest.mark.gpu
SZ = {("g1", True): 48, ("g1", False): 96, ("g2", True): 96, ("g2", False): 192}


@pytest.fixture(scope="module", autouse=True)
def dev():
    ca.init(0)


def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def group(tag):
    return (ca.G1, O.G1) if tag == "g1" else (ca.G2, O.G2)


def points(G, n, seed):
    pts = G.gen_seq(O.rand_scalars(seed, 1)[0], O.rand_scalars(seed + 1, 1)[0], n, threads=16) if n else np.zeros((0, 12 if G is O.G1 else 24), np.uint64)
    inf = np.zeros(n, np.uint8)
    inf[::37] = 1                                                    # identities mixed in
    return np.ascontiguousarray(pts), inf


def host(curve, data, mode, n):
    xy, inf = np.zeros((n, curve.AW), np.uint64), np.zeros(n, np.uint8)
    fn = lib().dgpu_g1_deserialize if curve.tag == "g1" else lib().dgpu_g2_deserialize
    buf = np.frombuffer(bytes(data), np.uint8)
    return fn(p_(buf), n, mode, p_(xy), p_(inf)), xy, inf


def device(curve, data, mode, n):
    xy, inf, bad = np.zeros((n, curve.AW), np.uint64), np.zeros(n, np.uint8), C.c_size_t(12345)
    fn = lib().dgpu_g1_deserialize_device if curve.tag == "g1" else lib().dgpu_g2_deserialize_device
    buf = np.frombuffer(bytes(data), np.uint8)
    return fn(p_(buf), n, mode, p_(xy), p_(inf), C.byref(bad)), xy, inf, bad.value


@pytest.mark.parametrize("tag", ["g1", "g2"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, (1 << 16) + 3])
def test_same_words_as_the_host(tag, n):
    curve, G = group(tag)
    pts, inf = points(G, n, 11 + n)
    for compressed in (True, False):
        data = serde.serialize(curve, pts, inf, compressed)
        for mode in (int(compressed), int(compressed) | 2):
            hrc, hxy, hinf = host(curve, data, mode, n)
            drc, dxy, dinf, bad = device(curve, data, mode, n)
            assert hrc == 0 and drc == 0 and bad == n, (tag, n, mode, drc, bad)
            assert dxy.tobytes() == hxy.tobytes() and dinf.tobytes() == hinf.tobytes(), (tag, n, mode)


def malformed(curve, good_rec, compressed):
    """one record of each refused class (bytes of one point)"""
    sz = SZ[(curve.tag, compressed)]
    P = M.P
    recs = {}
    recs["flag"] = bytes([good_rec[0] ^ 0x80]) + good_rec[1:]
    recs["x>=p"] = bytes([(0x80 if compressed else 0) | P.to_bytes(48, "big")[0]]) + P.to_bytes(48, "big")[1:] + good_rec[48:]
    recs["inf_payload"] = bytes([(0x80 if compressed else 0) | 0x40]) + bytes(sz - 2) + b"\x01"
    recs["inf_largest"] = bytes([(0x80 if compressed else 0) | 0x60]) + bytes(sz - 1)
    if not compressed:
        recs["largest"] = bytes([good_rec[0] | 0x20]) + good_rec[1:]
        recs["off_curve"] = good_rec[:-1] + bytes([good_rec[-1] ^ 1])
    elif curve.tag == "g1":
        x = next(x for x in range(1, 60) if U.g1_lift(x) is None)
        recs["no_root"] = bytes([0x80]) + x.to_bytes(48, "big")[1:]
    else:
        a = next(a for a in range(60) if U.g2_lift((a, 1)) is None)
        recs["no_root"] = bytes([0x80]) + (1).to_bytes(48, "big")[1:] + a.to_bytes(48, "big")
    off = U.off_subgroup_points()
    op = U.g1_abi(off["S"][0])[0] if curve.tag == "g1" else U.g2_abi(off["S2"][0])[0]
    recs["off_subgroup"] = serde.serialize(curve, op[None, :], None, compressed)
    return recs


@pytest.mark.parametrize("tag", ["g1", "g2"])
@pytest.mark.parametrize("compressed", [True, False])
def test_refusals_report_the_lowest_index(tag, compressed):
    curve, G = group(tag)
    n = 300
    pts, inf = points(G, n, 5)
    data = bytearray(serde.serialize(curve, pts, inf, compressed))
    sz = SZ[(tag, compressed)]
    mode = int(compressed)
    for name, rec in malformed(curve, bytes(data[sz:2 * sz]), compressed).items():
        for ks in ([0], [199], [n - 1], [250, 77]):
            bad = bytearray(data)
            for k in ks:
                bad[k * sz:(k + 1) * sz] = rec
            hrc, _, _ = host(curve, bad, mode, n)
            drc, _, _, first = device(curve, bad, mode, n)
            assert hrc == -3 and drc == -3 and first == min(ks), (name, ks, drc, first)
            with pytest.raises(DockGpuError) as e:
                serde.deserialize_device(curve, bytes(bad), compressed)
            assert e.value.index == min(ks)
        if name == "off_subgroup":                                  # Validate::No accepts it, with the host's words
            bad = bytearray(data); bad[199 * sz:200 * sz] = rec
            hrc, hxy, hinf = host(curve, bad, mode | 2, n)
            drc, dxy, dinf, first = device(curve, bad, mode | 2, n)
            assert hrc == 0 and drc == 0 and first == n and dxy.tobytes() == hxy.tobytes() and dinf.tobytes() == hinf.tobytes()


@pytest.mark.parametrize("tag,n", [("g1", 1 << 20), ("g2", 1 << 18)])
def test_full_size_from_fixed_base(tag, n):
    """a proving-key-sized batch made on the device, serialised on the host, decoded on the device: the original words"""
    curve, G = group(tag)
    sc = [int(x) for x in np.random.default_rng(n).integers(1, 1 << 62, n)]
    with WindowTable(curve, G.generator()) as t:
        pts, inf = t.multiply_many(sc)
    for compressed in (True, False):
        data = serde.serialize(curve, pts, inf, compressed)
        got, ginf = serde.deserialize_device(curve, data, compressed)
        assert (got == pts).all() and (ginf == inf).all()


@pytest.mark.parametrize("tag", ["g1", "g2"])
@pytest.mark.parametrize("n", [5000, 1 << 15])
def test_resident_bases_from_bytes(tag, n):
    curve, G = group(tag)
    pts, inf = points(G, n, 21)
    pts[inf != 0] = 0
    sc = O.rand_scalars(23, n)
    data = serde.serialize(curve, pts, inf, True)
    ref = ca.DeviceBases(curve, pts, inf)
    db = ca.DeviceBases.from_serialized(curve, data)
    ln = C.c_size_t(0)
    assert lib().dgpu_handle_len(db.handle, C.byref(ln)) == 0 and ln.value == n
    want = ref.msm_bigint(sc)
    assert (db.msm_bigint(sc) == want).all()
    if n <= 5000:
        ga, gi = G.to_affine(want)
        ra, ri = G.to_affine(G.msm(pts, sc, inf, threads=16))
        assert gi == ri and (ga == ra).all()
    db.precompute()
    assert (db.msm_bigint(sc) == want).all()
    # the optional decoded words of the C call
    xy, finf, h, bad = np.zeros((n, curve.AW), np.uint64), np.zeros(n, np.uint8), C.c_uint64(0), C.c_size_t(0)
    buf = np.frombuffer(data, np.uint8)
    fn = lib().dgpu_bases_upload_g1_serialized if tag == "g1" else lib().dgpu_bases_upload_g2_serialized
    assert fn(p_(buf), n, 1, p_(xy), p_(finf), C.byref(h), C.byref(bad)) == 0 and bad.value == n
    assert (xy == pts).all() and (finf == inf).all()
    lib().dgpu_bases_free(h.value)
    ref.free(); db.free()


@pytest.mark.parametrize("tag", ["g1", "g2"])
def test_refused_key_leaves_nothing(tag):
    import torch
    curve, G = group(tag)
    n = 4097
    pts, inf = points(G, n, 31)
    data = bytearray(serde.serialize(curve, pts, inf, True))
    sz = SZ[(tag, True)]
    rec = malformed(curve, bytes(data[sz:2 * sz]), True)["off_subgroup"]
    bad = bytearray(data); bad[1000 * sz:1001 * sz] = rec
    ca.DeviceBases.from_serialized(curve, bytes(data)).free()      # (the workspace has grown to this size)
    torch.cuda.synchronize()
    a0, f0 = lib().dgpu_device_alloc_count(), torch.cuda.mem_get_info()[0]
    h, first = C.c_uint64(0), C.c_size_t(0)
    buf = np.frombuffer(bytes(bad), np.uint8)
    fn = lib().dgpu_bases_upload_g1_serialized if tag == "g1" else lib().dgpu_bases_upload_g2_serialized
    assert fn(p_(buf), n, 1, None, None, C.byref(h), C.byref(first)) == -3 and first.value == 1000 and h.value == 0
    with pytest.raises(DockGpuError) as e:
        ca.DeviceBases.from_serialized(curve, bytes(bad))
    assert e.value.index == 1000
    assert lib().dgpu_device_alloc_count() == a0 and torch.cuda.mem_get_info()[0] == f0


@pytest.mark.parametrize("tag", ["g1", "g2"])
def test_validate_batch_matches_the_model(tag):
    curve, G = group(tag)
    off = U.off_subgroup_points()
    names, mul, abi = (("S", "-S", "T", "S11"), M.g1_mul, U.g1_abi) if tag == "g1" else (("T2", "S2"), M.g2_mul, U.g2_abi)
    good, _ = points(G, 200, 41)
    rows, want, inf = list(good), [True] * 200, [0] * 200
    for k in names:
        rows.append(abi(off[k][0])[0]); want.append(mul(off[k][0], M.R) is None); inf.append(0)
    offc = good[3].copy(); offc[-6:] = U.fp_abi((U.fp_int(offc[-6:]) + 1) % M.P); rows.append(offc); want.append(False); inf.append(0)
    unr = good[4].copy(); v = O.limbs_to_int(unr[:6]) + M.P
    if v < 2 ** 384:
        unr[:6] = O.int_to_limbs(v, 6); rows.append(unr); want.append(False); inf.append(0)
    rows.append(np.zeros(curve.AW, np.uint64)); want.append(True); inf.append(0)
    rows.append(offc.copy()); want.append(True); inf.append(1)
    pts = np.ascontiguousarray(np.stack(rows), np.uint64)
    got = serde.validate(curve, pts, np.array(inf, np.uint8))
    assert got.tolist() == want
    assert serde.validate(curve, good).all()
