"""GPU: point encoding on the device (dgpu_g*_serialize_device) and resident bases read back (dgpu_bases_read_g*, dgpu_bases_serialize_g*) against the
host encoders of dock_serde.cpp and the words the handles were made from: the same bytes at the sizes where the kernels' blocks and the staged
pieces change, round trips through dgpu_bases_upload_g*_serialized over plain handles, precomputed tables and sharded sets, the five queries of a
generated key (one of them against an encoder written here from the big-integer model), and refusals that leave nothing on the device."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import bls12_381_model as M
import lego_setup as LS
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd import serde, legogroth16 as LG
from crypto_amd._native import lib, DockGpuError
from crypto_amd.fixed_base import WindowTable

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SZ = {("g1", True): 48, ("g1", False): 96, ("g2", True): 96, ("g2", False): 192}


def stage_chunk_bytes():
    """STAGE_CHUNK_BYTES of msm_driver.hip.h: the piece the staged copies are cut to"""
    src = open(os.path.join(ROOT, "crypto_amd", "csrc", "msm_driver.hip.h")).read()
    m = re.search(r"constexpr size_t STAGE_CHUNK_BYTES = \(size_t\)(\d+) << (\d+);", src)
    assert m, "STAGE_CHUNK_BYTES not found"
    return int(m.group(1)) << int(m.group(2))


PIECE = stage_chunk_bytes()


@pytest.fixture(scope="module", autouse=True)
def dev():
    ca.init(0)


def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def group(tag):
    return (ca.G1, O.G1) if tag == "g1" else (ca.G2, O.G2)


def points(G, n, seed):
    pts = np.ascontiguousarray(G.gen_seq(O.rand_scalars(seed, 1)[0], O.rand_scalars(seed + 1, 1)[0], n, threads=16))
    inf = np.zeros(n, np.uint8)
    inf[::37] = 1                                                    # identities by flag (over non-zero words) ...
    pts[5::41] = 0                                                   # ... and by all-zero words
    return pts, inf


def model_bytes(curve, pts, inf, compressed):
    """the Zcash / arkworks encoding written from the big-integer model (not the library's encoder): big-endian coordinates, c1 before c0,
    flags 0x80 / 0x40 / 0x20 in byte 0; "largest" is y > (p - 1) / 2, on Fq2 by c1 unless it is zero"""
    k = 1 if curve.tag == "g1" else 2
    out = bytearray()
    half = (M.P - 1) // 2
    for row, f in zip(pts, inf):
        c = [U.fp_int(row[6 * j:6 * j + 6]) for j in range(2 * k)]           # x.c0 (x.c1) y.c0 (y.c1)
        if f or not row.any():
            rec = bytearray(SZ[(curve.tag, compressed)]); rec[0] = (0x80 if compressed else 0) | 0x40
            out += rec; continue
        x = c[:k][::-1]; y = c[k:][::-1]                                     # byte order: c1 first
        rec = b"".join(v.to_bytes(48, "big") for v in (x if compressed else x + y))
        rec = bytearray(rec)
        if compressed:
            hi = (y[0] > half) if (k == 1 or y[0] != 0) else (y[1] > half)
            rec[0] |= 0x80 | (0x20 if hi else 0)
        out += rec
    return bytes(out)


@pytest.mark.parametrize("tag", ["g1", "g2"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, (1 << 16) + 1])
def test_serialize_device_gives_the_host_bytes(tag, n):
    curve, G = group(tag)
    pts, inf = points(G, n, 100 + n)
    for compressed in (True, False):
        want = serde.serialize(curve, pts, inf, compressed)
        assert serde.serialize_device(curve, pts, inf, compressed) == want, (tag, n, compressed)
        assert serde.serialize_device(curve, pts, None, compressed) == serde.serialize(curve, pts, None, compressed), (tag, n, compressed)


@pytest.mark.parametrize("tag", ["g1", "g2"])
def test_serialize_device_one_point_past_a_whole_piece(tag):
    """n = STAGE_CHUNK_BYTES / (bytes per point) + 1: one whole piece and a piece of one point (the compressed form; the uncompressed one of the same
    points crosses more pieces)"""
    curve, G = group(tag)
    n = PIECE // SZ[(tag, True)] + 1
    pts, inf = points(G, n, 7)
    for compressed in (True, False):
        assert serde.serialize_device(curve, pts, inf, compressed) == serde.serialize(curve, pts, inf, compressed), (tag, compressed)


def check_handle(curve, db, pts, inf, data_c, data_u):
    """db holds pts (identities: inf or all-zero words): words, flags, both encodings, and sub-ranges equal to slices of the whole"""
    n = len(pts)
    ident = inf.astype(bool) | ~pts.any(axis=1)
    xy, fl = db.read()
    assert (fl.astype(bool) == ident).all() and not xy[ident].any() and (xy[~ident] == pts[~ident]).all()
    assert db.to_bytes(True) == data_c and db.to_bytes(False) == data_u
    for off, k in ((0, 1), (1, 64), (n // 3, n // 3 + 5), (n - 1, 1), (n - 65, 65), (n, 0), (17, 0)):
        sx, sf = db.read(off, k)
        assert (sx == xy[off:off + k]).all() and (sf == fl[off:off + k]).all(), (off, k)
        for comp, data in ((True, data_c), (False, data_u)):
            sz = SZ[(curve.tag, comp)]
            assert db.to_bytes(comp, off, k) == data[off * sz:(off + k) * sz], (off, k, comp)
    # words only / flags only
    w = np.zeros((n, curve.AW), np.uint64); f = np.zeros(n, np.uint8)
    L = lib()
    assert getattr(L, "dgpu_bases_read_%s" % curve.tag)(db.handle, 0, n, p_(w), None) == 0 and (w == xy).all()
    assert getattr(L, "dgpu_bases_read_%s" % curve.tag)(db.handle, 0, n, None, p_(f)) == 0 and (f == fl).all()


@pytest.mark.parametrize("tag", ["g1", "g2"])
def test_round_trip_plain_then_precomputed(tag):
    """bytes -> dgpu_bases_upload_*_serialized -> read / serialize: the same bytes and the decoded words; then the same handle as a precomputed table"""
    curve, G = group(tag)
    n = 5000
    pts, inf = points(G, n, 40)
    data_c, data_u = serde.serialize(curve, pts, inf, True), serde.serialize(curve, pts, inf, False)
    dec, dinf = serde.deserialize(curve, data_c, True)
    db = ca.DeviceBases.from_serialized(curve, data_c, True)
    assert db.table_shape() is None
    check_handle(curve, db, dec, dinf, data_c, data_u)
    db.precompute(16)
    assert db.table_shape() is not None
    check_handle(curve, db, dec, dinf, data_c, data_u)
    db.free()
    # words uploaded as they are (dgpu_bases_upload_*): identities by flag over non-zero words come back as zero words
    db = ca.DeviceBases(curve, pts, inf)
    check_handle(curve, db, pts, inf, data_c, data_u)
    db.free()


def test_sharded_sets_read_like_the_unsharded_handle():
    """dgpu_bases_upload_*_sharded over two contexts of the one GPU: every part read on its own context, results in global order, ranges across the
    parts' border; the same after the parts became tables"""
    ca.init_devices([0, 0])
    L = lib()
    try:
        assert L.dgpu_context_count() == 2
        for tag in ("g1", "g2"):
            curve, G = group(tag)
            n = 3001
            pts, inf = points(G, n, 60)
            data_c, data_u = serde.serialize(curve, pts, inf, True), serde.serialize(curve, pts, inf, False)
            sh = ca.ShardedDeviceBases(curve, pts, inf, ngpus=2)
            cnt = C.c_int32(0)
            assert L.dgpu_shard_count(sh.handle, C.byref(cnt)) == 0 and cnt.value == 2
            plain = ca.DeviceBases(curve, pts, inf)
            xy, fl = plain.read()
            sx, sf = sh.read()
            assert (sx == xy).all() and (sf == fl).all()
            check_handle(curve, sh, pts, inf, data_c, data_u)
            assert sh.to_bytes(True, n // 2 - 3, 7) == plain.to_bytes(True, n // 2 - 3, 7)
            sh.precompute(16)
            check_handle(curve, sh, pts, inf, data_c, data_u)
            sh.free(); plain.free()
    finally:
        L.dgpu_set_device(0)


def test_generated_key_queries_read_back():
    """dgpu_legogroth16_setup with the queries to the host: every handle reads back as query_xy / query_inf word for word and serializes as
    dgpu_g*_serialize of them; the a_query (a few thousand points) also against the model's encoder"""
    import test_gpu_setup as TS
    cs = LS.circuit(3000, x0=5)
    w, g1, g2 = TS.waste_and_generators(77)
    dr = TS.upload(cs)
    pk, _ = LG.generate_parameters_r1cs(dr, 2, *w, g1, g2, queries_to_host=True)
    for name, (xy, inf) in pk.host_queries.items():
        db = getattr(pk, name)
        curve = ca.G2 if name == "b_g2_query" else ca.G1
        assert db.n == len(xy), name
        rx, rf = db.read()
        assert (rx == xy).all() and (rf == inf).all(), name
        for comp in (True, False):
            assert db.to_bytes(comp) == serde.serialize(curve, xy, inf, comp), (name, comp)
    xy, inf = pk.host_queries["a_query"]
    assert len(xy) > 3000
    for comp in (True, False):
        assert pk.a_query.to_bytes(comp) == model_bytes(ca.G1, xy, inf, comp), comp
    TS.free_key(pk); dr.free()


def test_model_encoder_agrees_on_g2_flags():
    """the model's encoder against the device one on G2 points with y.c1 = 0 (twist points outside G2: the encoder never validates)"""
    import test_serde_encode_device_code_on_host as H
    pts = np.stack([U.g2_abi(pt)[0] for pt in H.twist_points_with_real_y(8, 9)])
    pts = np.concatenate([pts, H.neg_words(ca.G2, pts)])
    inf = np.zeros(len(pts), np.uint8)
    for comp in (True, False):
        got = serde.serialize_device(ca.G2, pts, None, comp)
        assert got == model_bytes(ca.G2, pts, inf, comp) == serde.serialize(ca.G2, pts, None, comp)
    db = ca.DeviceBases.from_serialized(ca.G2, serde.serialize(ca.G2, pts, None, True), True, validate=False)
    assert db.to_bytes(True) == model_bytes(ca.G2, pts, inf, True)
    db.free()


def test_refusals_keep_nothing():
    """window tables, scalars, freed / unknown handles, the other curve's handles, ranges past the end, missing outputs: DGPU_E_BADARG, and no
    device allocation by any of them; n = 0 on a valid handle is DGPU_OK"""
    L = lib()
    pts, inf = points(O.G1, 300, 90)
    pts2, inf2 = points(O.G2, 200, 91)
    g1 = ca.DeviceBases(ca.G1, pts, inf)
    g2 = ca.DeviceBases(ca.G2, pts2, inf2)
    tab = WindowTable(ca.G1, O.G1.generator())
    ds = ca.DeviceScalars(O.rand_scalars(5, 64))
    dead = ca.DeviceBases(ca.G1, pts[:50], inf[:50]); dead_h = dead.handle; dead.free()
    g1.read(); g1.to_bytes(); g2.read(); g2.to_bytes()                 # warm: the slots' workspaces exist
    xy, fl, out = np.zeros((400, 24), np.uint64), np.zeros(400, np.uint8), np.zeros(400 * 192, np.uint8)
    before = ca.device_alloc_count()
    R1, R2, S1, S2 = L.dgpu_bases_read_g1, L.dgpu_bases_read_g2, L.dgpu_bases_serialize_g1, L.dgpu_bases_serialize_g2
    for h in (tab.handle, ds.handle, dead_h, 0, 987654321):
        assert R1(h, 0, 1, p_(xy), p_(fl)) == -3 and S1(h, 0, 1, 1, p_(out)) == -3, h
        assert R2(h, 0, 1, p_(xy), p_(fl)) == -3 and S2(h, 0, 1, 0, p_(out)) == -3, h
    assert R1(g2.handle, 0, 1, p_(xy), p_(fl)) == -3 and S1(g2.handle, 0, 1, 1, p_(out)) == -3       # the other curve
    assert R2(g1.handle, 0, 1, p_(xy), p_(fl)) == -3 and S2(g1.handle, 0, 1, 1, p_(out)) == -3
    assert R1(g1.handle, 250, 51, p_(xy), p_(fl)) == -3 and S1(g1.handle, 301, 0, 1, p_(out)) == -3  # past the end
    assert R1(g1.handle, (1 << 64) - 1, 2, p_(xy), p_(fl)) == -3 and S2(g2.handle, 1, (1 << 64) - 1, 1, p_(out)) == -3
    assert R1(g1.handle, 0, 5, None, None) == -3 and S1(g1.handle, 0, 5, 1, None) == -3               # no output
    assert R1(g1.handle, 300, 0, None, None) == 0 and S2(g2.handle, 7, 0, 0, None) == 0              # n = 0
    assert L.dgpu_g1_serialize_device(None, None, 4, 1, p_(out)) == -3 and L.dgpu_g2_serialize_device(p_(pts2), None, 4, 1, None) == -3
    assert ca.device_alloc_count() == before
    with pytest.raises(DockGpuError):
        g1.read(299, 2)
    tab.free(); ds.free(); g1.free(); g2.free()
