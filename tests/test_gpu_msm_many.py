"""GPU (-m gpu): dgpu_msm_g*_handle_many — many small MSMs over one resident base set in one call (crypto_amd/csrc/many_kernels.hip.h: the tree of the
small path over a chunk of rows, short rows packed several to a block, then Horner + normalisation per row on the device).  Bar: bit-exact.  EVERY row of
every case equals the single call dgpu_msm_*_handle on that row; rows also equal the CPU oracle (all of them up to 2^14 terms per case, otherwise at
least eight: the first, the last and the two either side of each chunk boundary).  Shapes cover every packing boundary of the segmented tree (2 n groups
rounded up to a power of two: n = 1, 2, 3, 7 / 8, 15 / 16, 17 .. 32), the 128-terms-per-block boundary and the several-blocks-per-row form; the digit and
point edge cases of test_gpu_small_msm.py sit inside batches beside ordinary rows."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd._native import lib
from test_gpu_msm import normalised

pytestmark = pytest.mark.gpu
CUR = {"G1": (ca.G1, O.G1), "G2": (ca.G2, O.G2)}
R = U.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 600, 4096, 8192)
MS = (1, 2, 3, 16, 17, 64, 257)
CAP = {"G1": 1 << 18, "G2": 1 << 16}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)
    lib().dgpu_set_min_gpu_n(1)
    yield
    lib().dgpu_set_small_msm_max(8192)
    lib().dgpu_set_min_gpu_n(0)


_BASES = {}


def big_bases(gname):
    """8192 bases per curve, generated once (the shape sweep uses prefixes of one handle)"""
    if gname not in _BASES:
        _BASES[gname] = U.seq_bases(CUR[gname][1], 8192, 5100 + len(gname), threads=16)[0]
    return _BASES[gname]


def chunk_rows(n):
    """the library's rows per launch (include/dock_gpu.h)"""
    return min(4096, max(1, (1 << 17) // max(n, 1)))


def oracle_rows(m, n, chunk=None):
    """rows compared against the CPU oracle: all of them up to 2^14 terms, otherwise at least 8 including the first, the last and both sides of each chunk boundary"""
    if m * n <= (1 << 14):
        return list(range(m))
    c = chunk or chunk_rows(n)
    rows = {0, m - 1}
    for b in range(c, m, c):
        rows |= {b - 1, b}
    k = 0
    while len(rows) < min(8, m):
        rows.add((k * 2654435761 + 7) % m); k += 1
    return sorted(rows)


def check_batch(gname, db, bases, sc, offset=0, inf=None, montgomery=False, canon=None, chunk=None, what=""):
    """many == every single call == the oracle on oracle_rows; returns the many-call's rows.  canon: the canonical scalars when sc is in Montgomery form"""
    curve, G = CUR[gname]
    m, n = sc.shape[:2]
    got, flags = db.msm_many(sc, offset=offset, montgomery=montgomery, flags=True)
    assert got.shape == (m, curve.JW)
    for j in range(m):
        one = db.msm_bigint(np.ascontiguousarray(sc[j]), offset=offset, montgomery=montgomery)
        assert (got[j] == one).all(), (what, gname, m, n, j)
        assert flags[j] == (0 if got[j][G.AW:].any() else 1), (what, gname, m, n, j)
    plain = sc if canon is None else canon
    for j in oracle_rows(m, n, chunk):
        b = bases[offset:offset + n]
        fl = np.zeros(n, np.uint8) if inf is None else inf[offset:offset + n].copy()
        fl |= (~b.any(axis=1)).astype(np.uint8)
        assert (got[j] == normalised(G, G.msm(b, np.ascontiguousarray(plain[j]), fl, threads=16))).all(), (what, gname, m, n, j)
    return got


@pytest.mark.parametrize("gname,n", [(g, n) for g in ("G1", "G2") for n in NS])
def test_shapes(gname, n):
    curve, G = CUR[gname]
    bases = big_bases(gname)
    db = ca.DeviceBases(curve, bases)
    for m in MS:
        if m * n > CAP[gname]:
            continue
        sc = O.rand_scalars(9000 + 131 * n + m, m * n).reshape(m, n, 4)
        check_batch(gname, db, bases, sc)
    db.free()


@pytest.mark.parametrize("m,n", [(4096, 24), (2, 8192)])
def test_large_g1_cases(m, n):
    curve, G = CUR["G1"]
    bases = big_bases("G1")
    db = ca.DeviceBases(curve, bases)
    sc = O.rand_scalars(77000 + m, m * n).reshape(m, n, 4)
    check_batch("G1", db, bases, sc)
    db.free()


def _negated(G, bases):
    """P_i = -P_{i-1} for odd i"""
    neg = bases.copy(); h = G.AW // 2
    for i in range(1, len(bases), 2):
        neg[i] = bases[i - 1]
        for k in range(h // 6):
            y = U.fp_int(neg[i][h + 6 * k:h + 6 * k + 6]); neg[i][h + 6 * k:h + 6 * k + 6] = U.fp_abi((U.P - y) % U.P)
    return neg


@pytest.mark.parametrize("gname", ["G1", "G2"])
@pytest.mark.parametrize("n", [6, 24, 150])
def test_row_edge_cases_beside_ordinary_rows(gname, n):
    """one batch whose rows mix: all-zero scalars (identity row), r - 1 everywhere, the extreme-nibble scalars, all scalars of a row equal, ordinary rows"""
    curve, G = CUR[gname]
    bases, _, _ = U.seq_bases(G, n + 3, 310 + n, threads=16)
    lim = lambda v: O.int_to_limbs(v, 4)
    nib = lambda d: int(("%x" % d) * 63, 16) % (1 << 255)
    m = 23
    sc = O.rand_scalars(320 + n, m * n).reshape(m, n, 4)
    sc[1] = 0
    sc[4] = lim(R - 1)
    for k, d in enumerate((7, 8, 0xF, 9, 1)):
        sc[6][k::5] = lim(nib(d))
    sc[7] = lim(nib(8))
    sc[9] = sc[9][0]
    sc[11][::2] = 0; sc[11][1::3] = lim(1)
    sc[m - 1] = 0
    pats = [0, 1, R - 1, nib(8) + 1, nib(8) - 1, nib(7), (1 << 255) - 1, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 128, (1 << 192) - 1, 1 << 192, 0x8 << 60, 0x9 << 60]
    for k in range(n):
        sc[13][k] = lim(pats[k % len(pats)])
    db = ca.DeviceBases(curve, bases)
    got, flags = db.msm_many(sc, flags=True)
    assert flags[1] == 1 and flags[m - 1] == 1 and not got[1][G.AW:].any()
    check_batch(gname, db, bases, sc, what="digit edges")
    # offset > 0, &[Fr] rows, row_stride > n with garbage between the rows (bit 255 set in it: read as data it would refuse the call)
    check_batch(gname, db, bases, sc, offset=3, what="offset")
    mont = O.fr_to_mont(sc.reshape(-1, 4)).reshape(m, n, 4)
    check_batch(gname, db, bases, mont, offset=1, montgomery=True, canon=sc, what="montgomery")
    wide = np.full((m, n + 5, 4), np.uint64(0xffffffffffffffff), np.uint64)
    wide[:, :n] = sc
    strided = wide[:, :n]
    assert strided.strides[0] == 32 * (n + 5)
    assert (db.msm_many(strided, offset=2) == db.msm_many(sc, offset=2)).all()
    check_batch(gname, db, bases, strided, offset=2, what="row_stride")
    db.free()
    # a handle whose bases are all equal; P, -P pairs with equal scalars; identity bases (flag and zero words)
    same = np.tile(bases[2], (n, 1))
    db = ca.DeviceBases(curve, same); check_batch(gname, db, same, sc, what="equal bases"); db.free()
    neg = _negated(G, bases[:n])
    pair = sc.copy(); pair[:, 1::2] = pair[:, 0:n - (n % 2):2]
    db = ca.DeviceBases(curve, neg)
    got, flags = db.msm_many(pair, flags=True)
    if n % 2 == 0:
        assert flags.all()                                     # every row cancels
    check_batch(gname, db, neg, pair, what="P and -P"); db.free()
    inf = np.zeros(n, np.uint8); inf[::4] = 1; zb = bases[:n].copy(); zb[2::9] = 0
    db = ca.DeviceBases(curve, zb, inf); check_batch(gname, db, zb, sc, inf=inf, what="identity bases"); db.free()


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_refusals(gname):
    curve, G = CUR[gname]
    n, m = 20, 9
    bases, _, _ = U.seq_bases(G, n, 41, threads=16)
    db = ca.DeviceBases(curve, bases)
    fn = curve.fn("dgpu_msm_%s_handle_many")
    p = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)
    sc = O.rand_scalars(42, m * n).reshape(m, n, 4)
    out = np.zeros((m, curve.JW), np.uint64)
    bad = sc.copy(); bad[m - 1, n - 1, 3] |= np.uint64(1 << 63)           # one scalar with bit 255 set, in the last row
    assert fn(db.handle, 0, p(bad), n, n, m, 0, p(out), None) == -3
    assert fn(db.handle, 0, p(sc), n, n, m, 0, p(out), None) == 0         # the refused call left nothing behind
    assert (out == db.msm_many(sc)).all()
    assert fn(db.handle, 0, p(sc), n - 1, n, m, 0, p(out), None) == -3    # row_stride < n
    assert fn(db.handle, 1, p(sc), n, n, m, 0, p(out), None) == -3        # offset + n beyond the handle
    assert fn(db.handle + 12345, 0, p(sc), n, n, m, 0, p(out), None) == -3
    assert fn(db.handle, 0, None, n, n, m, 0, p(out), None) == -3
    assert fn(db.handle, 0, p(sc), n, n, m, 0, None, None) == -3
    assert fn(db.handle, 0, None, 0, n, 0, 0, None, None) == 0            # m = 0
    try:
        lib().dgpu_set_min_gpu_n(256)                                      # the handle threshold is min(256, 8) terms — of the BATCH
        TOO_SMALL = fn(db.handle, 0, p(sc), n, 1, 7, 0, p(out), None)
        served = db.msm_many(O.rand_scalars(43, 300).reshape(300, 1, 4))   # m = 300, n = 1: device work
        one_by_eight = fn(db.handle, 0, p(sc), n, 1, 8, 0, p(out), None)
    finally:
        lib().dgpu_set_min_gpu_n(1)
    assert TOO_SMALL == -6 and one_by_eight == 0                            # DGPU_E_TOO_SMALL
    s1 = O.rand_scalars(43, 300)
    for j in (0, 1, 150, 299):
        assert (served[j] == db.msm_bigint(s1[j:j + 1])).all()
    db.free()


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_chunks(twin, gname):
    """rows per launch set to 5 through the development surface: m = 4, 5, 6, 11 give the same bytes as unchunked; rows beside each boundary meet the oracle"""
    curve, G = CUR[gname]
    lib().dgpu_set_min_gpu_n(1)
    for n in (3, 40, 300):
        bases, _, _ = U.seq_bases(G, n, 510 + n, threads=16)
        db = ca.DeviceBases(curve, bases)
        for m in (4, 5, 6, 11):
            sc = O.rand_scalars(520 + n + m, m * n).reshape(m, n, 4)
            whole = db.msm_many(sc)
            try:
                assert twin.dgpu_set_many_chunk_rows(5) == 0
                got = check_batch(gname, db, bases, sc, chunk=5, what="chunk 5")
            finally:
                twin.dgpu_set_many_chunk_rows(0)
            assert (got == whole).all(), (n, m)
        db.free()


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_fallback_handles(gname):
    """handles the new kernels do not serve run their rows through the single-row driver inside the call: a precomputed table, more than 8192 bases,
    the small path switched off"""
    curve, G = CUR[gname]
    N = 10000
    bases, _, _ = U.seq_bases(G, N, 61, threads=16)
    db = ca.DeviceBases(curve, bases)
    sc = O.rand_scalars(62, 3 * 9000).reshape(3, 9000, 4)
    got = db.msm_many(sc)
    for j in range(3):
        assert (got[j] == db.msm_bigint(sc[j])).all()
    assert (got[0] == normalised(G, G.msm(bases[:9000], sc[0], threads=16))).all()
    db.free()
    n = 1 << 15
    tb, _, _ = U.seq_bases(G, n, 63, threads=16)
    db = ca.DeviceBases(curve, tb).precompute(16)
    assert db.table_shape() is not None
    sc = O.rand_scalars(64, 4 * 100).reshape(4, 100, 4)
    got = db.msm_many(sc, offset=5)
    for j in range(4):
        assert (got[j] == db.msm_bigint(sc[j], offset=5)).all()
    assert (got[3] == normalised(G, G.msm(tb[5:105], sc[3], threads=16))).all()
    db.free()
    db = ca.DeviceBases(curve, bases[:500])
    sc = O.rand_scalars(65, 6 * 77).reshape(6, 77, 4)
    fast = check_batch(gname, db, bases[:500], sc)
    try:
        assert lib().dgpu_set_small_msm_max(0) == 0
        slow = db.msm_many(sc)
    finally:
        lib().dgpu_set_small_msm_max(8192)
    assert (fast == slow).all()
    db.free()


def test_concurrent_calls_on_one_handle():
    """four host threads issue many-calls of different shapes on one handle while a fifth issues single calls on it: all equal the serial results,
    and a second round of the same shapes allocates nothing"""
    G, curve = O.G1, ca.G1
    bases, _, _ = U.seq_bases(G, 2000, 81, threads=16)
    db = ca.DeviceBases(curve, bases)
    shapes = [(64, 24), (7, 600), (300, 1), (33, 129), (5, 2000), (128, 8), (17, 64), (40, 33)]
    jobs = [(O.rand_scalars(820 + k, m * n).reshape(m, n, 4), (k * 3) % 5) for k, (m, n) in enumerate(shapes)]
    jobs = [(s, off if s.shape[1] + off <= 2000 else 0) for s, off in jobs]
    singles = [O.rand_scalars(840 + k, 100 + 50 * k) for k in range(6)]
    want = [db.msm_many(s, offset=off) for s, off in jobs]
    want1 = [db.msm_bigint(s) for s in singles]

    def many_worker(t):
        return [(k, db.msm_many(jobs[k][0], offset=jobs[k][1])) for rep in range(2) for k in range(t, len(jobs), 4)]

    def single_worker():
        return [[db.msm_bigint(s) for s in singles] for _ in range(6)]

    # (the serial calls above were each shape's first: a call that grows its slot sizes the idle slots with it, so whichever slot a thread is handed below has seen the shape)
    a0 = ca.device_alloc_count()
    with ThreadPoolExecutor(5) as ex:
        for rnd in range(2):
            f1 = ex.submit(single_worker)
            fm = [ex.submit(many_worker, t) for t in range(4)]
            for f in fm:
                for k, got in f.result():
                    assert (got == want[k]).all(), (rnd, shapes[k])
            for rep in f1.result():
                assert all((g == w).all() for g, w in zip(rep, want1)), rnd
    assert ca.device_alloc_count() == a0
    db.free()


def test_python_wrapper_equals_c_abi():
    import ctypes as C
    for gname in ("G1", "G2"):
        curve, G = CUR[gname]
        bases, _, _ = U.seq_bases(G, 40, 91, threads=16)
        db = ca.DeviceBases(curve, bases)
        m, n = 12, 37
        sc = O.rand_scalars(92, m * n).reshape(m, n, 4)
        out = np.zeros((m, curve.JW), np.uint64); inf = np.ones(m, np.uint8)
        rc = curve.fn("dgpu_msm_%s_handle_many")(db.handle, 2, sc.ctypes.data_as(C.c_void_p), n, n, m, 0, out.ctypes.data_as(C.c_void_p), inf.ctypes.data_as(C.c_void_p))
        assert rc == 0 and not inf.any()
        got, flags = db.msm_many(sc, offset=2, flags=True)
        assert (got == out).all() and (flags == inf).all()
        db.free()


def test_cpp_wrapper_equals_c_abi():
    """include/dock_gpu.hpp DeviceBases<G>::msm_many against the C ABI and the single call (tests/native/msm_many_driver.cpp)"""
    exe = os.path.join(ROOT, "tests", "native", "msm_many_driver")
    src = exe + ".cpp"
    hdr = os.path.join(ROOT, "include", "dock_gpu.hpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                               "-L" + os.path.join(ROOT, "crypto_amd"), "-ldock_gpu", "-L" + os.path.join(ROOT, "oracle"), "-loracle",
                               "-Wl,-rpath," + os.path.join(ROOT, "crypto_amd") + ":" + os.path.join(ROOT, "oracle")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout
