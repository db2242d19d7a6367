"""CPU: the per-lane routines of accumulator proofs in bulk (crypto_amd/csrc/acc_pok_kernels.hip.h: own_scalar, col_run, col_term, row_weights, fq_neg_words,
stage_src, mem_status, nm_status) compiled for the host with the FP29_CHECK operand asserts (tests/native/acc_pok_dev_host_shim.cpp) and driven as k_acc_pok_own,
k_acc_pok_stage, k_acc_pok_col_sums, k_col_finish and the chunks of dock_acc_pok.hip drive them, against the big-integer model of tests/acc_pok_model.py:
both proof kinds, both input forms, the values 0, 1, r - 1, r and 2^256 - 1, row counts on both sides of a lane's run (15, 16, 17), a wave (63, 64, 65), a block
(4095, 4096, 4097) and a forced chunk, the batching scalars 1, 2 and r - 1, the y-flip, and the status routines on every flag combination.  (The model itself
is checked against the oracle in tests/test_acc_pok_model.py.)  A green run shows the values are right and that no product leaves fr_mul's operand contract."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import acc_pok_model as AM
from bbs_model import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "acc_pok_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libacc_pok_dev_host_shim.so")
R2 = pow(2, 256, R)
TOP = (1 << 256) - 1
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
SHAPE = {0: dict(pts=3, resp=2, own=4), 1: dict(pts=5, resp=3, own=8)}
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC, os.path.join(HERE, "native", "col_frame_host.hpp")] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "col_sums.hip.h", "bbs_routines.hip.h", "acc_pok_kernels.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz = C.c_void_p, C.c_size_t
    L.shim_acc_pok_own.argtypes = [vp, vp, C.c_int, C.c_int, sz, vp]
    L.shim_acc_pok_stage.argtypes = [vp, vp, C.c_int, sz, vp, vp, vp, vp]
    L.shim_acc_pok_columns.argtypes = [vp, vp, vp, C.c_int, C.c_int, sz, sz, sz, vp, vp, vp, vp]
    L.shim_acc_fq_neg.argtypes = [vp, vp]
    L.shim_mem_status.argtypes = [C.c_int] * 3
    L.shim_nm_status.argtypes = [C.c_int] * 5
    L.shim_acc_pok_own.restype = L.shim_acc_pok_stage.restype = L.shim_acc_pok_columns.restype = L.shim_acc_fq_neg.restype = None
    L.shim_mem_status.restype = L.shim_nm_status.restype = C.c_int
    return L


def words(vals, k=8):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for v in vals for i in range(k)], dtype=np.uint32)


def ints(w, k=8):
    a = w.reshape(-1, k).astype(object)
    return [sum(int(x) << (32 * i) for i, x in enumerate(row)) for row in a]


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def form(vals, mont):
    return words([v * R2 % R for v in vals] if mont else vals)


def scenario(kind, rows, seed, mont):
    """`rows` proofs' scalars (the points play no part here) with the edge values spread over them: 0, 1, r - 1 in both forms, r and 2^256 - 1 as canonical
    words.  raw: what the kernels are handed; the proofs hold the same values (the model reduces what it reads)"""
    rng = np.random.default_rng(seed)
    nr = SHAPE[kind]["resp"]
    raw = [dict(c=rand(rng, 1)[0], resp=rand(rng, nr)) for _ in range(rows)]
    edges = [0, 1, R - 1] + ([] if mont else [R, TOP])
    for k, v in enumerate(edges):
        raw[k % rows]["c"] = v
        for q in range(nr):
            raw[(k + 1 + q) % rows]["resp"][q] = v
        raw[rows - 1]["resp"][k % nr] = v
    return raw, [AM.Proof(kind, [0] * SHAPE[kind]["pts"], q["resp"], q["c"]) for q in raw]


def arrays(raw, mont):
    return form([q["c"] for q in raw], mont), form([z for q in raw for z in q["resp"]], mont)


def launcher_run():
    hdr = open(os.path.join(CSRC, "col_launch.hip.h")).read()
    return int(re.search(r"\bCOL_RUN = (\d+)\b", hdr).group(1))


def test_the_constants_are_the_launchers():
    assert launcher_run() == 16
    src = open(os.path.join(CSRC, "k_acc_pok.hip")).read()
    assert "colk::col_blocks(rows)" in src and "colk::COL_RUN" in src and "dim3(256)" in src      # a block is 256 lanes of COL_RUN rows each: what the shim drives
    assert "in.kind == MEMBERSHIP ? 0 : 1, in.kind == MEMBERSHIP ? 0 : 2" in src                                                       # the column that is negated when it is finished: P's
    hdr = open(os.path.join(CSRC, "acc_pok_launch.hip.h")).read()
    assert "ACC_POK_EACH_CHUNK = 4096, ACC_POK_BATCH_CHUNK = 65536" in hdr


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("kind", [0, 1])
def test_own_scalars(shim, kind, mont):
    """k_acc_pok_own: canonical words below r of (z1, -z2, -c, -1), respectively (s_d, -c, -1 | s_r, -s_y, -s_d, -c, -1); c = 0 and every edge value among the rows"""
    no = SHAPE[kind]["own"]
    for rows in (1, 2, 15, 16, 17, 63, 64, 65, 257):
        raw, proofs = scenario(kind, rows, 100 * rows + kind, mont)
        own = np.zeros(8 * rows * no, np.uint32)
        shim.shim_acc_pok_own(*map(p_, arrays(raw, mont)), kind, mont, rows, p_(own))
        want = [v for p in proofs for v in p.own()]
        assert ints(own) == want and max(want) < R, rows


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("rho", [1, 2, R - 1])
@pytest.mark.parametrize("kind", [0, 1])
def test_batch_columns_and_weights(shim, kind, rho, mont):
    """k_acc_pok_col_sums / k_col_finish: the shared points' coefficients, the weights over the own points, rho^i and -rho^i for row counts on both sides
    of a lane's run (16), of a wave (64), of a block (256 x 16), in one chunk and in chunks that end inside a run, at a run's end and past a block"""
    run = launcher_run()
    assert 256 * run == 4096
    shapes = ((1, (1,)), (2, (2, 1)), (15, (15, 7)), (16, (16,)), (17, (17, 16)), (63, (63, 16)), (64, (64, 17)), (65, (65, 64)), (257, (257, 100)),
              (4095, (4095,)), (4096, (4096, 4095)), (4097, (4097, 4096, 65)))
    np_ = SHAPE[kind]["pts"]
    for rows, chunks in shapes:
        raw, proofs = scenario(kind, rows, 7 * rows + kind, mont)
        s, w, tp, tn = AM.batch(proofs, rho)
        assert tp[-1] == pow(rho, rows - 1, R)
        for chunk in chunks:
            oc, ow, op, on = np.zeros(8 * len(s), np.uint32), np.zeros(8 * np_ * rows, np.uint32), np.zeros(8 * rows, np.uint32), np.zeros(8 * rows, np.uint32)
            shim.shim_acc_pok_columns(*map(p_, arrays(raw, mont)), p_(form([rho], mont)), kind, mont, rows, chunk, run, p_(oc), p_(ow), p_(op), p_(on))
            assert ints(oc) == s, (rows, chunk)
            assert ints(ow) == [x for r in w for x in r], (rows, chunk)
            assert ints(op) == tp and ints(on) == tn, (rows, chunk)


@pytest.mark.parametrize("kind", [0, 1])
def test_staging_lays_out_bases_sides_and_flags(shim, kind):
    """k_acc_pok_stage's routine: every slot takes the point the layout names ([V, A', Abar, T], respectively [Q, J, T2 | V, C', P, Cbar, T1]), the pairing's
    sides are the proof's first point and minus its second, and the flags mark zero words — identities at every position among the rows"""
    rng = np.random.default_rng(77 + kind)
    npts, no = SHAPE[kind]["pts"], SHAPE[kind]["own"]
    rows = 65
    pt = lambda: [int.from_bytes(rng.bytes(60), "little") % P for _ in range(2)]
    points = [[pt() for _ in range(npts)] for _ in range(rows)]
    for k in range(npts):
        points[3 + k][k] = [0, 0]                                        # one identity at every position
    points[20][0] = points[20][1] = [0, 0]
    points[21] = [[0, 0]] * npts
    points[22][1][1] = 1                                                  # y = 1 flips to p - 1
    shared = [pt() for _ in range(3)]
    pw = words([c for row in points for q in row for c in q], 12)
    sw = words([c for q in shared for c in q], 12)
    own, pa, pb, skip = np.zeros(rows * no * 24, np.uint32), np.zeros(rows * 24, np.uint32), np.zeros(rows * 24, np.uint32), np.full(3 * rows, 9, np.uint8)
    shim.shim_acc_pok_stage(p_(pw), p_(sw), kind, rows, p_(own), p_(pa), p_(pb), p_(skip))
    V, Pp, Q = shared
    want_own, want_a, want_b = [], [], []
    for row in points:
        want_own += [V, row[0], row[1], row[2]] if kind == 0 else [Q, row[2], row[4], V, row[0], Pp, row[1], row[3]]
        want_a.append(row[0])
        want_b.append([row[1][0], (P - row[1][1]) % P])
    got = lambda a: [list(x) for x in zip(*[iter(ints(a, 12))] * 2)]
    assert got(own) == want_own and got(pa) == want_a and got(pb) == want_b
    zero = lambda q: 1 if q == [0, 0] else 0
    assert skip[:rows].tolist() == [zero(r[0]) for r in points] and skip[rows:2 * rows].tolist() == [zero(r[1]) for r in points]
    assert skip[2 * rows:].tolist() == [zero(r[2]) if kind == 1 else 0 for r in points]
    assert sum(skip[:rows]) == 3 and sum(skip[rows:2 * rows]) == 3


def test_base_field_words_and_statuses(shim):
    """-y = p - y (zero stays zero), and the order of the checks on every flag combination"""
    rng = np.random.default_rng(11)
    ys = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, (1 << 380) + 12345, 0xFFFFFFFF, 1 << 32, (1 << 352) - 1] + [int.from_bytes(rng.bytes(60), "little") % P for _ in range(20)]
    for y in ys:
        out = np.zeros(12, np.uint32)
        shim.shim_acc_fq_neg(p_(words([y], 12)), p_(out))
        assert ints(out, 12) == [(P - y) % P], hex(y)
    for bits in range(8):
        a_inf, schnorr, pairing = [(bits >> k) & 1 for k in range(3)]
        assert shim.shim_mem_status(a_inf, schnorr, pairing) == (1 if a_inf else 2 if not schnorr else 3 if not pairing else 0)
    for bits in range(32):
        c_inf, j_inf, short, long_, pairing = [(bits >> k) & 1 for k in range(5)]
        want = 1 if c_inf else 2 if j_inf else 3 if not short else 4 if not long_ else 5 if not pairing else 0
        assert shim.shim_nm_status(c_inf, j_inf, short, long_, pairing) == want
