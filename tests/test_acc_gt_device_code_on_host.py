"""CPU: the per-lane routines of the accumulator proofs with a GT commitment in bulk (crypto_amd/csrc/acc_gt_kernels.hip.h: own_scalar, col_run, col_term,
row_weights, seg_end, stage_src, first_failure) compiled for the host with the FP29_CHECK operand asserts (tests/native/acc_gt_dev_host_shim.cpp) and driven as
k_acc_gt_own, k_acc_gt_stage, k_acc_gt_sides, k_acc_gt_verdict, k_acc_gt_col_sums, k_col_finish and the chunks of dock_acc_gt.hip drive them, against the
big-integer model of tests/acc_gt_model.py: both proof kinds, both input forms, the values 0, 1, r - 1, r and 2^256 - 1 in every response and challenge
position, row counts on both sides of a lane's run (15, 16, 17), a wave (63, 64, 65), a block (4095, 4096, 4097) and forced chunks, the batching scalars 1, 2
and r - 1, and the verdict on every flag combination.  (The model itself is checked against the oracle in tests/test_acc_gt_model.py.)  A green run shows the
values are right and that no product leaves fr_mul's operand contract."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import acc_gt_model as GM
from acc_gt_model import MEM, NM
from bbs_model import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "acc_gt_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libacc_gt_dev_host_shim.so")
R2 = pow(2, 256, R)
TOP = (1 << 256) - 1
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC, os.path.join(HERE, "native", "col_frame_host.hpp")] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "col_sums.hip.h", "acc_gt_kernels.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz = C.c_void_p, C.c_size_t
    L.shim_acc_gt_shape.argtypes = [C.c_int, vp]
    L.shim_acc_gt_own.argtypes = [vp, vp, C.c_int, C.c_int, sz, vp]
    L.shim_acc_gt_stage.argtypes = [vp, vp, C.c_int, sz, vp]
    L.shim_acc_gt_sides.argtypes = [vp, vp, C.c_int, sz, vp, vp, vp]
    L.shim_acc_gt_verdict.argtypes = [vp, vp, vp, C.c_int, sz, vp]
    L.shim_acc_gt_columns.argtypes = [vp, vp, vp, C.c_int, C.c_int, sz, sz, sz, vp, vp, vp, vp, vp]
    for f in ("shape", "own", "stage", "sides", "verdict", "columns"):
        getattr(L, "shim_acc_gt_" + f).restype = None
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
    """`rows` proofs' scalars (the points play no part here) with the edge values in every response and challenge position: 0, 1, r - 1 in both forms, r and
    2^256 - 1 as canonical words.  raw: what the kernels are handed; the proofs hold the same values (the model reduces what it reads)"""
    rng = np.random.default_rng(seed)
    nr = GM.NRESP[kind]
    raw = [dict(c=rand(rng, 1)[0], resp=rand(rng, nr)) for _ in range(rows)]
    edges = [0, 1, R - 1] + ([] if mont else [R, TOP])
    for k, v in enumerate(edges):
        raw[k % rows]["c"] = v
        for q in range(nr):
            raw[(k + 1 + q) % rows]["resp"][q] = v
        raw[rows - 1]["resp"][k % nr] = v
    if rows >= 4:
        raw[rows - 2] = dict(c=edges[-1], resp=[edges[-1]] * nr)         # a whole row of the largest edge value, one of zeros
        raw[rows - 3] = dict(c=0, resp=[0] * nr)
    return raw, [GM.Proof(kind, [0] * GM.NPTS[kind], 0, q["resp"], q["c"]) for q in raw]


def arrays(raw, mont):
    return form([q["c"] for q in raw], mont), form([z for q in raw for z in q["resp"]], mont)


def launcher_run():
    hdr = open(os.path.join(CSRC, "col_launch.hip.h")).read()
    return int(re.search(r"\bCOL_RUN = (\d+)\b", hdr).group(1))


def test_the_constants_are_the_launchers_and_the_models(shim):
    assert launcher_run() == 16
    src = open(os.path.join(CSRC, "k_acc_gt.hip")).read()
    assert "colk::col_blocks(rows)" in src and "colk::COL_RUN" in src and "dim3(256)" in src      # a block is 256 lanes of COL_RUN rows each: what the shim drives
    assert "(size_t)shape_of(in.kind).g1cols, n, run_sums" in src                                 # the columns that are negated when they are finished: the sides'
    hdr = open(os.path.join(CSRC, "acc_gt_launch.hip.h")).read()
    assert "ACC_GT_EACH_CHUNK = 4096, ACC_GT_BATCH_CHUNK = 16384" in hdr and "UNMEASURED" in hdr
    for kind in (MEM, NM):
        out = np.zeros(16, np.int32)
        shim.shim_acc_gt_shape(kind, p_(out))
        pts, resp, own, segs, checks, g1cols, pcols = out[:7].tolist()
        assert (pts, resp, checks) == (GM.NPTS[kind], GM.NRESP[kind], GM.CHECKS[kind])
        assert out[7:7 + segs].tolist() == GM.SEG_ENDS[kind] and own == GM.SEG_ENDS[kind][-1] and segs == checks + 2
        assert g1cols + pcols + 1 == (5 if kind == MEM else 8)


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("kind", [MEM, NM])
def test_own_scalars(shim, kind, mont):
    """k_acc_gt_own: canonical words below r of the 17, respectively 27, own scalars of every row; every edge value in every position among the rows"""
    no = GM.SEG_ENDS[kind][-1]
    for rows in (1, 2, 15, 16, 17, 63, 64, 65, 257):
        raw, proofs = scenario(kind, rows, 100 * rows + kind, mont)
        own = np.zeros(8 * rows * no, np.uint32)
        shim.shim_acc_gt_own(*map(p_, arrays(raw, mont)), kind, mont, rows, p_(own))
        want = [v for p in proofs for v in p.own()]
        assert ints(own) == want and max(want) < R, rows


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("rho", [1, 2, R - 1])
@pytest.mark.parametrize("kind", [MEM, NM])
def test_batch_columns_and_weights(shim, kind, rho, mont):
    """k_acc_gt_col_sums / k_col_finish: the columns' coefficients, the weights over the own points, t s_y, t c and t for row counts on both sides of a lane's
    run (16), of a wave (64), of a block (256 x 16), in one chunk and in forced chunks that end inside a run, at a run's end and past a block"""
    run = launcher_run()
    assert 256 * run == 4096
    shapes = ((1, (1,)), (2, (2, 1)), (15, (15, 7)), (16, (16, 15)), (17, (17, 16)), (63, (63, 16)), (64, (64, 17)), (65, (65, 64, 63)), (257, (257, 100)),
              (4095, (4095,)), (4096, (4096, 4095)), (4097, (4097, 4096, 65)))
    if rho != 2:
        shapes = shapes[:9] + shapes[11:]
    np_ = GM.NPTS[kind]
    for rows, chunks in shapes:
        raw, proofs = scenario(kind, rows, 7 * rows + kind, mont)
        s, w, wp, wq, tp = GM.batch(proofs, rho)
        assert tp[-1] == pow(rho, rows - 1, R)
        for chunk in chunks:
            oc, ow = np.zeros(8 * len(s), np.uint32), np.zeros(8 * np_ * rows, np.uint32)
            op, oq, ot = (np.zeros(8 * rows, np.uint32) for _ in range(3))
            shim.shim_acc_gt_columns(*map(p_, arrays(raw, mont)), p_(form([rho], mont)), kind, mont, rows, chunk, run, p_(oc), p_(ow), p_(op), p_(oq), p_(ot))
            assert ints(oc) == s, (rows, chunk)
            assert ints(ow) == [x for r in w for x in r], (rows, chunk)
            assert ints(op) == wp and ints(oq) == wq and ints(ot) == tp, (rows, chunk)


@pytest.mark.parametrize("kind", [MEM, NM])
def test_staging_lays_out_the_bases_of_every_segment(shim, kind):
    """k_acc_gt_stage's routine: every base of a row is the point the model's layout names, shared points copied into every row, identities (zero words) at every
    position among the rows"""
    rng = np.random.default_rng(77 + kind)
    npts, no = GM.NPTS[kind], GM.SEG_ENDS[kind][-1]
    rows = 65
    pt = lambda: [int.from_bytes(rng.bytes(60), "little") % P for _ in range(2)]
    points = [[pt() for _ in range(npts)] for _ in range(rows)]
    for k in range(npts):
        points[3 + k][k] = [0, 0]
    points[21] = [[0, 0]] * npts
    V, X, Y, Z, K, Pp = shared = [pt() for _ in range(6)]
    pw = words([c for row in points for q in row for c in q], 12)
    sw = words([c for q in shared for c in q], 12)
    bases = np.zeros(rows * no * 24, np.uint32)
    shim.shim_acc_gt_stage(p_(pw), p_(sw), kind, rows, p_(bases))
    # the model lays out logs: hand it one distinct number per point and read the layout back
    tags = {"v": 1000, "x": 1001, "yk": 1002, "z": 1003, "k": 1004, "pi": 1005}
    by_tag = {1000: V, 1001: X, 1002: Y, 1003: Z, 1004: K, 1005: Pp}
    key = GM.Key(0, 0, 0, 0, 0, 0, 0)
    layout = GM.Proof(kind, list(range(npts)), 0, [0] * GM.NRESP[kind], 0).bases(key, **tags)
    want = [by_tag[t] if t >= 1000 else row[t] for row in points for t in layout]
    got = [list(x) for x in zip(*[iter(ints(bases, 12))] * 2)]
    assert got == want


@pytest.mark.parametrize("kind", [MEM, NM])
def test_sides_and_verdict_on_every_flag_combination(shim, kind):
    """k_acc_gt_sides: the last two sums of a row become pa = q and pb = p, zero words and a skip flag where the sum is the identity.  k_acc_gt_verdict: the
    first Schnorr sum that is not the identity, else the pairing value against the row's own R_E — one differing word anywhere refuses"""
    rng = np.random.default_rng(3 + kind)
    segs, J = GM.CHECKS[kind] + 2, GM.CHECKS[kind]
    rows = 1 << (J + 1)
    inf = np.array([[(i >> j) & 1 for j in range(J)] + [(i >> J) & 1, (i >> 1) & 1] for i in range(rows)], np.uint8)
    sums = rng.integers(1, 1 << 32, size=(rows, segs, 36), dtype=np.uint32)
    pa, pb, skip = np.zeros((rows, 24), np.uint32), np.zeros((rows, 24), np.uint32), np.full(2 * rows, 9, np.uint8)
    shim.shim_acc_gt_sides(p_(sums), p_(inf), kind, rows, p_(pa), p_(pb), p_(skip))
    for i in range(rows):
        pz, qz = bool(inf[i, segs - 2]), bool(inf[i, segs - 1])
        assert (pa[i] == (0 if qz else sums[i, segs - 1, :24])).all() and (pb[i] == (0 if pz else sums[i, segs - 2, :24])).all()
        assert (skip[i], skip[rows + i]) == (int(qz), int(pz))
    gt = rng.integers(0, 1 << 32, size=(rows, 144), dtype=np.uint32)
    for differ in (None, 0, 77, 143):
        r_e = gt.copy()
        if differ is not None:
            r_e[:, differ] ^= 1 << (differ % 32)
        status = np.full(rows, 99, np.uint8)
        shim.shim_acc_gt_verdict(p_(inf), p_(gt), p_(r_e), kind, rows, p_(status))
        for i in range(rows):
            bad = [j for j in range(J) if not inf[i, j]]
            assert status[i] == (bad[0] + 1 if bad else 0 if differ is None else J + 1), (i, differ)
