"""CPU: the per-lane routines of BBS+ proofs of knowledge in bulk (crypto_amd/csrc/bbs_pok_kernels.hip.h: pok_value, pok_row_entry, pok_own_scalar, pok_col_run,
pok_col_term, pok_weights, fq_neg_words, g1_is_negation, pok_status) compiled for the host with the FP29_CHECK operand asserts
(tests/native/bbs_pok_dev_host_shim.cpp) and driven as k_bbs_pok_rows, k_bbs_pok_own, k_bbs_pok_col_sums, k_col_finish and the chunks of dock_bbs.hip drive
them, against the big-integer model of tests/bbs_pok_model.py: both input forms, the values 0, 1, r - 1, r and 2^256 - 1, rows of L + 2 = 3, 31, 32, 33 entries, the
masks all-hidden, all-revealed, only first, only last, alternating and differing per row, row counts on both sides of a lane's run, a wave, a block and a forced
chunk, the batching scalars 1, 2 and r - 1.  (The model itself is checked against the oracle in tests/test_bbs_pok_model.py.)  A green run
shows the values are right and that no product leaves fr_mul's operand contract."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import bbs_pok_model as PM
from bbs_model import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "bbs_pok_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libbbs_pok_dev_host_shim.so")
R2 = pow(2, 256, R)
TOP = (1 << 256) - 1
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
MASKS = ["hidden", "revealed", "first", "last", "alternating", "per_row"]
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC, os.path.join(HERE, "native", "col_frame_host.hpp")] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "col_sums.hip.h", "bbs_routines.hip.h", "bbs_pok_kernels.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz = C.c_void_p, C.c_size_t
    L.shim_pok_rows.argtypes = [vp, vp, vp, vp, C.c_int, sz, sz, vp, vp]
    L.shim_pok_columns.argtypes = [vp, vp, vp, vp, vp, C.c_int, sz, sz, sz, sz, vp, vp, vp, vp]
    L.shim_fq_neg.argtypes = [vp, vp]
    L.shim_is_negation.argtypes = [vp, C.c_int, vp, C.c_int]
    L.shim_status.argtypes = [C.c_int] * 4
    L.shim_pok_rows.restype = L.shim_pok_columns.restype = L.shim_fq_neg.restype = None
    L.shim_is_negation.restype = L.shim_status.restype = C.c_int
    return L


def words(vals, k=8):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for v in vals for i in range(k)], dtype=np.uint32)


def ints(w, k=8):
    return [sum(int(x) << (32 * i) for i, x in enumerate(row)) for row in w.reshape(-1, k)]


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def form(vals, mont):
    return words([v * R2 % R for v in vals] if mont else vals)


def mask_row(kind, i, L):
    return {"hidden": [0] * L, "revealed": [1] * L, "first": [1] + [0] * (L - 1), "last": [0] * (L - 1) + [1], "alternating": [j & 1 for j in range(L)],
            "per_row": [(i >> (j % 5)) & 1 for j in range(L)]}[kind]


def scenario(rows, L, seed, mont, kind):
    """`rows` proofs' scalars (the points play no part here) with the edge values spread over them: 0, 1, r - 1 in both forms, r and 2^256 - 1 as canonical words.
    The proofs hold the values as given (the model reduces what it reads); raw: what the kernels are handed"""
    rng = np.random.default_rng(seed)
    raw = [dict(c=rand(rng, 1)[0], fixed=rand(rng, 4), values=rand(rng, L), mask=mask_row(kind, i, L)) for i in range(rows)]
    edges = [0, 1, R - 1] + ([] if mont else [R, TOP])
    for k, v in enumerate(edges):
        raw[k % rows]["c"] = v
        raw[(k + 1) % rows]["fixed"][k % 4] = v
        raw[(k + 2) % rows]["values"][k % L] = v
        raw[rows - 1]["values"][(L - 1 - k) % L] = v
    return raw, [PM.Proof([0] * 5, q["fixed"], q["values"], q["mask"], q["c"]) for q in raw]


def arrays(raw, mont):
    return (form([q["c"] for q in raw], mont), form([z for q in raw for z in q["fixed"]], mont), form([v for q in raw for v in q["values"]], mont),
            np.array([m for q in raw for m in q["mask"]], dtype=np.uint8) * 3)      # (any non-zero byte means revealed)


def launcher_run():
    hdr = open(os.path.join(CSRC, "col_launch.hip.h")).read()
    return int(re.search(r"\bCOL_RUN = (\d+)\b", hdr).group(1))


def test_the_constants_are_the_launchers():
    assert launcher_run() == 16
    src = open(os.path.join(CSRC, "k_bbs_pok.hip")).read()
    assert "colk::col_blocks(rows)" in src and "colk::COL_RUN" in src and "dim3(256)" in src      # a block is 256 lanes of COL_RUN rows each: what the shim drives
    assert "256 * COL_RUN" in open(os.path.join(CSRC, "k_cols.hip")).read()


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("n", [3, 31, 32, 33])
def test_rows_and_own_point_scalars(shim, n, mont):
    """k_bbs_pok_rows and k_bbs_pok_own: canonical words below r of (c, z4, y ..) and of (z1, z2, -c, c, -1 | z3, -1), every mask, c = 0 among the rows"""
    L = n - 2
    for kind in MASKS:
        for rows in (1, 63, 64, 65):
            raw, proofs = scenario(rows, L, 100 * n + rows, mont, kind)
            out, own = np.zeros(8 * rows * n, np.uint32), np.zeros(8 * rows * 7, np.uint32)
            shim.shim_pok_rows(*map(p_, arrays(raw, mont)), mont, rows, L, p_(out), p_(own))
            want = [v for p in proofs for v in p.row()]
            assert ints(out) == want and max(want) < R, (kind, rows)
            assert ints(own) == [v for p in proofs for v in p.own()], (kind, rows)


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("rho", [1, 2, R - 1])
def test_batch_columns_and_weights(shim, rho, mont):
    """k_bbs_pok_col_sums / k_col_finish: C_k, the five weights over the own points, rho^i and -rho^i for row counts on both sides of a lane's run (16), of a
    wave (64), of a block (256 x 16), in one chunk and in chunks that end inside a run, at a run's end and past a block"""
    run = launcher_run()
    shapes = ((1, 3, (1,), "revealed"), (2, 3, (2, 1), "hidden"), (15, 32, (15, 7), "first"), (17, 31, (17, 16), "last"), (63, 31, (63, 16), "per_row"),
              (64, 32, (64, 17), "alternating"), (65, 33, (65, 64), "per_row"), (257, 3, (257, 100), "per_row"), (256 * run + 1, 3, (256 * run + 1, 256 * run), "per_row"),
              (256 * run - 1, 3, (256 * run - 1,), "per_row"))
    for rows, n, chunks, kind in shapes:
        L = n - 2
        raw, proofs = scenario(rows, L, 7 * rows + n, mont, kind)
        c, w5, tp, tn = PM.batch(None, proofs, rho)
        assert tp[-1] == pow(rho, rows - 1, R)
        for chunk in chunks:
            oc, ow, op, on = np.zeros(8 * n, np.uint32), np.zeros(40 * rows, np.uint32), np.zeros(8 * rows, np.uint32), np.zeros(8 * rows, np.uint32)
            shim.shim_pok_columns(*map(p_, arrays(raw, mont)), p_(form([rho], mont)), mont, rows, L, chunk, run, p_(oc), p_(ow), p_(op), p_(on))
            assert ints(oc) == c, (rows, n, chunk)
            assert ints(ow) == [w for r in w5 for w in r], (rows, n, chunk)
            assert ints(op) == tp and ints(on) == tn, (rows, n, chunk)


def test_base_field_words(shim):
    """-y = p - y (zero stays zero), Q == -P on affine words with identity flags, and the order of the four verdicts"""
    rng = np.random.default_rng(11)
    ys = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, (1 << 380) + 12345, 0xFFFFFFFF, 1 << 32, (1 << 352) - 1] + [int.from_bytes(rng.bytes(60), "little") % P for _ in range(20)]
    for y in ys:
        out = np.zeros(12, np.uint32)
        shim.shim_fq_neg(p_(words([y], 12)), p_(out))
        assert ints(out, 12) == [(P - y) % P], hex(y)
    x, y = ys[-1], ys[-2]
    pt = lambda a, b: words([a, b], 12)
    for (a, ai, b, bi), want in [((pt(x, y), 0, pt(x, P - y), 0), 1), ((pt(x, y), 0, pt(x, y), 0), 0), ((pt(x, y), 0, pt(x ^ 1, P - y), 0), 0),
                                 ((pt(x, y), 0, pt(x, (P - y) ^ (1 << 380)), 0), 0), ((pt(x, y), 0, pt(x, P - y + 1), 0), 0), ((pt(0, 0), 1, pt(0, 0), 1), 1),
                                 ((pt(x, y), 0, pt(0, 0), 1), 0), ((pt(0, 0), 1, pt(x, P - y), 0), 0), ((pt(x, 1), 0, pt(x, P - 1), 0), 1),
                                 ((pt(x, 0xFFFFFFFF), 0, pt(x, P - 0xFFFFFFFF), 0), 1), ((pt(x ^ (1 << 64), y), 0, pt(x, P - y), 0), 0)]:
        assert shim.shim_is_negation(p_(a), ai, p_(b), bi) == want
    for bits in range(16):
        a_inf, first, second, pairing = [(bits >> k) & 1 for k in range(4)]
        want = 1 if a_inf else 2 if not first else 3 if not second else 4 if not pairing else 0
        assert shim.shim_status(a_inf, first, second, pairing) == want
