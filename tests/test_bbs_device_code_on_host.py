"""CPU: the per-lane routines of BBS+ in bulk (crypto_amd/csrc/bbs_kernels.hip.h: row_value, row_entry, pow_start, col_run, tree_step, col_finish, neg_product)
compiled for the host with the FP29_CHECK operand asserts (tests/native/bbs_dev_host_shim.cpp) and driven as k_bbs_rows, k_bbs_col_sums, k_col_finish and the
chunks of dock_bbs.hip drive them, against the big-integer model of tests/bbs_model.py: both input forms, the values 0, 1, r - 1, r and 2^256 - 1, rows of
L + 2 = 3, 31, 32, 33 entries, row counts on both sides of a wave, a lane's run, a block and a chunk, the batching scalars 1, 2 and r - 1.  The host's batch
inversion of x + e (acc_host_tables.hpp issue_inverses with its zero flags) against the same model, share by share.  The model itself is checked once against the
oracle's group arithmetic.  A green run shows the values are right and that no product leaves fr_mul's operand contract."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import oracle_c as O
import bbs_model as BM
from bbs_model import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "bbs_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libbbs_dev_host_shim.so")
R2 = pow(2, 256, R)
TOP = (1 << 256) - 1
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC, os.path.join(HERE, "native", "col_frame_host.hpp")] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "col_sums.hip.h", "bbs_routines.hip.h", "bbs_kernels.hip.h", "acc_host_tables.hpp", "host_field.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-mbmi2", "-madx", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz = C.c_void_p, C.c_size_t
    L.shim_rows.argtypes = [vp, vp, vp, C.c_int, sz, sz, vp]
    L.shim_columns.argtypes = [vp, vp, vp, vp, C.c_int, sz, sz, sz, sz, vp, vp, vp]
    L.shim_inverses.argtypes = [vp, sz, vp, C.c_int, sz, vp, vp]
    L.shim_rows.restype = L.shim_columns.restype = None
    L.shim_inverses.restype = C.c_int
    return L


def words(vals):
    return np.array([(v >> (32 * k)) & 0xFFFFFFFF for v in vals for k in range(8)], dtype=np.uint32)


def ints(w):
    return [sum(int(x) << (32 * k) for k, x in enumerate(row)) for row in w.reshape(-1, 8)]


def limbs64(vals):
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in vals for k in range(4)], dtype=np.uint64)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def launcher_run():
    hdr = open(os.path.join(CSRC, "col_launch.hip.h")).read()
    return int(re.search(r"\bCOL_RUN = (\d+)\b", hdr).group(1))


def test_the_constants_are_the_launchers():
    assert launcher_run() == 16
    src = open(os.path.join(CSRC, "k_bbs.hip")).read()
    assert "colk::col_blocks(rows)" in src and "colk::COL_RUN" in src and "dim3(256)" in src and "256 * COL_RUN" in open(os.path.join(CSRC, "k_cols.hip")).read()      # a block is 256 lanes of COL_RUN rows each: what the shim drives


def scenario(rows, L, seed, mont):
    """(e, s, msgs) with the edge values spread over the rows: 0, 1, r - 1 in both forms, r and 2^256 - 1 as canonical words"""
    rng = np.random.default_rng(seed)
    e, s, msgs = rand(rng, rows), rand(rng, rows), [rand(rng, L) for _ in range(rows)]
    edges = [0, 1, R - 1] + ([] if mont else [R, TOP])
    for k, v in enumerate(edges):
        s[k % rows] = v
        msgs[(k + 1) % rows][k % L] = v
        msgs[rows - 1][(L - 1 - k) % L] = v
        e[(k + 2) % rows] = v
    return e, s, msgs


def form(vals, mont):
    return words([v * R2 % R for v in vals] if mont else vals)


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("n", [3, 31, 32, 33])
def test_rows(shim, n, mont):
    """k_bbs_rows for signing (mult = t_i, with t_i = 0 for a row without a signature) and for verification (mult = one): canonical words below r"""
    L = n - 2
    for rows in (1, 63, 64, 65):
        e, s, msgs = scenario(rows, L, 100 * n + rows, mont)
        flat = [v for r in msgs for v in r]
        ts = rand(np.random.default_rng(rows), rows)
        ts[0] = 0
        for t in (None, ts):
            out = np.zeros(8 * rows * n, np.uint32)
            shim.shim_rows(p_(form(s, mont)), p_(form(flat, mont)), None if t is None else p_(form(t, 1)), mont, rows, n, p_(out))
            want = [v for i in range(rows) for v in BM.row(s[i], msgs[i], 1 if t is None else t[i])]
            assert ints(out) == want, (rows, t is None)
            assert max(want) < R


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("rho", [1, 2, R - 1])
def test_batch_columns(shim, rho, mont):
    """k_bbs_col_sums / k_col_finish: -c_k, rho^i and rho^i e_i for row counts on both sides of a lane's run (16), of a wave (64), of a block (256 x 16), in
    one chunk and in chunks that end inside a run, at a run's end and past a block"""
    run = launcher_run()
    for rows, n, chunks in ((1, 3, (1,)), (2, 3, (2, 1)), (63, 31, (63, 16)), (64, 32, (64, 17)), (65, 33, (65, 64)), (257, 3, (257, 100)), (256 * run + 1, 3, (256 * run + 1, 256 * run))):
        L = n - 2
        e, s, msgs = scenario(rows, L, 7 * rows + n, mont)
        flat = [v for r in msgs for v in r]
        c, wts, we = BM.columns(rho, e, s, msgs)
        assert wts[-1] == pow(rho, rows - 1, R)
        for chunk in chunks:
            oc, ow, oe = np.zeros(8 * n, np.uint32), np.zeros(8 * rows, np.uint32), np.zeros(8 * rows, np.uint32)
            shim.shim_columns(p_(form(e, mont)), p_(form(s, mont)), p_(form(flat, mont)), p_(form([rho], mont)), mont, rows, n, chunk, run, p_(oc), p_(ow), p_(oe))
            assert ints(oc) == [(R - v) % R for v in c], (rows, n, chunk)
            assert ints(ow) == wts and ints(oe) == we, (rows, n, chunk)


def test_columns_of_a_chunk_start_from_their_row_offset():
    """the model's own consistency: the sums of two chunks add up to the whole (what the second pass relies on)"""
    rng = np.random.default_rng(5)
    e, s, msgs = rand(rng, 40), rand(rng, 40), [rand(rng, 2) for _ in range(40)]
    c, w, we = BM.columns(3, e, s, msgs)
    c0, w0, we0 = BM.columns(3, e[:25], s[:25], msgs[:25])
    c1, w1, we1 = BM.columns(3, e[25:], s[25:], msgs[25:], i0=25)
    assert [(a + b) % R for a, b in zip(c0, c1)] == c and w0 + w1 == w and we0 + we1 == we


@pytest.mark.parametrize("mont", [0, 1])
def test_host_inverses_with_rows_that_have_none(shim, mont):
    """x + e_i = 0 in the first and in the last position, alone, both, and beside each other: flagged, zero words, every other inverse right, share by share"""
    rng = np.random.default_rng(77)
    x = rand(rng, 1)[0]
    minus = (R - x) % R
    f = (lambda vals: limbs64([v * R2 % R for v in vals])) if mont else limbs64
    for m, shares, bad in ((1, 1, [0]), (5, 1, [0]), (5, 1, [4]), (5, 2, [0, 4]), (64, 3, [0, 1, 63]), (65, 16, [64]), (9, 4, [])):
        e = rand(rng, m)
        for i in bad:
            e[i] = minus
        if not mont and m > 2:
            e[2] = e[2] + R if e[2] + R <= TOP else e[2]                             # canonical words are taken mod r
        t, zero = np.full(4 * m, 7, np.uint64), np.full(m, 7, np.uint8)
        assert shim.shim_inverses(p_(f(e)), m, p_(f([x])), mont, shares, p_(t), p_(zero)) == 0
        want = BM.inverses(x, e)
        assert zero.tolist() == [int(z) for _, z in want]
        got = [sum(int(v) << (64 * k) for k, v in enumerate(row)) for row in t.reshape(-1, 4)]
        assert got == [v * R2 % R for v, _ in want], (m, shares, bad)


def test_the_model_against_the_oracle():
    """one signature from known discrete logs: the oracle's MSM over the parameter points gives b, (x + e) A = b, and the reference's pairing equation holds"""
    G = O.G1
    rng = np.random.default_rng(99)
    x, gamma = rand(rng, 2)
    key = BM.Key(x, gamma, rand(rng, 4))
    e, s, msgs = rand(rng, 1)[0], rand(rng, 1)[0], rand(rng, 3)
    lim = lambda v: O.int_to_limbs(v % R, 4)
    gen = G.generator()
    pts = np.stack([G.to_affine(G.mul(gen, lim(k)))[0] for k in key.params_scalars(3)])
    b = G.to_affine(G.msm(pts, np.stack([lim(v) for v in BM.row(s, msgs)])))[0]
    assert (b == G.to_affine(G.mul(gen, lim(key.b(s, msgs))))[0]).all()
    a = key.a(e, s, msgs)
    A = G.to_affine(G.mul(gen, lim(a)))[0]
    assert (G.to_affine(G.mul(A, lim(x + e)))[0] == b).all()
    assert key.verifies(a, e, s, msgs) and not key.verifies(a, e, s, [msgs[0] + 1] + msgs[1:])
    d = G.to_affine(G.mul(gen, lim(key.d(a, e, s, msgs))))[0]
    g2 = O.G2.generator()
    w = O.G2.to_affine(O.G2.mul(g2, lim(x)))[0]
    gt = O.final_exponentiation(O.multi_miller_loop(np.stack([A, d]), np.stack([w, g2])))
    assert gt is not None and (gt == O.fp12_one()).all()
    assert key.a((R - x) % R, s, msgs) is None
