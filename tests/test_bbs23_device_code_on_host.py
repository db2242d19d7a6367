"""CPU: the per-lane routines of BBS (2023) in bulk — bbs_routines.hip.h's row_value_fixed with one fixed column (the signature calls) and
crypto_amd/csrc/bbs23_kernels.hip.h (row_entry, own_scalar, col_run, col_term, row_weights, stage_src, fq_neg_words, g1_is_negation, status_of) — compiled for the
host with the FP29_CHECK operand asserts (tests/native/bbs23_dev_host_shim.cpp) and driven as the kernels and the chunks of dock_bbs.hip drive them, against the
big-integer model of tests/bbs23_model.py: both proof kinds, both input forms, the values 0, 1, r - 1, r and 2^256 - 1, rows of L + 1 = 2, 31, 32, 33 entries, every
mask kind, row counts on both sides of a lane's run (15, 16, 17), a wave (63, 64, 65), a block (4095, 4096, 4097) and a forced chunk, the batching scalars 1, 2
and r - 1, the y-flip, and the status routine on every flag combination.  (The model itself is checked against the oracle in tests/test_bbs23_model.py.)  A green
run shows the values are right and that no product leaves fr_mul's operand contract."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import bbs23_model as M
from bbs23_model import R, CDL, IETF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "bbs23_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libbbs23_dev_host_shim.so")
R2 = pow(2, 256, R)
TOP = (1 << 256) - 1
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
SHAPE = {CDL: dict(pts=5, resp=3, own=6), IETF: dict(pts=3, resp=2, own=3)}
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC, os.path.join(HERE, "native", "col_frame_host.hpp")] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "col_sums.hip.h", "bbs_routines.hip.h", "bbs23_kernels.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
    L.shim_bbs23_sig_rows.argtypes = [vp, vp, ci, sz, sz, vp]
    L.shim_bbs23_sig_columns.argtypes = [vp, vp, vp, ci, sz, sz, sz, sz, vp, vp, vp]
    L.shim_bbs23_rows.argtypes = [vp, vp, vp, vp, sz, ci, ci, sz, vp, vp]
    L.shim_bbs23_stage.argtypes = [vp, ci, sz, vp, vp, vp, vp]
    L.shim_bbs23_columns.argtypes = [vp, vp, vp, vp, sz, vp, ci, ci, sz, sz, sz, vp, vp, vp, vp]
    L.shim_bbs23_fq_neg.argtypes = [vp, vp]
    L.shim_bbs23_is_negation.argtypes = [vp, ci, vp, ci]
    L.shim_bbs23_status.argtypes = [ci] * 4
    for f in (L.shim_bbs23_sig_rows, L.shim_bbs23_sig_columns, L.shim_bbs23_rows, L.shim_bbs23_stage, L.shim_bbs23_columns, L.shim_bbs23_fq_neg):
        f.restype = None
    L.shim_bbs23_is_negation.restype = L.shim_bbs23_status.restype = ci
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


def edges(mont):
    return [0, 1, R - 1] + ([] if mont else [R, TOP])


def mask_of(i, L):
    kind = i % 6
    if kind == 0:
        return [1 if (i * 7 + j * j + j // 3) % 3 == 0 else 0 for j in range(L)]
    return {1: [0] * L, 2: [1] * L, 3: [1] + [0] * (L - 1), 4: [0] * (L - 1) + [1], 5: [j & 1 for j in range(L)]}[kind]


def scenario(kind, rows, L, seed, mont):
    """`rows` proofs' scalars (the points play no part here) with the edge values spread over them and every mask kind in turn.  raw: what the kernels are
    handed; the proofs hold the same values (the model reduces what it reads)"""
    rng = np.random.default_rng(seed)
    nr = SHAPE[kind]["resp"]
    raw = [dict(c=rand(rng, 1)[0], resp=rand(rng, nr), vals=rand(rng, L), mask=mask_of(i, L)) for i in range(rows)]
    for k, v in enumerate(edges(mont)):
        raw[k % rows]["c"] = v
        for q in range(nr):
            raw[(k + 1 + q) % rows]["resp"][q] = v
        raw[rows - 1]["resp"][k % nr] = v
        raw[(k + 2) % rows]["vals"][k % L] = v
        raw[(2 * k + 1) % rows]["vals"][L - 1] = v                        # (rows 1 and 2 of six: everything hidden, everything revealed)
    return raw, [M.Proof(kind, [0] * SHAPE[kind]["pts"], q["resp"], q["vals"], q["mask"], q["c"]) for q in raw]


def arrays(raw, mont):
    return (form([q["c"] for q in raw], mont), form([z for q in raw for z in q["resp"]], mont), form([v for q in raw for v in q["vals"]], mont),
            np.array([m for q in raw for m in q["mask"]], np.uint8))


def launcher_run():
    hdr = open(os.path.join(CSRC, "col_launch.hip.h")).read()
    return int(re.search(r"\bCOL_RUN = (\d+)\b", hdr).group(1))


def test_the_constants_are_the_launchers():
    assert launcher_run() == 16
    src = open(os.path.join(CSRC, "k_bbs23.hip")).read()
    assert "colk::col_blocks(rows)" in src and "colk::COL_RUN" in src and "dim3(256)" in src      # a block is 256 lanes of COL_RUN rows each: what the shim drives
    assert "n = in.L + 1" in src
    hdr = open(os.path.join(CSRC, "bbs23_launch.hip.h")).read()
    assert "BBS23_EACH_CHUNK = 4096, BBS23_BATCH_CHUNK = 65536" in hdr
    drv = open(os.path.join(CSRC, "dock_bbs.hip")).read()
    assert drv.count("montgomery != 0, 1}") == 3 and drv.count("montgomery != 0, 2}") == 3                # the fixed columns of the 2023 and the BBS+ signature calls


@pytest.mark.parametrize("mont", [0, 1])
def test_signature_rows_with_one_fixed_column(shim, mont):
    """k_bbs_rows, fixed = 1, for signing (mult = t_i, with t_i = 0 for a row without a signature) and for verification (mult = one): canonical words below r"""
    rng = np.random.default_rng(3 + mont)
    x = rand(rng, 1)[0]
    for L in (1, 30, 31, 32):
        for rows in (1, 15, 16, 17, 65):
            msgs, es = [rand(rng, L) for _ in range(rows)], rand(rng, rows)
            for k, v in enumerate(edges(mont)):
                msgs[k % rows][k % L] = v
            es[rows // 2] = (R - x) % R
            flat = form([v for m in msgs for v in m], mont)
            out = np.zeros(8 * rows * (L + 1), np.uint32)
            shim.shim_bbs23_sig_rows(p_(flat), None, mont, rows, L + 1, p_(out))
            assert ints(out) == [v for m in msgs for v in M.row(m)], (L, rows)
            t = form([ti for ti, _ in M.inverses(x, es)], 1)
            shim.shim_bbs23_sig_rows(p_(flat), p_(t), mont, rows, L + 1, p_(out))
            want = [v for r in M.sign_rows(x, es, msgs) for v in r]
            assert ints(out) == want and max(want) < R and want[(rows // 2) * (L + 1)] == 0, (L, rows)


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("rho", [1, 2, R - 1])
def test_signature_columns_with_one_fixed_column(shim, rho, mont):
    """k_bbs_col_sums / k_col_finish, fixed = 1: -c_k for the L + 1 columns, rho^i and rho^i e_i, in one chunk and in forced chunks"""
    run = launcher_run()
    shapes = ((1, 1, (1,)), (15, 1, (15, 7)), (16, 2, (16,)), (17, 30, (17, 16)), (63, 31, (63, 16)), (64, 32, (64, 17)), (65, 30, (65, 64)), (4095, 1, (4095,)),
              (4096, 1, (4096, 4095)), (4097, 1, (4097, 4096, 65)))
    for rows, L, chunks in shapes:
        rng = np.random.default_rng(rows + L)
        msgs, es = [rand(rng, L) for _ in range(rows)], rand(rng, rows)
        for k, v in enumerate(edges(mont)):
            msgs[k % rows][k % L] = v
            es[(k + 1) % rows] = v
        c, wts, we = M.columns(rho, es, msgs)
        for chunk in chunks:
            oc, ow, oe = np.zeros(8 * (L + 1), np.uint32), np.zeros(8 * rows, np.uint32), np.zeros(8 * rows, np.uint32)
            shim.shim_bbs23_sig_columns(p_(form(es, mont)), p_(form([v for m in msgs for v in m], mont)), p_(form([rho], mont)), mont, rows, L + 1, chunk, run, p_(oc), p_(ow), p_(oe))
            assert ints(oc) == [(R - v) % R for v in c], (rows, L, chunk)
            assert ints(ow) == wts and ints(oe) == we, (rows, L, chunk)


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("kind", [CDL, IETF])
def test_rows_and_own_scalars(shim, kind, mont):
    """k_bbs23_rows and k_bbs23_own: canonical words below r of (c, y_1 .. y_L) for rows of 2, 31, 32 and 33 entries under every mask kind, and of
    (z1, z2, -c, -1 | z3, -1), respectively (z_a, z_b, -1); c = 0 and every edge value among the rows"""
    no = SHAPE[kind]["own"]
    for L in (1, 30, 31, 32):
        for rows in (1, 2, 15, 16, 17, 63, 64, 65):
            raw, proofs = scenario(kind, rows, L, 100 * rows + L + kind, mont)
            out, own = np.zeros(8 * rows * (L + 1), np.uint32), np.zeros(8 * rows * no, np.uint32)
            shim.shim_bbs23_rows(*map(p_, arrays(raw, mont)), L, kind, mont, rows, p_(out), p_(own))
            want = [v for p in proofs for v in p.row()]
            assert ints(out) == want and max(want) < R, (L, rows)
            want = [v for p in proofs for v in p.own()]
            assert ints(own) == want and max(want) < R, (L, rows)
        if rows >= 6:
            assert {tuple(q["mask"]) for q in raw} >= {tuple(mask_of(i, L)) for i in range(6)}


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("rho", [1, 2, R - 1])
@pytest.mark.parametrize("kind", [CDL, IETF])
def test_batch_columns_and_weights(shim, kind, rho, mont):
    """k_bbs23_col_sums / k_col_finish: C_k, the weights over the own points, rho^i and -rho^i for row counts on both sides of a lane's run (16), of a wave
    (64), of a block (256 x 16), in one chunk and in chunks that end inside a run, at a run's end and past a block"""
    run = launcher_run()
    assert 256 * run == 4096
    shapes = ((1, 1, (1,)), (2, 2, (2, 1)), (15, 1, (15, 7)), (16, 30, (16,)), (17, 31, (17, 16)), (63, 32, (63, 16)), (64, 1, (64, 17)), (65, 30, (65, 64)), (257, 2, (257, 100)),
              (4095, 1, (4095,)), (4096, 1, (4096, 4095)), (4097, 1, (4097, 4096, 65)))
    np_ = SHAPE[kind]["pts"]
    for rows, L, chunks in shapes:
        raw, proofs = scenario(kind, rows, L, 7 * rows + L + kind, mont)
        s, w, tp, tn = M.batch(None, proofs, rho)
        assert tp[-1] == pow(rho, rows - 1, R) and len(s) == L + 1
        for chunk in chunks:
            oc, ow, op, on = np.zeros(8 * (L + 1), np.uint32), np.zeros(8 * np_ * rows, np.uint32), np.zeros(8 * rows, np.uint32), np.zeros(8 * rows, np.uint32)
            shim.shim_bbs23_columns(*map(p_, arrays(raw, mont)), L, p_(form([rho], mont)), kind, mont, rows, chunk, run, p_(oc), p_(ow), p_(op), p_(on))
            assert ints(oc) == s, (rows, chunk)
            assert ints(ow) == [x for r in w for x in r], (rows, chunk)
            assert ints(op) == tp and ints(on) == tn, (rows, chunk)


@pytest.mark.parametrize("kind", [CDL, IETF])
def test_staging_lays_out_bases_sides_and_flags(shim, kind):
    """k_bbs23_stage's routine: every slot takes the point the layout names ([Abar, d, Bbar, T1 | d, T2], respectively [Abar, Bbar, T]), the pairing's sides are
    Abar and -Bbar, and the flags mark zero words — identities at every position among the rows"""
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
    pw = words([c for row in points for q in row for c in q], 12)
    own, pa, pb, skip = np.zeros(rows * no * 24, np.uint32), np.zeros(rows * 24, np.uint32), np.zeros(rows * 24, np.uint32), np.full(2 * rows, 9, np.uint8)
    shim.shim_bbs23_stage(p_(pw), kind, rows, p_(own), p_(pa), p_(pb), p_(skip))
    want_own, want_a, want_b = [], [], []
    for row in points:
        want_own += [row[0], row[2], row[1], row[3], row[2], row[4]] if kind == CDL else [row[0], row[1], row[2]]
        want_a.append(row[0])
        want_b.append([row[1][0], (P - row[1][1]) % P])
    got = lambda a: [list(x) for x in zip(*[iter(ints(a, 12))] * 2)]
    assert got(own) == want_own and got(pa) == want_a and got(pb) == want_b
    zero = lambda q: 1 if q == [0, 0] else 0
    assert skip[:rows].tolist() == [zero(r[0]) for r in points] and skip[rows:].tolist() == [zero(r[1]) for r in points]
    assert sum(skip[:rows]) == 3 and sum(skip[rows:]) == 3
    # the model names the same bases for the own scalars
    pf = M.Proof(kind, list(range(10, 10 + npts)), [0] * SHAPE[kind]["resp"], [0], [0], 0)
    assert pf.own_bases() == ([10, 12, 11, 13, 12, 14] if kind == CDL else [10, 11, 12])


def test_base_field_words_and_statuses(shim):
    """-y = p - y (zero stays zero), Q = -P on affine words with flags, and the order of the checks on every flag combination"""
    rng = np.random.default_rng(11)
    ys = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, (1 << 380) + 12345, 0xFFFFFFFF, 1 << 32, (1 << 352) - 1] + [int.from_bytes(rng.bytes(60), "little") % P for _ in range(20)]
    for y in ys:
        out = np.zeros(12, np.uint32)
        shim.shim_bbs23_fq_neg(p_(words([y], 12)), p_(out))
        assert ints(out, 12) == [(P - y) % P], hex(y)
        if y:
            x = int.from_bytes(rng.bytes(60), "little") % P
            a, b = words([x, y], 12), words([x, P - y], 12)
            assert shim.shim_bbs23_is_negation(p_(a), 0, p_(b), 0) == 1
            assert shim.shim_bbs23_is_negation(p_(a), 0, p_(a), 0) == (1 if 2 * y == P else 0)
            assert shim.shim_bbs23_is_negation(p_(a), 0, p_(words([x ^ 1, P - y], 12)), 0) == 0
            assert shim.shim_bbs23_is_negation(p_(a), 0, p_(words([x, (P - y) ^ (1 << 352)], 12)), 0) == 0
            assert shim.shim_bbs23_is_negation(p_(a), 1, p_(b), 0) == 0 and shim.shim_bbs23_is_negation(p_(a), 0, p_(b), 1) == 0
            assert shim.shim_bbs23_is_negation(p_(a), 1, p_(a), 1) == 1
    for bits in range(16):
        a_inf, first, second, pairing = [(bits >> k) & 1 for k in range(4)]
        assert shim.shim_bbs23_status(a_inf, first, second, pairing) == (1 if a_inf else 2 if not first else 3 if not second else 4 if not pairing else 0)
    assert {shim.shim_bbs23_status(a, 1, s, p) for a in (0, 1) for s in (0, 1) for p in (0, 1)} == {0, 1, 3, 4}      # IETF: first_ok is always set, 2 never comes
