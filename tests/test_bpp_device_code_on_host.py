"""CPU: the per-lane routines of Bulletproofs++ range proofs in bulk (crypto_amd/csrc/bpp_kernels.hip.h: bpp_consts, bpp_shared, batch_weight_index, shape_ok)
compiled for the host with the FP29_CHECK operand asserts (tests/native/bpp_dev_host_shim.cpp, a stand-alone host build) and driven as k_bpp_consts, k_bpp_shared,
k_bpp_col_sums, k_col_finish and the chunks of dock_bpp.hip drive them, against the closed form of tests/bpp_model.py: all 9 + NG shared and m + 4 + 2 K own
scalars of every shape of the issue, both input forms, the values 0, 1, r - 1, r and 2^256 - 1 in every input position (each challenge, l0, n0), the status-2
cases t = 0, r = 0, e = -k, and the batch's column sums and weights at proof counts on both sides of a lane's run (15, 16, 17) and of a wave (63, 64, 65), in
forced chunks, under the batching scalars 1, 2 and r - 1.  A green run shows the values are right and that no product leaves fr_mul's operand contract."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import bpp_model as BM
from bbs_model import R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "bpp_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libbpp_dev_host_shim.so")
R2 = pow(2, 256, R)
TOP = (1 << 256) - 1
IDS = ["%d-%d-%d" % s for s in BM.SHAPES]
p_ = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC, os.path.join(HERE, "native", "col_frame_host.hpp")] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "col_sums.hip.h", "bbs_routines.hip.h", "bpp_kernels.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz, i, u = C.c_void_p, C.c_size_t, C.c_int, C.c_uint
    L.shim_bpp_shape.argtypes = [u, u, u, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.shim_bpp_shape.restype = i
    L.shim_bpp_scalars.argtypes = [u, u, u, vp, vp, i, sz, sz, vp, vp, vp]
    L.shim_bpp_columns.argtypes = [u, u, u, vp, vp, vp, i, sz, sz, sz, vp, vp]
    L.shim_bpp_scalars.restype = L.shim_bpp_columns.restype = None
    return L


def words(vals):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for v in vals for i in range(8)], dtype=np.uint32)


def ints(w):
    return [sum(int(x) << (32 * i) for i, x in enumerate(row)) for row in w.reshape(-1, 8).astype(object)]


def form(vals, mont):
    return words([v * R2 % R for v in vals] if mont else vals)


def synthetic(shape, rows, seed, mont, edges=True):
    """`rows` proofs' scalars (the points play no part here).  With edges the first proofs carry 0, 1, r - 1 (and, as canonical words, r and 2^256 - 1) in every
    input position in turn: position p < 7 + K challenge p, then l0, n0.  Returns the raw values per proof (challenges, then l0, n0) and the model's proofs"""
    rnd = BM.make_rnd(seed)
    npos = 7 + shape.K + 2
    raw = [[rnd() for _ in range(npos)] for _ in range(rows)]
    if edges:
        vals = [0, 1, R - 1] + ([] if mont else [R, TOP])
        k = 0
        for pos in range(npos):
            for v in vals:
                raw[k][pos] = v
                k += 1
        assert k <= rows
    proofs = [BM.Proof([0] * shape.m, 0, 0, 0, 0, [0] * shape.K, [0] * shape.K, [q[-2]], [q[-1]], q[:-2]) for q in raw]
    return raw, proofs


def run_scalars(L, shape, raw, mont, own_stride=None):
    rows, nc = len(raw), 7 + shape.K
    own_stride = own_stride or shape.own
    chal = form([v for q in raw for v in q[:nc]], mont)
    l_n = form([v for q in raw for v in q[nc:]], mont)
    shared, own, bad = np.zeros(rows * shape.shared * 8, np.uint32), np.zeros(rows * own_stride * 8, np.uint32), np.zeros(rows, np.uint8)
    L.shim_bpp_scalars(shape.base, shape.num_bits, shape.m, p_(chal), p_(l_n), 1 if mont else 0, rows, own_stride, p_(shared), p_(own), p_(bad))
    sh, ow = ints(shared), ints(own)
    return [sh[i * shape.shared:(i + 1) * shape.shared] for i in range(rows)], [ow[i * own_stride:(i + 1) * own_stride] for i in range(rows)], bad.tolist()


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("shape", BM.SHAPES, ids=IDS)
def test_every_scalar_equals_the_closed_form(shim, shape, mont):
    s = BM.Shape(*shape)
    rows = (7 + s.K + 2) * (3 if mont else 5) + 3
    raw, proofs = synthetic(s, rows, 7 + s.NG, mont)
    shared, own, bad = run_scalars(shim, s, raw, mont)
    n2 = 0
    for i, p in enumerate(proofs):
        want = BM.verify_closed(s, p)
        assert bad[i] == (1 if want is None else 0), (i, raw[i])
        if want is None:
            n2 += 1
            continue
        assert shared[i] == want[0], (i, [k for k in range(s.shared) if shared[i][k] != want[0][k]][:4])
        assert own[i] == want[1], (i, [k for k in range(s.own) if own[i][k] != want[1][k]][:4])
    assert n2 >= 3                       # t = 0, r = 0, e = 0 at least (r and 2^256 - 1 add theirs in the canonical form)


@pytest.mark.parametrize("shape", [(2, 8, 1), (16, 8, 1), (2, 64, 2)], ids=["2-8-1", "16-8-1", "2-64-2"])
def test_the_one_behind_the_own_scalars(shim, shape):
    """the each call's layout: own + 1 scalars a proof, the last of them one (the scalar of P_i)"""
    s = BM.Shape(*shape)
    raw, proofs = synthetic(s, 3, 5, False, edges=False)
    _, own, bad = run_scalars(shim, s, raw, False, own_stride=s.own + 1)
    for i, p in enumerate(proofs):
        assert own[i] == BM.verify_closed(s, p)[1] + [1] and not bad[i]


@pytest.mark.parametrize("shape", BM.SHAPES, ids=IDS)
def test_status_two(shim, shape):
    """t = 0, r = 0 and e = -k for every k < base, in both forms and as the non-canonical words r and r - k + r; e = -base is NOT one"""
    s = BM.Shape(*shape)
    for mont in (False, True):
        cases = [(6, 0), (3, 0)] + [(0, (R - k) % R) for k in range(s.base)]
        if not mont:
            cases += [(6, R), (3, R), (0, 2 * R - 1)]
        raw, _ = synthetic(s, len(cases) + 1, 11, mont, edges=False)
        for i, (pos, v) in enumerate(cases):
            raw[i][pos] = v
        raw[-1][0] = R - s.base
        _, _, bad = run_scalars(shim, s, raw, mont)
        assert bad == [1] * len(cases) + [0]


@pytest.mark.parametrize("shape", BM.SHAPES, ids=IDS)
def test_column_sums_and_weights(shim, shape):
    s = BM.Shape(*shape)
    total = 65
    for mont in (False, True):
        raw, proofs = synthetic(s, total, 23 + s.NG, mont, edges=False)
        raw[0][-1] = raw[64][-2] = R - 1
        proofs[0].n[0] = proofs[64].l[0] = R - 1
        shared, own, bad = run_scalars(shim, s, raw, mont)
        assert not any(bad)
        sh_w, own_w = words([v for r_ in shared for v in r_]), words([v for r_ in own for v in r_])
        for rows, chunk in ((15, 15), (16, 16), (17, 16), (63, 63), (64, 16), (65, 16), (65, 64), (65, 65)):
            for rho in (1, 2, R - 1):
                c, wts = np.zeros(s.shared * 8, np.uint32), np.zeros(rows * s.own * 8, np.uint32)
                shim.shim_bpp_columns(s.base, s.num_bits, s.m, p_(sh_w), p_(own_w), p_(form([rho], mont)), 1 if mont else 0, rows, chunk, 16, p_(c), p_(wts))
                want_c = [sum(pow(rho, i, R) * shared[i][k] for i in range(rows)) % R for k in range(s.shared)]
                assert ints(c) == want_c, (rows, chunk, rho)
                got = ints(wts)
                # every chunk's weights lie in the order of its three point arrays
                for i0 in range(0, rows, chunk):
                    n = min(chunk, rows - i0)
                    part = got[i0 * s.own:(i0 + n) * s.own]
                    for i in range(n):
                        w = pow(rho, i0 + i, R)
                        mine = part[i * s.m:(i + 1) * s.m] + part[n * s.m + 4 * i:n * s.m + 4 * i + 4] + part[n * (s.m + 4) + 2 * s.K * i:n * (s.m + 4) + 2 * s.K * (i + 1)]
                        assert mine == [w * o % R for o in own[i0 + i]], (rows, chunk, rho, i0 + i)
        if mont:
            continue
        # the model's own batch_columns agrees with the sums above on the first chunk
        coeff, wl = BM.batch_columns(s, proofs[:17], 2)
        assert coeff == [sum(pow(2, i, R) * shared[i][k] for i in range(17)) % R for k in range(s.shared)] and wl[16] == [pow(2, 16, R) * o % R for o in own[16]]


def test_shapes_the_calls_refuse(shim):
    for base in range(0, 34):
        for num_bits in (0, 1, 2, 3, 4, 6, 8, 16, 24, 32, 64, 128):
            for m in (0, 1, 2, 3, 4, 8, 16):
                NG, K, own = C.c_int(), C.c_int(), C.c_int()
                ok = shim.shim_bpp_shape(base, num_bits, m, C.byref(NG), C.byref(K), C.byref(own))
                pow2 = lambda v: v > 0 and v & (v - 1) == 0
                good = base in (2, 4, 8, 16) and pow2(num_bits) and base.bit_length() - 1 <= num_bits <= 64 and pow2(m) and m <= 8
                if good:
                    s = BM.Shape(base, num_bits, m)
                    good = pow2(s.NG)
                assert bool(ok) == good, (base, num_bits, m)
                if good:
                    assert (NG.value, K.value, own.value) == (s.NG, s.K, s.own)
