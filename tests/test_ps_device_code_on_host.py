"""CPU: the per-lane routines of PS (Coconut) signatures in bulk — crypto_amd/csrc/ps_kernels.hip.h (sign_scalar, pok_row_entry, col_scalars, g2_equal, status_of)
and bbs_routines.hip.h's row_value_fixed with one fixed column (the verification rows) — compiled for the host with the FP29_CHECK operand asserts
(tests/native/ps_dev_host_shim.cpp) and driven as the kernels and the chunks of dock_ps.hip drive them, against the big-integer model of tests/ps_model.py: both
input forms, the values 0, 1, r - 1, r and 2^256 - 1, L = 1, 2, 30, 31, 32, every mask kind, row counts on both sides of a wave (63, 64, 65), a block (255, 256,
257) and a forced chunk, the batching scalars 1, 2 and r - 1, and the status routine on every flag combination with the precedence 3 > 1 > 4.  (The model itself
is checked against the oracle in tests/test_ps_model.py.)  A green run shows the values are right and that no product leaves fr_mul's operand contract."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import ps_model as M
from ps_model import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "ps_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libps_dev_host_shim.so")
R2 = pow(2, 256, R)
TOP = (1 << 256) - 1
LS = (1, 2, 30, 31, 32)
ROWS = (1, 2, 63, 64, 65, 255, 256, 257)
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "col_sums.hip.h", "bbs_routines.hip.h", "ps_kernels.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
    L.shim_ps_sign_rows.argtypes = [vp, vp, vp, ci, sz, sz, sz, vp]
    L.shim_ps_verify_rows.argtypes = [vp, ci, sz, sz, vp]
    L.shim_ps_pok_rows.argtypes = [vp, vp, vp, sz, ci, sz, vp]
    L.shim_ps_col_scalars.argtypes = [vp, vp, ci, sz, sz, sz, sz, vp]
    L.shim_ps_g2_equal.argtypes = [vp, ci, vp, ci]
    L.shim_ps_status.argtypes = [ci] * 4
    for f in (L.shim_ps_sign_rows, L.shim_ps_verify_rows, L.shim_ps_pok_rows, L.shim_ps_col_scalars):
        f.restype = None
    L.shim_ps_g2_equal.restype = L.shim_ps_status.restype = ci
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


def test_the_constants_are_the_launchers():
    hdr = open(os.path.join(CSRC, "ps_launch.hip.h")).read()
    assert re.search(r"PS_EACH_CHUNK = 4096, PS_BATCH_TERMS = \(size_t\)1 << 20, PS_BATCH_CHUNK = 65536, PS_COL_RUN = 16\b", hdr)
    src = open(os.path.join(CSRC, "k_ps.hip")).read()
    assert "dim3((unsigned)(L + 2), (unsigned)nb), dim3(256)" in src and "256 * PS_COL_RUN" in src           # a block is 256 lanes of PS_COL_RUN rows each: what the shim drives
    assert "blocks_for(2 * rows * (in.L + 2))" in src                                                        # two rows of L + 2 entries per proof
    assert "bbsk::launch_bbs_rows(s, nullptr, msgs, nullptr, mont, rows, n, 1, out_rows)" in hdr             # launch_ps_rows: one fixed column, no s, no multiplier


@pytest.mark.parametrize("mont", [0, 1])
def test_sign_scalars(shim, mont):
    """k_ps_sign_rows: (r_i, r_i (x + sum y_j m_ij)) as canonical words below r — r_i = 0, u_i = 0 by a message that solves it, every edge value in the key, the
    r_i and the messages, in one chunk and in forced chunks"""
    for L in LS:
        for rows in ROWS:
            rng = np.random.default_rng(1000 * L + rows + mont)
            x, ys = rand(rng, 1)[0], rand(rng, L)
            rs, msgs = rand(rng, rows), [rand(rng, L) for _ in range(rows)]
            for k, v in enumerate(edges(mont)):
                msgs[k % rows][k % L] = v
                rs[(k + 1) % rows] = v
                msgs[(2 * k + 1) % rows][L - 1] = v
            if rows >= 63:
                i = rows // 2                                                       # u_i = 0: the first message solves x + sum y_j m_j = 0
                msgs[i][0] = (-(x + sum(y * m for y, m in zip(ys[1:], msgs[i][1:]))) * M.inv(ys[0])) % R
                rs[i] = rs[i] % R or 1
            want = [v for r, m in zip(rs, msgs) for v in M.sign_scalars(x, ys, r, m)]
            if rows >= 63:
                assert want[2 * (rows // 2) + 1] == 0 and want[2 * (rows // 2)] != 0
            for chunk in sorted({rows, 16, 100}):
                out = np.zeros(16 * rows, np.uint32)
                shim.shim_ps_sign_rows(p_(form([x] + ys, mont)), p_(form(rs, mont)), p_(form([v for m in msgs for v in m], mont)), mont, rows, L, chunk, p_(out))
                assert ints(out) == want and max(want) < R, (L, rows, chunk)
    # the key's own edge values: x and every y_j among 0, 1, r - 1 (and r, 2^256 - 1 in the canonical form)
    rng = np.random.default_rng(77 + mont)
    for L in (1, 2, 32):
        for v in edges(mont):
            for key in ([v] + rand(rng, L), [rand(rng, 1)[0]] + [v] * L):
                rs, msgs = rand(rng, 3), [rand(rng, L) for _ in range(3)]
                out = np.zeros(48, np.uint32)
                shim.shim_ps_sign_rows(p_(form(key, mont)), p_(form(rs, mont)), p_(form([q for m in msgs for q in m], mont)), mont, 3, L, 3, p_(out))
                assert ints(out) == [q for r, m in zip(rs, msgs) for q in M.sign_scalars(key[0], key[1:], r, m)], (L, v)


@pytest.mark.parametrize("mont", [0, 1])
def test_verification_rows(shim, mont):
    """k_bbs_rows with one fixed column and no multiplier: (1, m_i1 .. m_iL) as canonical words below r"""
    for L in LS:
        for rows in (1, 63, 64, 65, 257):
            rng = np.random.default_rng(L + rows)
            msgs = [rand(rng, L) for _ in range(rows)]
            for k, v in enumerate(edges(mont)):
                msgs[k % rows][k % L] = v
            out = np.zeros(8 * rows * (L + 1), np.uint32)
            shim.shim_ps_verify_rows(p_(form([v for m in msgs for v in m], mont)), mont, rows, L + 1, p_(out))
            want = [v for m in msgs for v in M.verify_row(m)]
            assert ints(out) == want and max(want) < R, (L, rows)


@pytest.mark.parametrize("mont", [0, 1])
def test_proof_rows(shim, mont):
    """k_ps_pok_rows: the S rows (0, hidden ? z : 0 .., z_r) of the chunk, then its R rows (1, revealed ? m : 0 .., 0), under every mask kind"""
    for L in LS:
        for rows in ROWS:
            rng = np.random.default_rng(100 * rows + L)
            proofs = [M.Proof([1, 1], 0, 0, rand(rng, L), mask_of(i, L), rand(rng, 1)[0], 0) for i in range(rows)]
            raw = [dict(vals=list(p.values), z=p.z_r) for p in proofs]
            for k, v in enumerate(edges(mont)):
                raw[k % rows]["z"] = v
                raw[(k + 2) % rows]["vals"][k % L] = v
                raw[(2 * k + 1) % rows]["vals"][L - 1] = v                  # (rows 1 and 2 of six: everything hidden, everything revealed)
            proofs = [M.Proof(p.sig, 0, 0, q["vals"], p.mask, q["z"], 0) for p, q in zip(proofs, raw)]
            out = np.zeros(8 * 2 * rows * (L + 2), np.uint32)
            shim.shim_ps_pok_rows(p_(form([q["z"] for q in raw], mont)), p_(form([v for q in raw for v in q["vals"]], mont)),
                                  p_(np.array([m for p in proofs for m in p.mask], np.uint8)), L, mont, rows, p_(out))
            want = [v for p in proofs for v in p.rows()[0]] + [v for p in proofs for v in p.rows()[1]]
            assert ints(out) == want and max(want) < R, (L, rows)
            if rows >= 6:
                assert {tuple(p.mask) for p in proofs} >= {tuple(mask_of(i, L)) for i in range(6)}


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("rho", [1, 2, R - 1])
def test_batch_columns(shim, rho, mont):
    """k_ps_col_scalars: rho^i, rho^i m_ij and -rho^i column-major, for row counts on both sides of a lane's run (16), a wave and a block, in one chunk and in
    chunks that end inside a run, at a run's end and past a block"""
    hdr = open(os.path.join(CSRC, "ps_launch.hip.h")).read()
    run = int(re.search(r"PS_COL_RUN = (\d+)\b", hdr).group(1))
    shapes = ((1, 1, (1,)), (2, 2, (2, 1)), (15, 1, (15, 7)), (16, 30, (16,)), (17, 31, (17, 16)), (63, 32, (63, 16)), (64, 1, (64, 17)), (65, 30, (65, 64)), (255, 2, (255,)),
              (256, 2, (256, 100)), (257, 2, (257, 256)), (4097, 1, (4097, 4096, 65)))
    for rows, L, chunks in shapes:
        rng = np.random.default_rng(7 * rows + L)
        msgs = [rand(rng, L) for _ in range(rows)]
        for k, v in enumerate(edges(mont)):
            msgs[k % rows][k % L] = v
        want = [v for col in M.col_scalars(rho, msgs) for v in col]
        for chunk in chunks:
            out = np.zeros(8 * (L + 2) * rows, np.uint32)
            shim.shim_ps_col_scalars(p_(form([v for m in msgs for v in m], mont)), p_(form([rho], mont)), mont, rows, L, chunk, run, p_(out))
            assert ints(out) == want and max(want) < R, (rows, L, chunk)


def test_point_words_and_statuses(shim):
    """equality of two affine G2 points on words and flags (an identity: a flag or zero words), and the order of the checks on every flag combination: 3 over 1
    over 4, never 2"""
    rng = np.random.default_rng(11)
    a = rng.integers(1, 1 << 32, 48, dtype=np.uint64).astype(np.uint32)
    z = np.zeros(48, np.uint32)
    assert shim.shim_ps_g2_equal(p_(a), 0, p_(a.copy()), 0) == 1
    for k in (0, 1, 11, 12, 23, 24, 47):
        for bit in (0, 31):
            b = a.copy(); b[k] ^= np.uint32(1 << bit)
            assert shim.shim_ps_g2_equal(p_(a), 0, p_(b), 0) == 0, (k, bit)
    assert shim.shim_ps_g2_equal(p_(a), 1, p_(a), 0) == 0 and shim.shim_ps_g2_equal(p_(a), 0, p_(a), 1) == 0 and shim.shim_ps_g2_equal(p_(a), 1, p_(a), 1) == 1
    assert shim.shim_ps_g2_equal(p_(z), 0, p_(a), 0) == 0 and shim.shim_ps_g2_equal(p_(a), 0, p_(z), 0) == 0
    assert shim.shim_ps_g2_equal(p_(z), 0, p_(z), 0) == 1 and shim.shim_ps_g2_equal(p_(a), 1, p_(z), 0) == 1 and shim.shim_ps_g2_equal(p_(z), 0, p_(a), 1) == 1
    seen = set()
    for bits in range(16):
        s, i1, i2, p = [(bits >> k) & 1 for k in range(4)]
        got = shim.shim_ps_status(s, i1, i2, p)
        assert got == M.status_of(s, i1, i2, p) == (3 if not s else 1 if (i1 or i2) else 4 if not p else 0), bits
        seen.add(got)
    assert seen == {0, 1, 3, 4}
    assert shim.shim_ps_status(0, 1, 1, 0) == 3 and shim.shim_ps_status(1, 1, 0, 0) == 1 and shim.shim_ps_status(1, 0, 0, 0) == 4
