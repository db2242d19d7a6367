"""CPU: the per-lane routines of range proofs over weak-BB signatures in bulk (crypto_amd/csrc/smc_kernels.hip.h: own_scalars, col_run, merge_weight, fq_neg_words,
stage_src, proof_verdict, ref_position) compiled for the host with the FP29_CHECK operand asserts (tests/native/smc_dev_host_shim.cpp, a stand-alone host build) and
driven as k_smc_own, k_smc_stage, k_smc_merge_weights, k_smc_verdict, k_smc_col_sums, k_col_finish and the chunks of dock_smc.hip drive them, against the
big-integer model of tests/smc_model.py: one and two sides, l in {0, 1, 2, 16, 17, 64}, both input forms, the values 0, 1, r - 1, r and 2^256 - 1 among every kind
of scalar (the statement's constants too), proof counts on both sides of a lane's run (15, 16, 17) and of a wave (63, 64, 65), forced chunks, the batching
scalars 1, 2 and r - 1, the y-flip, and the verdict routine on planted flags.  A green run shows the values are right and that no product — the 65-term inner
product of a side among them — leaves fr_mul's operand contract."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import smc_model as SM
from bbs_model import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "smc_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libsmc_dev_host_shim.so")
R2 = pow(2, 256, R)
TOP = (1 << 256) - 1
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
LS = [0, 1, 2, 16, 17, 64]
p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC, os.path.join(HERE, "native", "col_frame_host.hpp")] + [os.path.join(CSRC, h) for h in ("fr29.hip.h", "col_sums.hip.h", "bbs_routines.hip.h", "smc_kernels.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.shim_smc_own.argtypes = [vp, vp, vp, vp, i, i, i, sz, vp]
    L.shim_smc_stage.argtypes = [vp, vp, vp, vp, i, i, sz, vp, vp, vp, vp]
    L.shim_smc_verdict.argtypes = [vp, vp, vp, i, i, i, sz, vp, vp]
    L.shim_smc_merge_weights.argtypes = [vp, i, i, i, sz, vp]
    L.shim_smc_columns.argtypes = [vp, vp, i, i, i, sz, sz, sz, vp, vp, vp, vp, vp, vp]
    L.shim_smc_fq_neg.argtypes = [vp, vp]
    L.shim_smc_ref_position.argtypes = [i, i, C.c_uint]
    for f in (L.shim_smc_own, L.shim_smc_stage, L.shim_smc_verdict, L.shim_smc_merge_weights, L.shim_smc_columns, L.shim_smc_fq_neg):
        f.restype = None
    L.shim_smc_ref_position.restype = C.c_uint
    return L


def words(vals, k=8):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for v in vals for i in range(k)], dtype=np.uint32)


def ints(w, k=8):
    a = w.reshape(-1, k).astype(object)
    return [sum(int(x) << (32 * i) for i, x in enumerate(row)) for row in a]


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def form(vals, mont):
    return words([v * R2 % R for v in vals] if mont else vals) if vals else np.zeros(8, np.uint32)


def scenario(sides, l, rows, seed, mont):
    """`rows` proofs' scalars and a statement of arbitrary constants (the points play no part here) with the edge values spread over every kind of scalar:
    0, 1, r - 1 in both forms, r and 2^256 - 1 as canonical words.  Returns the raw values the kernels are handed, the statement and the proofs of the model
    (which reduces what it reads)"""
    rng = np.random.default_rng(seed)
    D = sides * l
    edges = [0, 1, R - 1] + ([] if mont else [R, TOP])
    w, consts = rand(rng, l), [rand(rng, 3) for _ in range(sides)]
    for k, v in enumerate(edges):
        if l:
            w[(3 * k) % l] = v
        consts[k % sides][k % 3] = v
    raw = [dict(c=rand(rng, 1)[0], zr=rand(rng, sides), z=rand(rng, 2 * D)) for _ in range(rows)]
    for k, v in enumerate(edges):
        raw[k % rows]["c"] = v
        raw[(k + 1) % rows]["zr"][k % sides] = v
        if D:
            raw[(k + 2) % rows]["z"][(5 * k) % (2 * D)] = v
            raw[rows - 1]["z"][2 * ((k * 7) % D) + 1] = v
    if l:
        raw[0]["z"][1:2 * l:2] = [R - 1] * l                              # the longest inner product at its largest: every z2 of side 0 is r - 1 ...
    st = SM.Statement.raw(sides, l, w, consts)
    proofs = [SM.Proof(0, q["c"], [0] * sides, q["zr"], [SM.Digit(0, 0, 0, q["z"][2 * d], q["z"][2 * d + 1]) for d in range(D)]) for q in raw]
    return raw, (w, consts), st, proofs


def arrays(raw, stmt, mont):
    w, consts = stmt
    flat = [v for t in consts for v in t] + [0] * (3 * (2 - len(consts))) + w
    return form([q["c"] for q in raw], mont), form([v for q in raw for v in q["zr"]], mont), form([v for q in raw for v in q["z"]], mont), form(flat, mont)


def own_words(shim, raw, stmt, sides, l, mont):
    own = np.zeros(8 * 4 * len(raw) * sides * (l + 1), np.uint32)
    shim.shim_smc_own(*map(p_, arrays(raw, stmt, mont)), sides, l, mont, len(raw), p_(own))
    return own


def launcher_run():
    hdr = open(os.path.join(CSRC, "col_launch.hip.h")).read()
    return int(re.search(r"\bCOL_RUN = (\d+)\b", hdr).group(1))


def test_the_constants_are_the_launchers():
    assert launcher_run() == 16
    src = open(os.path.join(CSRC, "k_smc.hip")).read()
    assert "colk::col_blocks(rows * eq_count(sides, l))" in src and "colk::COL_RUN" in src and "dim3(256)" in src      # what the shim drives
    assert "i0 * eq_count(sides, l), i0 * digit_count(sides, l)" in src                                                          # the chunk's first exponents
    hdr = open(os.path.join(CSRC, "smc_launch.hip.h")).read()
    assert "SMC_EACH_SLICES = 4096, SMC_BATCH_EQS = 16384" in hdr and "SMC_MAX_L = 64" in hdr and "SMC_STMT_CONSTS = 6" in hdr


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("sides", [1, 2])
@pytest.mark.parametrize("l", LS)
def test_own_scalars(shim, l, sides, mont):
    """k_smc_own: canonical words below r of (a c, b c + sum w z2, e zr, -1) per side and (z1, -z2, -c, -1) per digit; every edge value among the rows"""
    for rows in (1, 15, 16, 17) if l > 2 else (1, 2, 15, 16, 17, 63, 64, 65):
        raw, stmt, st, proofs = scenario(sides, l, rows, 100 * rows + 10 * l + sides, mont)
        want = [v for p in proofs for v in p.own(st)]
        assert ints(own_words(shim, raw, stmt, sides, l, mont)) == want and max(want) < R, rows


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("rho", [1, 2, R - 1])
@pytest.mark.parametrize("sides", [1, 2])
def test_batch_columns_and_weights(shim, sides, rho, mont):
    """k_smc_col_sums / k_col_finish: the coefficients of g1, g, h, the weights over C, D and the digits' points, +-rho^slice, for proof counts on both sides
    of a lane's run, of a wave and of a block of 256 x 16 equations, in one chunk and in chunks that end inside a run"""
    run = launcher_run()
    shapes = [(0, 1, (1,)), (0, 17, (17, 5)), (0, 4097, (4097, 4096)), (1, 15, (15, 7)), (1, 16, (16,)), (1, 17, (17, 16)), (1, 63, (63, 16)), (1, 64, (64, 17)), (1, 65, (65, 64)),
              (2, 65, (65, 11)), (16, 17, (17, 3)), (17, 16, (16, 15)), (64, 3, (3, 2)), (64, 65, (65, 64)), (2, 1366, (1366, 683))]
    for l, rows, chunks in shapes:
        if mont and rows > 100:
            continue
        raw, stmt, st, proofs = scenario(sides, l, rows, 7 * rows + l + sides, mont)
        own = own_words(shim, raw, stmt, sides, l, mont)
        S, ws, wdig, tp, tn = SM.batch(st, proofs, rho)
        D = sides * l
        for chunk in chunks:
            oc, owc, owd = np.zeros(24, np.uint32), np.zeros(8 * rows, np.uint32), np.zeros(8 * rows * sides, np.uint32)
            og, op, on = (np.zeros(8 * max(k * rows * D, 1), np.uint32) for k in (3, 1, 1))
            shim.shim_smc_columns(p_(own), p_(form([rho], mont)), sides, l, mont, rows, chunk, run, p_(oc), p_(owc), p_(owd), p_(og), p_(op), p_(on))
            assert ints(oc) == S, (l, rows, chunk)
            assert ints(owc) + ints(owd) == ws, (l, rows, chunk)
            if D:
                assert ints(og) == wdig and ints(op) == tp and ints(on) == tn, (l, rows, chunk)
                assert tp[-1] == pow(rho, rows * D - 1, R)


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("sides", [1, 2])
def test_merge_weights(shim, sides, mont):
    """k_smc_merge_weights: random_i^d twice over, d side-major; random in {1, 2, r - 1} and the edge values among the rows"""
    for l in LS[1:]:
        rows, D = 17, sides * l
        rnd = ([1, 2, R - 1] + ([] if mont else [R + 5, TOP]) + rand(np.random.default_rng(l), rows))[:rows]
        tw = np.zeros(8 * 2 * rows * D, np.uint32)
        shim.shim_smc_merge_weights(p_(form(rnd, mont)), sides, l, mont, rows, p_(tw))
        want = [pow(x % R, d, R) for x in rnd for d in range(D)]
        assert ints(tw) == want + want, l


@pytest.mark.parametrize("sides", [1, 2])
@pytest.mark.parametrize("l", [0, 1, 2, 17])
def test_staging_lays_out_bases_sides_and_flags(shim, l, sides):
    """k_smc_stage's routine: every slot takes the point the layout names ([C, g, h, D_s] per side, [g1, A', Abar, T] per digit), the pairing's sides are A' and
    minus Abar, and the flags mark zero words — identities at every position among the rows"""
    rng = np.random.default_rng(77 + l + sides)
    rows, D = 17, sides * l
    pt = lambda: [int.from_bytes(rng.bytes(60), "little") % P for _ in range(2)]
    Cs, Ds = [pt() for _ in range(rows)], [[pt() for _ in range(sides)] for _ in range(rows)]
    dig = [[[pt() for _ in range(3)] for _ in range(D)] for _ in range(rows)]
    Cs[2], Ds[3][sides - 1] = [0, 0], [0, 0]
    if D:
        for k in range(3):
            dig[4 + k][(k * 5) % D][k] = [0, 0]                           # one identity at every position
        dig[8][D - 1] = [[0, 0]] * 3
        dig[9][0][1][1] = 1                                               # y = 1 flips to p - 1
    shared = [pt() for _ in range(3)]
    w12 = lambda pts: words([c for q in pts for c in q], 12) if pts else np.zeros(24, np.uint32)
    bases, pa, pb = np.zeros(rows * sides * (l + 1) * 4 * 24, np.uint32), np.zeros(max(rows * D, 1) * 24, np.uint32), np.zeros(max(rows * D, 1) * 24, np.uint32)
    skip = np.full(max(2 * rows * D, 1), 9, np.uint8)
    shim.shim_smc_stage(p_(w12(Cs)), p_(w12([q for r in Ds for q in r])), p_(w12([q for r in dig for d in r for q in d])), p_(w12(shared)), sides, l, rows, p_(bases), p_(pa), p_(pb), p_(skip))
    g1, g, h = shared
    want, want_a, want_b = [], [], []
    for i in range(rows):
        for s in range(sides):
            want += [Cs[i], g, h, Ds[i][s]]
        for d in dig[i]:
            want += [g1, d[0], d[1], d[2]]
            want_a.append(d[0])
            want_b.append([d[1][0], (P - d[1][1]) % P])
    got = lambda a: [list(x) for x in zip(*[iter(ints(a, 12))] * 2)]
    assert got(bases) == want
    if D:
        assert got(pa) == want_a and got(pb) == want_b
        zero = lambda q: 1 if q == [0, 0] else 0
        assert skip[:rows * D].tolist() == [zero(d[0]) for r in dig for d in r] and skip[rows * D:].tolist() == [zero(d[1]) for r in dig for d in r]
        assert sum(skip[:rows * D]) == 2 and sum(skip[rows * D:]) == 2


def test_base_field_words_and_the_order_of_errors(shim):
    """-y = p - y (zero stays zero); the reference's position of every digit; and (status, detail) on planted flags: a failed side wins, the smallest 4 q + k
    among the bad digits, the merged check last"""
    rng = np.random.default_rng(11)
    ys = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, (1 << 380) + 12345, 0xFFFFFFFF, 1 << 32, (1 << 352) - 1] + [int.from_bytes(rng.bytes(60), "little") % P for _ in range(20)]
    for y in ys:
        out = np.zeros(12, np.uint32)
        shim.shim_smc_fq_neg(p_(words([y], 12)), p_(out))
        assert ints(out, 12) == [(P - y) % P], hex(y)
    for sides in (1, 2):
        for l in LS[1:]:
            st = SM.Statement.raw(sides, l, [0] * l, [(0, 0, 0)] * sides)
            assert [shim.shim_smc_ref_position(sides, l, d) for d in range(sides * l)] == [st.ref_position(d) for d in range(sides * l)]
            assert sorted(st.ref_position(d) for d in range(sides * l)) == list(range(sides * l))
    for sides, l in ((1, 0), (2, 0), (1, 1), (1, 5), (2, 3), (2, 64)):
        M, D = sides * (l + 1), sides * l
        st = SM.Statement.raw(sides, l, [0] * l, [(0, 0, 0)] * sides)
        rows = 40
        seg, pair, skip = (rng.random((rows, M)) > 0.15).astype(np.uint8), (rng.random((rows, max(D, 1))) > 0.15).astype(np.uint8), (rng.random((2, rows, max(D, 1))) < 0.1).astype(np.uint8)
        seg[0], pair[0], skip[0, 0] = 1, 1, 0                             # a clean proof
        seg[1], pair[1], skip[0, 1] = 1, 0, 0                             # pairings alone
        for merged in (0, 1):
            if merged and not D:
                continue
            pr = np.ascontiguousarray(pair[:, 0] if merged else pair[:, :D])
            status, detail = np.full(rows, 9, np.uint8), np.full(rows, -9, np.int32)
            shim.shim_smc_verdict(p_(seg), p_(pr), p_(np.ascontiguousarray(skip[:, :, :D])), sides, l, merged, rows, p_(status), p_(detail))
            for i in range(rows):
                bad_side = [s for s in range(sides) if not seg[i, s]]
                cands = [4 * st.ref_position(d) + (1 if skip[0, i, d] else 2 if not seg[i, sides + d] else 3)
                         for d in range(D) if skip[0, i, d] or not seg[i, sides + d] or (not merged and not pair[i, d])]
                want = (1, bad_side[0] + 1) if bad_side else (2, min(cands)) if cands else (3, 0) if merged and not pair[i, 0] else (0, 0)
                assert (int(status[i]), int(detail[i])) == want, (sides, l, merged, i)
