"""The device arithmetic one function at a time, at the limb edges, against big integers.

Every other GPU test drives a whole entry point with seeded random points and scalars, so the field code only ever sees uniformly random operands; the
host tests (test_device_code_on_host.py) see edge operands but run what g++ made of the headers, and cannot run the lane-shared forms at all.  Here the
edge operands go through the functions compiled for the device, one function per kernel (crypto_amd/csrc/selftest_kernels.hip.h, the development twin's
dgpu_selftest_arith), and every output is compared with Python integers and bls12_381_model only.

Two halves over the SAME operand tables and expectations:
  * test_host_*: the wrappers built for the host under the FP29_CHECK bound tracker (tests/native/fp29_host_shim.cpp shim_selftest_arith).  No GPU.  It
    shows the expectations are right and the operands are inside each function's contract: an (op, stress) pair is in a table only because this half runs
    it without an assertion.  The lane-shared forms have no host build; their operands are those of their one-lane twins.
  * test_gpu_* (-m gpu): the same rows on the device.  A failure that the host half does not share points at code generation or at a lane exchange.
Rows interleave the operand classes (neighbouring lanes diverge in data-dependent branches) and their number is no multiple of 64 (a partial last wave).

The layer above the field and curve headers follows the same pattern:
  * test_host_gt_ops / test_gpu_gt_ops: the six-lane group functions of gt_kernels.hip.h (selftest_gt_kernels.hip.h) — gt_get_abi / gt_put / gt_get / gt_put_abi,
    gt_conj, gt_neg, gt_mul (also aliased, as the Miller tail squares), gt_cyc_sqr, gt_frob1, gt_frob2, gt_inv, gt_exp_by_x, gt_final_exp, gt_in_cyclotomic /
    gt_in_gt, gt_shrink on raw limbs up to the edge of its contract, k_miller_tail's load-shrink-square-multiply step, gt_signed_digits.  The host half runs
    the wrappers with six threads as the lanes (tests/native/gt_dev_host_shim.cpp shim_selftest_gt); the device runs them behind GT_GROUP_PROLOGUE with 1, 3
    and 10 groups per wave, and a row count that is no multiple of 3, 10 or 64, so GtLanesDev's slot offsets, ballots and early lane exits are all taken.
    Elements carry zero, one and p - 1 coefficients, single w^e, subfield elements and equal / opposite neighbours: what a wrong select or constant needs to show.
  * test_host_line_steps / test_gpu_line_steps: line_dbl_step and line_add_step against a transcription of the ark-ec formulas written here (which
    test_host_line_transcription_is_the_miller_loops_step ties to the Miller loop); line_dbl_step_fast, line_dbl_step_ws and line_add_step_ws on the host only.
Not covered per function: the lane-distributed line kernels (whole Miller loops only) and, on the device, one-lane G2 chains.
"""
import ctypes as C
import functools
import os
import random
import subprocess
import numpy as np
import pytest
import bls12_381_model as M
import util as U

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "crypto_amd", "csrc")
SRC = os.path.join(HERE, "native", "fp29_host_shim.cpp")
SO = os.path.join(HERE, "native", "libfp29_host_shim.so")
GT_SRC = os.path.join(HERE, "native", "gt_dev_host_shim.cpp")
GT_SO = os.path.join(HERE, "native", "libgt_dev_host_shim.so")
P, R = M.P, M.R
MAXP = 24                                   # ST_MAXP: points per chain row

# name: (number in selftest_kernels.hip.h, u64 words in, u64 words out per row, has a host build)
_CH1, _CH2 = 1 + MAXP * 12, 1 + MAXP * 24
OPS = {
    "fp_roundtrip": (0, 6, 6, 1), "fp_mul": (1, 12, 6, 1), "fp_sqr": (2, 6, 6, 1), "fp_mul2": (3, 24, 6, 1), "fp_mul_sub": (4, 24, 6, 1), "fp_mul12": (5, 6, 6, 1),
    "fp_canon": (6, 6, 7, 1), "fp_iszero": (7, 12, 1, 1), "fp_inv": (8, 6, 6, 1), "fp_submul": (9, 18, 6, 1),
    "fs_roundtrip": (16, 6, 6, 1), "fs_mul": (17, 12, 6, 1), "fs_sqr": (18, 6, 6, 1), "fs_mul2": (19, 24, 6, 1), "fs_mul_sub": (20, 24, 6, 1), "fs_neg": (21, 12, 12, 1),
    "fs_bal": (22, 12, 6, 1), "fs_bal_wide": (23, 18, 6, 1), "fs_iszero": (24, 12, 1, 1), "fs_via_fp": (25, 6, 12, 1), "fs_submul": (26, 18, 6, 1),
    "fp2_mul": (32, 24, 12, 1), "fp2_sqr": (33, 12, 12, 1), "fs2_mul": (34, 24, 12, 1), "fs2_sqr": (35, 12, 12, 1), "fp2_inv": (36, 12, 12, 0),
    "fp2h_mul": (40, 24, 12, 0), "fp2h_sqr": (41, 12, 12, 0), "fp2h_mul_sub": (42, 48, 12, 0), "fp2h_sqr_m": (43, 12, 12, 0), "fp2h_mul_xi_n": (44, 12, 12, 0),
    "fp2h_inv": (45, 12, 12, 0), "fs2h_mul": (46, 24, 12, 0), "fs2h_mul_two": (47, 48, 24, 0), "fs2h_sqr": (48, 12, 12, 0), "fs2h_mul_sub": (49, 48, 12, 0),
    "fr_roundtrip": (56, 4, 4, 1), "fr_mul": (57, 8, 4, 1), "fr_butterflies": (58, 12, 8, 1), "fr_canon": (59, 4, 5, 1), "fr_inv": (60, 4, 4, 1), "fr_batch_inv": (61, None, None, 1),
    "g1_madd": (64, _CH1, 24, 1), "g1_tree": (65, _CH1, 24, 1), "g1_dbl": (66, _CH1, 24, 1),
    "g1s_madd": (68, _CH1, 24, 1), "g1s_tree": (69, _CH1, 24, 1), "g1s_dbl": (70, _CH1, 24, 1), "g1s_tree_rounds": (71, _CH1, 24, 1), "g1s_dbl_rounds": (72, _CH1, 24, 1),
    "g2_madd": (74, _CH2, 48, 1), "g2_tree": (75, _CH2, 48, 1), "g2_dbl": (76, _CH2, 48, 1),
    "g2s_madd": (78, _CH2, 48, 1), "g2s_madd_early": (79, _CH2, 48, 1), "g2s_tree": (80, _CH2, 48, 1), "g2s_dbl": (81, _CH2, 48, 1), "g2s_tree_rounds": (82, _CH2, 48, 1),
    "g2s_dbl_rounds": (83, _CH2, 48, 1),
    "g1_madd_2l": (88, _CH1, 24, 0), "g1_dbl_2l": (89, _CH1, 24, 0), "g2_madd_4l": (90, _CH2, 48, 0), "g2_dbl_4l": (91, _CH2, 48, 0), "g1_phi": (92, _CH1, 24, 0),
    "g1_to_affine": (93, _CH1, 13, 0), "g2h_to_affine": (95, _CH2, 25, 0),
    "f12_mul": (100, 144, 72, 1), "f12_mul_roles": (101, 144, 72, 1), "f12_mul_by_014": (102, 108, 72, 1), "line_dbl": (104, 36, 72, 1), "line_add": (105, 60, 72, 1),
    "gt_roundtrip": (110, 72, 156, 1), "gt_conj": (111, 72, 72, 1), "gt_neg": (112, 72, 72, 1), "gt_mul": (113, 144, 72, 1), "gt_sqr_by_mul": (114, 72, 72, 1),
    "gt_cyc_sqr": (115, 72, 72, 1), "gt_frob1": (116, 72, 72, 1), "gt_frob2": (117, 72, 72, 1), "gt_inv": (118, 72, 72, 1), "gt_exp_by_x": (119, 72, 72, 1),
    "gt_final_exp": (120, 72, 73, 1), "gt_membership": (121, 72, 1, 1), "gt_shrink": (122, 84, 156, 1), "gt_tail_step": (123, 168, 72, 1), "gt_digits": (124, 4, 9, 1),
}
# the six-lane group ops (ST_GT_OP of selftest_gt_kernels.hip.h): stress = reps | G << 8; on the host they run through shim_selftest_gt
GT_SIX = {k for k in OPS if k.startswith("gt_") and k != "gt_digits"}
GT_GROUPS = (1, 3, 10)                      # groups per wave the twin accepts


# ---- the two backends ----
@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("fp29.hip.h", "fp30s.hip.h", "fs2_pair.hip.h", "fp2_29.hip.h", "ec29.hip.h", "pairing29.hip.h", "fr29.hip.h",
                                                      "fp_safegcd.hip.h", "selftest_kernels.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.shim_selftest_arith.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]
    L.shim_line_steps.argtypes = L.shim_selftest_arith.argtypes
    return L


def _run(fn, name, stress, rows, out_words=None):
    op, iw, ow, _ = OPS[name]
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    iw = rows.shape[1] if iw is None else iw
    ow = out_words if ow is None else ow
    assert rows.shape[1] == iw, (name, rows.shape, iw)
    out = np.zeros((len(rows), ow), np.uint64)
    rc = fn(op, stress, rows.ctypes.data_as(C.c_void_p), iw, len(rows), out.ctypes.data_as(C.c_void_p), ow)
    assert rc == 0, (name, stress, rc)
    return out


@pytest.fixture(scope="module")
def gt_shim():
    """tests/native/gt_dev_host_shim.cpp: six threads as the six lanes of a group (the library test_gt_device_code_on_host.py builds, same flags)"""
    deps = [GT_SRC] + [os.path.join(CSRC, f) for f in ("gt_kernels.hip.h", "pairing29.hip.h", "fp29.hip.h", "fp2_29.hip.h", "fp_safegcd.hip.h", "selftest_kernels.hip.h",
                                                         "selftest_gt_kernels.hip.h")]
    if not os.path.exists(GT_SO) or any(os.path.getmtime(d) > os.path.getmtime(GT_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", GT_SO, GT_SRC])
    L = C.CDLL(GT_SO)
    L.shim_selftest_gt.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]
    return L


def host_backend(shim):
    return lambda name, stress, rows, out_words=None: _run(shim.shim_selftest_arith, name, stress, rows, out_words)


def gt_host_backend(gt_shim):
    return lambda name, stress, rows, out_words=None: _run(gt_shim.shim_selftest_gt, name, stress, rows, out_words)


def gpu_backend(T):
    return lambda name, stress, rows, out_words=None: _run(T.dgpu_selftest_arith, name, stress, rows, out_words)


# ---- encodings (plain integers <-> ABI words) ----
def words(vals, nbytes):
    """ints -> [n, nbytes / 8] u64, little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(nbytes, "little") for v in vals), dtype=np.uint64).reshape(len(vals), nbytes // 8).copy()


def enc_fp(vals):
    return words([v * M.FP_R % P for v in vals], 48)


def enc_f2(vals):
    return np.hstack([enc_fp([v[0] for v in vals]), enc_fp([v[1] for v in vals])])


def cols(tuples, enc=enc_fp):
    """rows of k operands -> [n, k * words]"""
    return np.hstack([enc([t[j] for t in tuples]) for j in range(len(tuples[0]))])


def limbs29(v, n):
    """the n 29-bit limbs of v as n u32 packed into u64 words"""
    l = [(v >> (29 * i)) & (2 ** 29 - 1) for i in range(n)]
    return [l[2 * i] | (l[2 * i + 1] << 32) for i in range(n // 2)]


def interleave(*classes):
    """round-robin merge: neighbouring rows come from different operand classes"""
    out, its = [], [iter(c) for c in classes]
    while its:
        for it in list(its):
            try:
                out.append(next(it))
            except StopIteration:
                its.remove(it)
    return out


def odd_rows(rows):
    """no multiple of 64, so the last wave is partial (for every lanes-per-row of 1, 2 and 4)"""
    while len(rows) % 64 == 0 or (2 * len(rows)) % 64 == 0 or (4 * len(rows)) % 64 == 0:
        rows = rows + [rows[len(rows) // 2]]
    return rows


def mismatch(got, want, rows, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        w = int(np.nonzero(got[i] != want[i])[0][0])
        raise AssertionError("%s: %d of %d rows differ; first: row %d, word %d, operands %s" % (what, len(bad), len(got), i, w, [hex(x) if isinstance(x, int) else x for x in rows[i]]))


# ---- edge operands ----
def _patterns(mod, bits_list, top):
    """limb patterns in the given radices, reduced: every limb full, every limb 2^(b-1) and 2^(b-1) - 1 (the signed boundary), alternating zero / full"""
    out = []
    for b in bits_list:
        n = (top + b - 1) // b
        for limb in (2 ** b - 1, 2 ** (b - 1), 2 ** (b - 1) - 1):
            out.append(sum(limb << (b * i) for i in range(n)) % 2 ** top % mod)
        out.append(sum((2 ** b - 1) << (b * i) for i in range(0, n, 2)) % 2 ** top % mod)
        out.append(sum((2 ** b - 1) << (b * i) for i in range(1, n, 2)) % 2 ** top % mod)
    return out


def _images(vals, mod, radices):
    """each value as it stands and as the operand whose Montgomery image (x * 2^k) it is: the kernels compute on the images"""
    out = list(vals)
    for k in radices:
        inv = pow(2 ** k, -1, mod)
        out += [v * inv % mod for v in vals]
    return out


def _uniq(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v); out.append(v)
    return out


FP_BASE = [0, 1, 2, 3, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 2 ** 29, 2 ** 29 - 1, 2 ** 30, 2 ** 58 + 1, 2 ** 360, 2 ** 360 - 1, 2 ** 377, 2 ** 377 - 1, 2 ** 380, P - 2 ** 29]
# Montgomery radices: 2^406 (fp29.hip.h), 2^390 (fp30s.hip.h), 2^384 (the ABI words themselves)
FP_CORE = _uniq(FP_BASE + _images(_patterns(P, (29, 30), 381), P, (406, 390))[10:] + _patterns(P, (29, 30), 381))          # all ordered pairs of these
FP_EXT = _uniq(_images([s * 2 ** (29 * k) % P for k in range(14) for s in (1, -1)] + [s * 2 ** (30 * k) % P for k in range(13) for s in (1, -1)], P, (406, 390, 384)))
FP_SMALL_BITS = list(range(1, 381, 7))          # random values of every magnitude (the inversion's division steps end early)
FR_BASE = [0, 1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 2 ** 29, 2 ** 29 - 1, 2 ** 30, 2 ** 58 + 1, 2 ** 232, 2 ** 232 - 1, 2 ** 254, 2 ** 254 - 1, R - 2 ** 29]
FR_OVER = [R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 2 ** 255, 2 ** 256 - 1, 2 ** 256 - 2 ** 29]         # values >= r in the 256-bit words
FR_CORE = _uniq(FR_BASE + _images(_patterns(R, (29, 32), 255), R, (290, 256))[10:] + _patterns(R, (29, 32), 255)) + FR_OVER
FR_EXT = _uniq(_images([s * 2 ** (29 * k) % R for k in range(9) for s in (1, -1)], R, (290, 256)))


@functools.lru_cache(None)
def fp_tables():
    """(unary operands, ordered pairs, windows of 3, windows of 4) over Fp: every ordered pair of the core set (a = b and a = p - b among them), the extended
    set against itself, its negative and its neighbour, and 2000 seeded random pairs — interleaved"""
    rng = random.Random(20261)
    core = [(a, b) for a in FP_CORE for b in FP_CORE]
    ext = [t for i, x in enumerate(FP_EXT) for t in ((x, x), (x, (P - x) % P), (x, FP_EXT[(i + 1) % len(FP_EXT)]))]
    rnd = [(rng.randrange(P), rng.randrange(P)) for _ in range(2000)]
    pairs = odd_rows(interleave(core, ext, rnd))
    un = odd_rows(interleave(FP_CORE + FP_EXT, [rng.randrange(P) for _ in range(300)], [rng.randrange(1 << k) for k in FP_SMALL_BITS]))
    w3 = odd_rows([(un[i], un[i + 1], un[i + 2]) for i in range(len(un) - 2)])
    w4 = [(un[i], un[i + 1], un[i + 2], un[i + 3]) for i in range(len(un) - 3)]
    # a b = c d exactly (the difference is zero), and a b = -c d
    w4 = odd_rows(interleave(w4, [t for a, b in zip(FP_CORE, FP_CORE[1:]) for t in ((a, b, a, b), (a, b, b, a), (a, b, (P - a) % P, b))]))
    return un, pairs, w3, w4


@functools.lru_cache(None)
def fr_tables():
    rng = random.Random(20262)
    core = [(a, b) for a in FR_CORE for b in FR_CORE]
    ext = [t for i, x in enumerate(FR_EXT) for t in ((x, x), (x, (R - x) % R), (x, FR_EXT[(i + 1) % len(FR_EXT)]))]
    rnd = [(rng.randrange(R), rng.randrange(R)) for _ in range(2000)]
    pairs = odd_rows(interleave(core, ext, rnd))
    un = odd_rows(interleave(FR_CORE + FR_EXT, [rng.randrange(R) for _ in range(300)], [rng.randrange(1 << 256) for _ in range(40)]))
    w3 = odd_rows([(un[i], un[i + 1], un[i + 2]) for i in range(len(un) - 2)])
    return un, pairs, w3


@functools.lru_cache(None)
def f2_tables():
    rng = random.Random(20263)
    # component pairs that hit a0 = a1, a0 = -a1 (the factors of the square), zero halves, and the limb patterns in either half
    e = FP_CORE[:24] + FP_CORE[-10:]
    edge = [(a, b) for a in e[:12] for b in e[:12]] + [(a, a) for a in e] + [(a, (P - a) % P) for a in e] + [(a, e[(i + 5) % len(e)]) for i, a in enumerate(e)]
    un = odd_rows(interleave(edge, [(rng.randrange(P), rng.randrange(P)) for _ in range(200)]))
    pairs = odd_rows(interleave([(a, b) for a in edge[::3] for b in edge[1::7]], [(a, a) for a in edge], [(a, (a[0], (P - a[1]) % P)) for a in edge],
                                [((rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))) for _ in range(500)]))
    w4 = [(un[i], un[i + 1], un[i + 2], un[i + 3]) for i in range(len(un) - 3)]
    w4 = odd_rows(interleave(w4, [t for a, b in zip(edge, edge[1:]) for t in ((a, b, a, b), (a, b, b, a))]))
    return un, pairs, w4


# ---- the field families: (op, stress) tables, run by either backend ----
def check_fp(run):
    un, pairs, w3, w4 = fp_tables()
    for f in ("fp", "fs"):
        mismatch(run(f + "_roundtrip", 1, enc_fp(un)), enc_fp(un), [(a,) for a in un], f + "_roundtrip")
        mismatch(run(f + "_sqr", 1, enc_fp(un)), enc_fp([a * a % P for a in un]), [(a,) for a in un], f + "_sqr")
        mismatch(run(f + "_mul", 1, cols(pairs)), enc_fp([a * b % P for a, b in pairs]), pairs, f + "_mul")
        mismatch(run(f + "_mul2", 1, cols(w4)), enc_fp([(a * b + c * d) % P for a, b, c, d in w4]), w4, f + "_mul2")
        mismatch(run(f + "_mul_sub", 1, cols(w4)), enc_fp([(a * b - c * d) % P for a, b, c, d in w4]), w4, f + "_mul_sub")
        mismatch(run(f + "_submul", 1, cols(w3)), enc_fp([(a - b) * c % P for a, b, c in w3]), w3, f + "_submul")
        z = run(f + "_iszero", 1, cols(pairs))[:, 0]
        for (a, b), flags in zip(pairs, z):
            assert bool(flags & 2) == (a == b), (f + "_iszero: exact", hex(a), hex(b), int(flags))
            assert (flags & 1) or not (flags & 2), (f + "_iszero: the cheap test must not miss a zero", hex(a), hex(b), int(flags))


def check_fp_lazy(run):
    """operands added to themselves un-normalised before the function (the stress levels the bound tracker accepts)"""
    un, pairs, w3, _ = fp_tables()
    for k in (1, 2, 5, 7):
        mismatch(run("fp_mul12", k, enc_fp(un)), enc_fp([12 * k * a % P for a in un]), [(a,) for a in un], "fp_mul12 k=%d" % k)
    for k in (1, 3, 7):
        want = words([w for a in un for w in limbs29(k * (a * 2 ** 406 % P) % P, 14)], 8).reshape(len(un), 7)
        mismatch(run("fp_canon", k, enc_fp(un)), want, [(a,) for a in un], "fp_canon k=%d" % k)
        mismatch(run("fp_inv", k, enc_fp(un)), enc_fp([pow(k * a, -1, P) if a else 0 for a in un]), [(a,) for a in un], "fp_inv k=%d" % k)
    # fs_bal takes two balanced terms (the tracker refuses 2 a - 2 b: a digit of 2^31 does not fit the carry pass), fs_bal_wide three
    mismatch(run("fs_bal", 1, cols(pairs)), enc_fp([(a - b) % P for a, b in pairs]), pairs, "fs_bal")
    mismatch(run("fs_bal_wide", 1, cols(w3)), enc_fp([(a - b - c) % P for a, b, c in w3]), w3, "fs_bal_wide")
    got = run("fs_neg", 1, cols(pairs))          # the sign of the second half: the low bit of b's ABI words
    flag = enc_fp([b for _, b in pairs])[:, 0] & np.uint64(1)
    want = np.hstack([enc_fp([(P - a) % P for a, _ in pairs]), enc_fp([(P - a) % P if s else a for (a, _), s in zip(pairs, flag)])])
    mismatch(got, want, pairs, "fs_neg / fs_cond_neg")
    mismatch(run("fs_via_fp", 1, enc_fp(un)), np.hstack([enc_fp(un), enc_fp(un)]), [(a,) for a in un], "fp_from_fs / fs_from_fp")


def check_f2(run, names):
    un, pairs, w4 = f2_tables()
    inv = lambda a: M.f2_inv(a) if a != (0, 0) else (0, 0)
    table = {
        "mul": (pairs, lambda a, b: M.f2_mul(a, b)), "sqr": (un, lambda a: M.f2_sqr(a)), "sqr_m": (un, lambda a: M.f2_sqr(a)), "mul_xi_n": (un, lambda a: M.f2_mul_xi(a)),
        "mul_sub": (w4, lambda a, b, c, d: M.f2_sub(M.f2_mul(a, b), M.f2_mul(c, d))), "inv": (un, inv),
    }
    for name in names:
        kind = name.split("_", 1)[1]
        if kind == "mul_two":
            got = run(name, 1, cols(w4, enc_f2))
            want = np.hstack([enc_f2([M.f2_mul(a, b) for a, b, _, _ in w4]), enc_f2([M.f2_mul(c, d) for _, _, c, d in w4])])
            mismatch(got, want, w4, name)
            continue
        rows, fn = table[kind]
        rows = [r if isinstance(r[0], tuple) else (r,) for r in rows]
        mismatch(run(name, 1, cols(rows, enc_f2)), enc_f2([fn(*r) for r in rows]), rows, name)


def enc_fr(vals):
    return words(vals, 32)


def check_fr(run):
    un, pairs, w3 = fr_tables()
    RI = pow(M.FR_R, -1, R)
    for mont in (0, 1):
        mismatch(run("fr_roundtrip", mont, enc_fr(un)), enc_fr([a % R for a in un]), [(a,) for a in un], "fr words mont=%d" % mont)
    mismatch(run("fr_mul", 0, cols(pairs, enc_fr)), enc_fr([a * b % R for a, b in pairs]), pairs, "fr_mul")
    mismatch(run("fr_mul", 1, cols(pairs, enc_fr)), enc_fr([a * b * RI % R for a, b in pairs]), pairs, "fr_mul (Montgomery words)")
    want = []
    for a, b, w in w3:
        x, y = a, b
        for _ in range(30):
            t = y * w % R
            x, y = (x + t) % R, (x - t) % R
        want.append((x, y))
    mismatch(run("fr_butterflies", 30, cols(w3, enc_fr)), cols(want, enc_fr), w3, "fr butterflies")
    for k in (1, 3, 7):
        want = words([w for a in un for w in limbs29(k * (a * 2 ** 290 % R) % R, 10)], 8).reshape(len(un), 5)
        mismatch(run("fr_canon", k, enc_fr(un)), want, [(a,) for a in un], "fr_canon k=%d" % k)
        mismatch(run("fr_inv", k, enc_fr(un)), enc_fr([pow(k * a, -1, R) if a % R else 0 for a in un]), [(a,) for a in un], "fr_inv k=%d" % k)
    nz = [a for a in un if a % R]
    for share in (1, 2, 3, 7, 8, 9):            # lane g of G inverts elements g, g + G, g + 2 G, ... with one fr_inv
        G = 67
        flat = (nz * (2 + G * share // len(nz)))[share:share + G * share]
        got = run("fr_batch_inv", share, enc_fr(flat).reshape(G, 4 * share), out_words=4 * share).reshape(G * share, 4)
        mismatch(got, enc_fr([pow(a, -1, R) for a in flat]), [(a,) for a in flat], "fr_batch_inv share=%d" % share)


# ---- Fp12 ----
@functools.lru_cache(None)
def f12_rows():
    rng = random.Random(20264)
    rnd = lambda: tuple(tuple((rng.randrange(P), rng.randrange(P)) for _ in range(3)) for _ in range(2))
    const = lambda v: tuple(tuple((v, v) for _ in range(3)) for _ in range(2))
    one = (((1, 0), (0, 0), (0, 0)), ((0, 0), (0, 0), (0, 0)))
    pat = _patterns(P, (29, 30), 381)
    mixed = tuple(tuple((pat[(2 * (3 * i + j)) % len(pat)], pat[(2 * (3 * i + j) + 1) % len(pat)]) for j in range(3)) for i in range(2))
    edge = [one, const(P - 1), const(0), const((P - 1) // 2), mixed, const(2 ** 380)]
    pairs = interleave([(a, b) for a in edge for b in edge], [(rnd(), rnd()) for _ in range(13)])
    f2s = lambda: (rng.randrange(P), rng.randrange(P))
    sparse = interleave([(a, (P - 1, P - 1), (0, 0), (pat[0], pat[3])) for a in edge] + [(a, (0, 0), (0, 0), (0, 0)) for a in edge[:2]], [(rnd(), f2s(), f2s(), f2s()) for _ in range(9)])
    return pairs, sparse


def _f12_flat(f):
    return [c for six in f for two in six for c in two]


def check_f12(run):
    pairs, sparse = f12_rows()
    enc12 = lambda fs: np.hstack([enc_fp([_f12_flat(f)[k] for f in fs]) for k in range(12)])
    rows = np.hstack([enc12([a for a, _ in pairs]), enc12([b for _, b in pairs])])
    srows = np.hstack([enc12([a for a, _, _, _ in sparse])] + [enc_f2([t[j] for t in sparse]) for j in (1, 2, 3)])
    for reps in (1, 2, 7):
        want = []
        for a, b in pairs:
            w = M.f12_mul(a, b)
            for _ in range(reps - 1):
                w = M.f12_mul(w, b)
            want.append(w)
        for name in ("f12_mul", "f12_mul_roles"):
            mismatch(run(name, reps, rows), enc12(want), [("pair %d" % i,) for i in range(len(pairs))], "%s reps=%d" % (name, reps))
        want = []
        for a, c0, c1, c4 in sparse:
            w = a
            for _ in range(reps):
                w = M.f12_mul_by_014(w, c0, c1, c4)
            want.append(w)
        mismatch(run("f12_mul_by_014", reps, srows), enc12(want), [("row %d" % i,) for i in range(len(sparse))], "f12_mul_by_014 reps=%d" % reps)


# ---- group law ----
CHAINS = [([], []), ([0], [0]), ([0], [1]), ([0, 1], [0, 0]), ([0, 0], [0, 0]), ([0, 0], [0, 1]), ([0, 0, 0], [0, 1, 0]),
          ([0, 1, 0, 1], [0, 0, 1, 1]), ([0] * 5, [0] * 5), ([1, 2, 3, 1, 2, 3], [0, 0, 0, 1, 1, 1]),
          ([1, 2, 3, 1, 2, 3, 5], [0, 0, 0, 1, 1, 1, 1]), (list(range(12)) * 2, [int(i % 3 == 0) for i in range(24)])]
TREES = [[0], [0, 1], [0, 0], [0, 1, 2, 3, 4], list(range(12)) * 2, [0, 1, 0, 1], [5] * 8]


class Group:
    def __init__(self, g):
        rng = random.Random(20265 + g)
        off = U.off_subgroup_points()
        if g == 1:
            self.add, self.neg, self.mul, gen, self.W, self.enc = M.g1_add, M.g1_neg, M.g1_mul, M.G1_GEN, 12, lambda p: np.concatenate([enc_fp([p[0]])[0], enc_fp([p[1]])[0]])
            odd = [off[k][0] for k in ("S", "-S", "T", "S11")]
        else:
            self.add, self.neg, self.mul, gen, self.W, self.enc = M.g2_add, M.g2_neg, M.g2_mul, M.G2_GEN, 24, lambda p: np.concatenate([enc_f2([p[0]])[0], enc_f2([p[1]])[0]])
            odd = [off[k][0] for k in ("T2", "S2")]
        rand = [self.mul(gen, rng.randrange(1, R)) for _ in range(12)]
        small = [self.mul(gen, k) for k in range(1, 7)] + [self.neg(self.mul(gen, k)) for k in (1, 2, 3)] + rand[:3]
        # off-subgroup points (S = (0, 2): x words all zero, order 3, so S + S = -S and S + S + S is the identity inside a chain), their negatives and sums
        mixed = (odd + [self.neg(q) for q in odd] + [self.add(odd[0], rand[0]), self.add(odd[-1], odd[-1])] + small + rand)[:12]
        self.palettes = [rand, small, mixed]
        rows = [(pal, idx, ng) for pal in self.palettes for idx, ng in CHAINS]
        allp = rand + small + mixed
        for _ in range(70):                     # random walks over all three palettes: repeats and negatives meet often
            n = rng.randrange(1, MAXP + 1)
            rows.append((allp, [rng.randrange(len(allp)) if rng.random() < .6 else rng.randrange(4) + 24 for _ in range(n)], [rng.randrange(2) for _ in range(n)]))
        self.chains = odd_rows(interleave(rows[:36], rows[36:]))
        trees = [(pal, idx, [0] * len(idx)) for pal in self.palettes for idx in TREES]
        # P + (-P) through the general addition, then + Q; and a tree of one repeated off-subgroup point
        trees += [([pal[0], self.neg(pal[0]), pal[3]], [0, 1][:n] + [2][:n - 2], [0] * n) for pal in self.palettes for n in (2, 3)]
        for _ in range(40):
            n = rng.randrange(1, MAXP + 1)
            trees.append((allp, [rng.randrange(len(allp)) for _ in range(n)], [0] * n))
        self.trees = odd_rows(trees)
        self.dbls = odd_rows([(q, k) for q in (rand[2], small[0], mixed[0], mixed[1], mixed[2], rand[5], mixed[-1]) for k in (1, 2, 16, 20)])

    def rows(self, table):
        out = np.zeros((len(table), 1 + MAXP * self.W), np.uint64)
        for r, (pal, idx, ng) in enumerate(table):
            out[r, 0] = len(idx) | (sum(s << i for i, s in enumerate(ng)) << 32)
            for i, j in enumerate(idx):
                out[r, 1 + self.W * i:1 + self.W * (i + 1)] = self.enc(pal[j])
        return out

    def dbl_rows(self):
        out = np.zeros((len(self.dbls), 1 + MAXP * self.W), np.uint64)
        for r, (q, k) in enumerate(self.dbls):
            out[r, 0] = k
            out[r, 1:1 + self.W] = self.enc(q)
        return out

    def sums(self, table):
        out = []
        for pal, idx, ng in table:
            acc = None
            for j, s in zip(idx, ng):
                acc = self.add(acc, self.neg(pal[j]) if s else pal[j])
            out.append(acc)
        return out

    def dec(self, o):
        """XYZZ words -> the model's affine point (None: the identity)"""
        if self.W == 12:
            X, Y, ZZ, ZZZ = [U.fp_int(o[6 * i:6 * i + 6]) for i in range(4)]
            if ZZ == 0 and X == 0:
                return None
            return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)
        f = lambda i: (U.fp_int(o[12 * i:12 * i + 6]), U.fp_int(o[12 * i + 6:12 * i + 12]))
        X, Y, ZZ, ZZZ = f(0), f(1), f(2), f(3)
        if ZZ == (0, 0) and X == (0, 0):
            return None
        return (M.f2_mul(X, M.f2_inv(ZZ)), M.f2_mul(Y, M.f2_inv(ZZZ)))


@functools.lru_cache(None)
def group(g):
    G = Group(g)
    return G, G.sums(G.chains), G.sums(G.trees), [G.mul(q, 1 << k) for q, k in G.dbls]


def points_equal(G, got, want, table, what):
    for i, (o, w) in enumerate(zip(got, want)):
        assert G.dec(o) == w, "%s: row %d (%s)" % (what, i, table[i][1:])


def check_group(run, g, ops):
    """ops: names by role — madd chains, trees, doubling chains (2^k P), shared doubling chains, phi, to_affine"""
    G, chain_sums, tree_sums, dbl_pts = group(g)
    for name in ops.get("madd", ()):
        points_equal(G, run(name, 1, G.rows(G.chains)), chain_sums, G.chains, name)
    for name in ops.get("tree", ()):
        points_equal(G, run(name, 1, G.rows(G.trees)), tree_sums, G.trees, name)
    for name in ops.get("dbl", ()):
        points_equal(G, run(name, 1, G.dbl_rows()), dbl_pts, [(None, d) for d in G.dbls], name)
    for name in ops.get("phi", ()):
        # beta: the cube root of unity with phi(G) = lambda G on the subgroup (checked here, through the model); phi(x, y) = (beta x, y) on the whole curve
        beta = next(b for b in (pow(c, (P - 1) // 3, P) for c in range(2, 20)) if b != 1 and (b * M.G1_GEN[0] % P, M.G1_GEN[1]) == M.g1_mul(M.G1_GEN, U.GLV_LAMBDA))
        points_equal(G, run(name, 1, G.rows(G.chains)), [None if q is None else (beta * q[0] % P, q[1]) for q in chain_sums], G.chains, name)
    for name in ops.get("affine", ()):
        got = run(name, 1, G.rows(G.chains))
        flag = lambda v: np.array([v], np.uint64)                      # (a plain list here would turn the whole row into floats)
        enc = lambda q: np.concatenate([np.zeros(G.W, np.uint64), flag(1)]) if q is None else np.concatenate([G.enc(q), flag(0)])
        mismatch(got, np.stack([enc(q) for q in chain_sums]), [t[1:] for t in G.chains], name)


G1_HOST = {"madd": ("g1_madd", "g1s_madd"), "tree": ("g1_tree", "g1s_tree", "g1s_tree_rounds"), "dbl": ("g1_dbl", "g1s_dbl", "g1s_dbl_rounds")}
G2_HOST = {"madd": ("g2_madd", "g2s_madd", "g2s_madd_early"), "tree": ("g2_tree", "g2s_tree", "g2s_tree_rounds"), "dbl": ("g2_dbl", "g2s_dbl", "g2s_dbl_rounds")}
G1_DEVICE = {"madd": ("g1_madd_2l",), "dbl": ("g1_dbl_2l",), "phi": ("g1_phi",), "affine": ("g1_to_affine",)}
G2_DEVICE = {"madd": ("g2_madd_4l",), "dbl": ("g2_dbl_4l",), "affine": ("g2h_to_affine",)}
F2_HOST = ("fp2_mul", "fp2_sqr", "fs2_mul", "fs2_sqr")
F2_DEVICE = ("fp2_inv", "fp2h_mul", "fp2h_sqr", "fp2h_mul_sub", "fp2h_sqr_m", "fp2h_mul_xi_n", "fp2h_inv", "fs2h_mul", "fs2h_mul_two", "fs2h_sqr", "fs2h_mul_sub")


# ---- the six-lane GT group arithmetic (gt_kernels.hip.h, gt_lanes.hip.h): expectations from bls12_381_model alone ----
F2Z = (0, 0)
F12_ZERO = ((F2Z,) * 3, (F2Z,) * 3)
X_BITS = bin(M.X_ABS)[3:]                    # the bits of |x| below the top one


GT_FIXED = [F12_ZERO, M.F12_ONE, (((P - 1, 0), F2Z, F2Z), (F2Z,) * 3)]          # zero, one, minus one


def enc12(fs):
    """model elements -> [n, 72] ABI words (tower order)"""
    return np.hstack([enc_fp([_f12_flat(f)[k] for f in fs]) for k in range(12)])


def from_w(c):
    """the element sum c[e] w^e: coefficient e = 2 j + i is the tower's c_i.c_j (lane e of a group holds c[e])"""
    return ((c[0], c[2], c[4]), (c[1], c[3], c[5]))


def w_coeffs(f):
    return [f[e & 1][e >> 1] for e in range(6)]


def gt_odd(rows):
    """no multiple of 3, of 10 or of 64: at every G the last wave is partial, and so is the last block's group count"""
    rows = list(rows)
    while len(rows) % 3 == 0 or len(rows) % 10 == 0 or len(rows) % 64 == 0:
        rows.append(rows[len(rows) // 2])
    return rows


def carried(v):
    """v as fully carried limbs of 29 bits, everything above bit 377 in the top one"""
    return [(v >> (29 * i)) & (2 ** 29 - 1) for i in range(13)] + [v >> 377]


def raw_words(limbs):
    """14 u32 limbs -> 7 u64 words"""
    return [limbs[2 * i] | (limbs[2 * i + 1] << 32) for i in range(7)]


def limbs_value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


@functools.lru_cache(None)
def gt_elements():
    """the element classes, interleaved: zero, one, minus one, every coefficient p - 1 and (p - 1) / 2; the six w^e alone and scaled by (1, 1); elements of Fp,
    Fp2, Fp6 (odd w-coefficients zero) and c1 w (even ones zero); limb patterns in either half; neighbouring coefficients equal / negatives of each other; random"""
    rng = random.Random(20266)
    f2r = lambda: (rng.randrange(P), rng.randrange(P))
    const = lambda v: from_w([(v, v)] * 6)
    pat = _patterns(P, (29, 30), 381)
    fixed = GT_FIXED + [const(P - 1), const((P - 1) // 2)]
    basis = [from_w([s if k == e else F2Z for k in range(6)]) for e in range(6) for s in ((1, 0), (1, 1))]
    sub = [from_w([(rng.randrange(P), 0)] + [F2Z] * 5), from_w([f2r()] + [F2Z] * 5), from_w([f2r(), F2Z, f2r(), F2Z, f2r(), F2Z]), from_w([F2Z, f2r(), F2Z, f2r(), F2Z, f2r()])]
    limb = [from_w([(pat[(2 * e) % len(pat)], rng.randrange(P)) for e in range(6)]), from_w([(rng.randrange(P), pat[(2 * e + 1) % len(pat)]) for e in range(6)]),
            from_w([(pat[e], pat[(e + 5) % len(pat)]) for e in range(6)])]
    a, b, c = f2r(), f2r(), f2r()
    n = M.f2_neg
    neigh = [from_w([a] * 6), from_w([a, a, b, b, c, c]), from_w([(a[0], a[0]), (b[0], b[0]), (c[0], c[0]), a, b, c]),
             from_w([a, n(a), b, n(b), c, n(c)]), from_w([(a[0], P - a[0]), (b[0], P - b[0]), a, n(a), c, c])]
    rnd = [from_w([f2r() for _ in range(6)]) for _ in range(12)]
    return interleave(fixed, basis, sub, limb, neigh, rnd)


@functools.lru_cache(None)
def gt_cyclotomic():
    """u^((p^6 - 1)(p^2 + 1)) of the non-zero elements: conj(u) / u, then its p^2-power times itself"""
    out = []
    for u in gt_elements():
        if u != F12_ZERO:
            t = M.f12_mul(M.f12_conj(u), M.f12_inv(u))
            out.append(M.f12_mul(M.f12_frob(t, 2), t))
    return out


@functools.lru_cache(None)
def gt_members():
    return [M.final_exponentiation(c) for c in [c for c in gt_cyclotomic() if c != M.F12_ONE][3::5][:6]]


def _pow_by_mul(a, b, reps):
    w = M.f12_mul(a, b)
    for _ in range(reps - 1):
        w = M.f12_mul(w, b)
    return w


GT_REPS = (1, 2, 5)


@functools.lru_cache(None)
def gt_table(op):
    """(rows, labels, {reps: expected words}) of one op — built once, shared by both halves"""
    els = gt_elements()
    lab = lambda n: [("row %d" % i,) for i in range(n)]
    if op in ("gt_roundtrip", "gt_conj", "gt_neg", "gt_sqr_by_mul", "gt_frob1", "gt_frob2", "gt_inv"):
        rows = gt_odd(els)
        fn = {"gt_roundtrip": lambda a: a, "gt_conj": M.f12_conj, "gt_neg": lambda a: tuple(tuple(M.f2_neg(c) for c in six) for six in a),
              "gt_sqr_by_mul": lambda a: M.f12_mul(a, a), "gt_frob1": lambda a: M.f12_frob(a, 1), "gt_frob2": lambda a: M.f12_frob(a, 2),
              "gt_inv": lambda a: a if a == F12_ZERO else M.f12_inv(a)}[op]
        return enc12(rows), rows, {1: enc12([fn(a) for a in rows])}
    if op == "gt_mul":
        n = len(els)
        pairs = gt_odd(interleave([(els[i], els[(7 * i + 3) % n]) for i in range(n)], [(a, a) for a in els[::3]], [(a, M.f12_conj(a)) for a in els[1::4]]))
        rows = np.hstack([enc12([a for a, _ in pairs]), enc12([b for _, b in pairs])])
        return rows, lab(len(pairs)), {r: enc12([_pow_by_mul(a, b, r) for a, b in pairs]) for r in GT_REPS}
    if op in ("gt_cyc_sqr", "gt_exp_by_x"):
        rows = gt_odd(interleave(gt_cyclotomic(), gt_members()))
        if op == "gt_exp_by_x":
            return enc12(rows), lab(len(rows)), {1: enc12([M.f12_conj(M.f12_pow(c, M.X_ABS)) for c in rows])}
        want, cur = {}, rows
        for r in range(1, max(GT_REPS) + 1):
            cur = [M.f12_mul(c, c) for c in cur]
            if r in GT_REPS:
                want[r] = enc12(cur)
        return enc12(rows), lab(len(rows)), want
    if op == "gt_final_exp":
        cyc = gt_cyclotomic()
        rows = gt_odd(GT_FIXED + els[3:8] + els[17:23] + [cyc[-1], cyc[-2], gt_members()[0]])
        assert len(rows) < 20
        fe = [M.final_exponentiation(a) for a in rows]
        want = np.hstack([enc12([F12_ZERO if w is None else w for w in fe]), np.array([[int(w is None)] for w in fe], np.uint64)])
        return enc12(rows), lab(len(rows)), {1: want}
    if op == "gt_tail_step":
        n = len(els)
        pairs = gt_odd([(els[i], els[(5 * i + 2) % n]) for i in range(31)])
        ks = (0, 1, 2, 15, 16, 199)                     # k p + (the coefficient's Montgomery image): raw values up to 200 p, as the sparse products leave them
        raw = lambda f, s: [w for j, c in enumerate(_f12_flat(f)) for w in raw_words(carried(ks[(s + j) % len(ks)] * P + c * 2 ** 406 % P))]
        rows = np.array([raw(f, i) + raw(l, i + 3) for i, (f, l) in enumerate(pairs)], np.uint64)
        want, cur = {}, [f for f, _ in pairs]
        for r in range(1, max(GT_REPS) + 1):
            cur = [M.f12_mul(M.f12_mul(f, f), l) for f, (_, l) in zip(cur, pairs)]
            if r in GT_REPS:
                want[r] = enc12(cur)
        return rows, lab(len(pairs)), want
    raise KeyError(op)


@functools.lru_cache(None)
def gt_membership_table():
    """rows and verdicts (bit 0: in the cyclotomic subgroup, bit 1: in GT): zero 0, one 3, cyclotomic images 1 — or 3 where the model says f^r = 1 —, GT members 3,
    each GT member with one word of one coefficient changed 0, elements outside the cyclotomic subgroup 0.  Minus one is 0 as well: the subgroup's order
    p^4 - p^2 + 1 is odd, so it holds no element of order two — the model's power below says so, whatever one might expect of a norm-one element."""
    els, cyc, gts = gt_elements(), gt_cyclotomic(), gt_members()
    m1 = GT_FIXED[2]
    assert M.f12_pow(m1, P ** 4 - P ** 2 + 1) == m1 != M.F12_ONE and M.f12_mul(m1, m1) == M.F12_ONE

    def in_cyclotomic(f):                               # f^(p^4) f = f^(p^2), through the model's Frobenius
        f2 = M.f12_frob(f, 2)
        return f != F12_ZERO and M.f12_mul(M.f12_frob(f2, 2), f) == f2
    assert all(M.f12_pow(g, R) == M.F12_ONE for g in gts)
    fixed = list(zip(enc12(GT_FIXED), (0, 3, 0)))
    images = [(w, 3 if M.f12_pow(c, R) == M.F12_ONE else 1) for w, c in zip(enc12(cyc), cyc)]
    members = [(w, 3) for w in enc12(gts)]
    broken = []
    for i, w in enumerate(enc12(gts)):
        w = w.copy()
        w[6 * (2 * i + 1) + i] ^= np.uint64(1)          # word i of coefficient 2 i + 1
        assert U.fp_int(w[6 * (2 * i + 1):6 * (2 * i + 2)]) < P
        broken.append((w, 0))
    outside = [a for a in els if a not in GT_FIXED and not in_cyclotomic(a)]
    assert len(outside) >= 12
    rows = gt_odd(interleave(fixed, images, members, broken, [(w, 0) for w in enc12(outside)]))
    return np.stack([w for w, _ in rows]), np.array([v for _, v in rows], np.uint64)


@functools.lru_cache(None)
def gt_shrink_table():
    """gt_shrink's inputs, twelve Fp per row (lane e: the row's Fp 2 e and 2 e + 1).  k p + d as carried limbs, k in 0, 1, 2, 15, 16, 199, 200, 5038 and d in 0, 1,
    p - 1 and the limb patterns; and limbs written directly: every low limb 0, 2^29 - 1 or 2^29 + 7 under a top limb of 0, 1, 12, 13, 14, 25, 26, 27, 208, 2600,
    2^16 - 1.  The host half (the function's own assertions: low limbs <= 2^29 + 7, top limb < 2^16) accepts every one of them, so all are kept — those with a top
    limb of 2600 and more, the range k_miller_tail's comment speaks of, among them."""
    ds = [0, 1, P - 1] + _patterns(P, (29, 30), 381)
    kd = [carried(k * P + d) for k in (0, 1, 2, 15, 16, 199, 200, 5038) for d in ds]
    direct = [[low] * 13 + [top] for low in (0, 2 ** 29 - 1, 2 ** 29 + 7) for top in (0, 1, 12, 13, 14, 25, 26, 27, 208, 2600, 2 ** 16 - 1)]
    fps = interleave(kd, direct)
    assert any(l[13] >= 2600 for l in fps)
    while len(fps) % 12 or (len(fps) // 12) % 3 == 0 or (len(fps) // 12) % 10 == 0:
        fps.append(fps[(5 * len(fps)) % len(kd)])
    return np.array([w for l in fps for w in raw_words(l)], np.uint64).reshape(len(fps) // 12, 84), fps


def check_gt_shrink(got, fps):
    """per Fp: result = input mod p, limbs 0..12 < 2^29, value < 2 p; the canonical words are those of the value"""
    o = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 52)           # per lane: c0's 14 limbs, c1's, then 12 + 12 canonical words
    i22 = pow(2 ** 22, -1, P)                                                 # limbs hold x 2^406, the ABI words x 2^384
    for i, l in enumerate(fps):
        lane, half = o[i // 2], i % 2
        r = [int(x) for x in lane[14 * half:14 * half + 14]]
        v, vin = limbs_value(r), limbs_value(l)
        assert v % P == vin % P, ("gt_shrink: value", i, l, r)
        assert all(x < 2 ** 29 for x in r[:13]) and v < 2 * P, ("gt_shrink: limbs carried, value < 2 p", i, l, r)
        canon = sum(int(x) << (32 * j) for j, x in enumerate(lane[28 + 12 * half:40 + 12 * half]))
        assert canon == vin * i22 % P, ("gt_shrink: canonical words", i, l)


@functools.lru_cache(None)
def gt_digits_table():
    from test_gpu_gt_pow import EDGE                    # (the exponents the GT-power tests use)
    rng = random.Random(20268)
    exps = odd_rows(_uniq(EDGE + [int("8" * 64, 16), int("9" * 64, 16), int("7" * 63 + "9", 16), 2 ** 256 - 1] + [rng.randrange(2 ** 256) for _ in range(40)]))
    want = []
    for x in exps:                                      # v = nibble + carry; v > 8 gives v - 16 and a carry; digit 64 is the carry out of bit 255
        d, c = [], 0
        for w in range(64):
            v = ((x >> (4 * w)) & 15) + c
            c = 1 if v > 8 else 0
            d.append(v - 16 * c)
        d.append(c)
        assert sum(v * 16 ** w for w, v in enumerate(d)) == x and all(-7 <= v <= 8 for v in d)
        want.append(d)
    return exps, want


def check_gt(run, family, groups):
    """one family of ops through either backend, every table at every G of `groups` (and at every reps for the ops that feed their output back)"""
    def plain(op):
        rows, lab, want = gt_table(op)
        for G in groups:
            for reps, w in want.items():
                mismatch(run(op, reps | G << 8, rows), w, lab, "%s G=%d reps=%d" % (op, G, reps))
    if family == "lane_local":
        rows, els, want = gt_table("gt_roundtrip")
        srows, fps = gt_shrink_table()
        for G in groups:
            got = run("gt_roundtrip", 1 | G << 8, rows)
            mismatch(got[:, :72], want[1], [("row %d" % i,) for i in range(len(els))], "gt_roundtrip G=%d" % G)
            raw = np.ascontiguousarray(got[:, 72:]).view(np.uint32).reshape(len(els), 6, 2, 14)          # the scratch element in the internal form
            for i, f in enumerate(els):
                for e, c in enumerate(w_coeffs(f)):
                    for h in (0, 1):
                        l = [int(x) for x in raw[i, e, h]]
                        assert limbs_value(l) % P == c[h] * 2 ** 406 % P and limbs_value(l) < 2 * P and all(x <= 2 ** 29 + 7 for x in l[:13]), ("gt_put / gt_get", G, i, e, h)
            check_gt_shrink(run("gt_shrink", 1 | G << 8, srows), fps)
        for op in ("gt_conj", "gt_neg", "gt_frob1", "gt_frob2"):
            plain(op)
    elif family == "products":
        for op in ("gt_mul", "gt_sqr_by_mul", "gt_tail_step"):
            plain(op)
    elif family == "cyclotomic":
        for op in ("gt_cyc_sqr", "gt_exp_by_x"):
            plain(op)
    elif family == "inverse":
        plain("gt_inv")
    elif family == "final_exp":
        plain("gt_final_exp")
    elif family == "membership":
        rows, want = gt_membership_table()
        for G in groups:
            got = run("gt_membership", 1 | G << 8, rows)[:, 0]
            bad = np.nonzero(got != want)[0]
            assert not len(bad), ("gt_membership G=%d: rows %s give %s, want %s" % (G, bad[:8], got[bad[:8]], want[bad[:8]]))
    elif family == "digits":
        exps, want = gt_digits_table()
        got = run("gt_digits", 1, words(exps, 32))
        d = np.ascontiguousarray(got).view(np.int8).reshape(len(exps), 72)
        for i, x in enumerate(exps):
            assert [int(v) for v in d[i, :65]] == want[i] and not d[i, 65:].any(), ("gt_signed_digits", hex(x))
    else:
        raise KeyError(family)


GT_FAMILIES = ("lane_local", "products", "cyclotomic", "inverse", "final_exp", "membership", "digits")


# ---- the line steps (pairing29.hip.h) against a transcription of the ark-ec M-twist formulas (bls12/g2.rs double_in_place / add_in_place) ----
def line_dbl(Rp):
    X, Y, Z = Rp
    half = lambda t: M.f2_mul_fp(t, (P + 1) // 2)
    a, b, c = half(M.f2_mul(X, Y)), M.f2_sqr(Y), M.f2_sqr(Z)
    e = M.f2_mul_fp(M.f2_mul(c, (1, 1)), 12)
    f = M.f2_mul_fp(e, 3)
    g, h = half(M.f2_add(b, f)), M.f2_sub(M.f2_sqr(M.f2_add(Y, Z)), M.f2_add(b, c))
    i, j = M.f2_sub(e, b), M.f2_sqr(X)
    Rn = (M.f2_mul(a, M.f2_sub(b, f)), M.f2_sub(M.f2_sqr(g), M.f2_mul_fp(M.f2_sqr(e), 3)), M.f2_mul(b, h))
    return Rn, (i, M.f2_mul_fp(j, 3), M.f2_neg(h))


def line_add(Rp, Q):
    X, Y, Z = Rp
    theta, lam = M.f2_sub(Y, M.f2_mul(Q[1], Z)), M.f2_sub(X, M.f2_mul(Q[0], Z))
    c, d = M.f2_sqr(theta), M.f2_sqr(lam)
    e, f, g = M.f2_mul(lam, d), M.f2_mul(Z, c), M.f2_mul(X, d)
    h = M.f2_sub(M.f2_add(e, f), M.f2_add(g, g))
    Rn = (M.f2_mul(lam, h), M.f2_sub(M.f2_mul(theta, M.f2_sub(g, h)), M.f2_mul(e, Y)), M.f2_mul(Z, e))
    return Rn, (M.f2_sub(M.f2_mul(theta, Q[0]), M.f2_mul(lam, Q[1])), M.f2_neg(theta), lam)


LINE_STEPS = (1, 3)


@functools.lru_cache(None)
def line_tables():
    """(doubling rows R, addition rows (R, Q)): R = Q with Z = 1 (the first step) over generator multiples 1 .. 6, their negatives and the off-subgroup points;
    coordinates with a zero half, c0 = +-c1, limb patterns, Y = 0, random R; for the addition also R projectively equal to Q and to -Q (theta = lambda = 0, and
    lambda = 0 alone).  The formulas are polynomial, so the degenerate rows have exact expected words too."""
    rng = random.Random(20267)
    f2r = lambda: (rng.randrange(P), rng.randrange(P))
    off = U.off_subgroup_points()
    pts = [M.g2_mul(M.G2_GEN, k) for k in range(1, 7)]
    pts = pts + [M.g2_neg(q) for q in pts] + [off["T2"][0], off["S2"][0]]
    pat = _patterns(P, (29, 30), 381)
    a, b, c = (rng.randrange(P) for _ in range(3))
    first = [(q[0], q[1], (1, 0)) for q in pts]
    edge = [((a, 0), (0, b), (c, 0)), ((0, a), (b, 0), (0, c)), ((a, a), (b, P - b), (c, c)), ((a, P - a), (b, b), (c, P - c)),
            ((pat[0], pat[1]), (pat[2], pat[3]), (pat[4], pat[5])), ((pat[5], pat[6]), (pat[7], pat[8]), (pat[9], pat[0])),
            (f2r(), F2Z, f2r()), (pts[0][0], F2Z, (1, 0)), (F2Z, f2r(), f2r()), (f2r(), f2r(), F2Z)]
    rnd = [(f2r(), f2r(), f2r()) for _ in range(10)]
    dbl = odd_rows(interleave(first, edge, rnd))
    scale = lambda q, z, s=1: (M.f2_mul(q[0], z), M.f2_mul(M.f2_mul_fp(q[1], s % P), z), z)
    add = [(line_dbl(r)[0], (r[0], r[1])) for r in first]                                    # the loop's own first addition: R = 2 Q
    add += [(scale(q, f2r()), q) for q in pts[:4]] + [(scale(q, f2r(), -1), q) for q in pts[:4]] + [((q[0], q[1], (1, 0)), q) for q in pts[4:6]]
    add += [(r, (r[2], r[0])) for r in edge] + [(r, pts[i]) for i, r in enumerate(edge)] + [(r, pts[(3 * i) % len(pts)]) for i, r in enumerate(rnd)]
    add += [((f2r(), f2r(), f2r()), (f2r(), f2r())) for _ in range(6)]
    return dbl, odd_rows(add)


@functools.lru_cache(None)
def line_expected():
    dbl, add = line_tables()
    flat = lambda Rn, l: Rn + l
    want = {}
    for s in LINE_STEPS:
        out = []
        for r in dbl:
            for _ in range(s):
                r, l = line_dbl(r)
            out.append(flat(r, l))
        want["dbl", s] = cols(out, enc_f2)
        out = []
        for r, q in add:
            for _ in range(s):
                r, l = line_add(r, q)
            out.append(flat(r, l))
        want["add", s] = cols(out, enc_f2)
    return cols(dbl, enc_f2), cols([r + q for r, q in add], enc_f2), want


def check_lines(run, names=("line_dbl", "line_add")):
    dbl, add = line_tables()
    drows, arows, want = line_expected()
    for s in LINE_STEPS:
        mismatch(run(names[0], s, drows), want["dbl", s], dbl, "%s x %d" % (names[0], s))
        mismatch(run(names[1], s, arows), want["add", s], add, "%s x %d" % (names[1], s))


def test_op_table_matches_the_kernel_header():
    """the numbers and row shapes above are those of selftest_kernels.hip.h and selftest_gt_kernels.hip.h (a mismatch would otherwise only show as a refused call)"""
    import re
    src = open(os.path.join(CSRC, "selftest_kernels.hip.h")).read() + open(os.path.join(CSRC, "selftest_gt_kernels.hip.h")).read()
    body = re.search(r"enum : int \{(.*?)ST_OP_END", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    num, nxt = {}, 0
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        if "=" in item:
            item, v = [s.strip() for s in item.split("=")]
            nxt = int(v)
        num[item[3:].lower()] = nxt
        nxt += 1
    assert num == {k: v[0] for k, v in OPS.items()}
    val = lambda e: eval(re.sub(r"SW<(\w+)>::N", lambda m: {"Fp": "12", "Fs": "12", "Fp2": "24", "Fs2": "24"}[m.group(1)], e.replace("ST_CHAIN_IN(Fp)", str(_CH1)).replace("ST_CHAIN_IN(Fs)", str(_CH1))
                                 .replace("ST_CHAIN_IN(Fp2)", str(_CH2)).replace("ST_CHAIN_IN(Fs2)", str(_CH2)).replace("ST_PT_OUT(Fp)", "24").replace("ST_PT_OUT(Fs)", "24")
                                 .replace("ST_PT_OUT(Fp2)", "48").replace("ST_PT_OUT(Fs2)", "48").replace("ST_GT_RAW", "84").replace("ST_GT_SHRUNK", "26").replace("GT_LANES", "6")))
    assert re.search(r"constexpr int ST_GT_RAW = GT_LANES \* NL;", src) and re.search(r"constexpr int ST_GT_SHRUNK = 26;", src)
    seen = {}
    for dev, name, lanes, iw, ow in re.findall(r"^ST_(DEV_)?OP\(ST_(\w+), (\d), (.+?), ([^,]+?)\) \{", src, re.M):
        seen[name.lower()] = (val(iw), val(ow), 0 if dev else 1)
    six = {}
    for name, iw, ow in re.findall(r"^ST_GT_OP\(ST_(\w+), (.+?), ([^,]+?)\) \{", src, re.M):        # the third macro: six lanes per row, host and device
        six[name.lower()] = (val(iw), val(ow), 1)
    assert set(six) == GT_SIX and not set(six) & set(seen)
    seen.update(six)
    assert seen == {k: v[1:] for k, v in OPS.items() if v[1] is not None}


# ---- the CPU half: the same rows through the wrappers' host build, under the bound tracker ----
def test_host_fp_and_fs(shim):
    check_fp(host_backend(shim))


def test_host_fp_and_fs_lazy_operands(shim):
    check_fp_lazy(host_backend(shim))


def test_host_fp2(shim):
    check_f2(host_backend(shim), F2_HOST)


def test_host_fr(shim):
    check_fr(host_backend(shim))


def test_host_fp12(shim):
    check_f12(host_backend(shim))


@pytest.mark.parametrize("g", [1, 2])
def test_host_group_law(shim, g):
    check_group(host_backend(shim), g, G1_HOST if g == 1 else G2_HOST)


@pytest.mark.parametrize("family", GT_FAMILIES)
def test_host_gt_ops(gt_shim, family):
    """the six-lane wrappers with six threads as the lanes, under the bound tracker (G means nothing on the host)"""
    check_gt(gt_host_backend(gt_shim), family, (1,))


def test_host_gt_refuses_other_ops_and_shapes(gt_shim):
    z = np.zeros(256, np.uint64)
    p = z.ctypes.data_as(C.c_void_p)
    assert gt_shim.shim_selftest_gt(OPS["gt_conj"][0], 1 | 3 << 8, p, 72, 1, p, 72) == 0
    assert gt_shim.shim_selftest_gt(OPS["gt_conj"][0], 1 | 1 << 8, p, 71, 1, p, 72) == -3
    assert gt_shim.shim_selftest_gt(OPS["fp_mul"][0], 1 | 1 << 8, p, 12, 1, p, 6) == -3
    assert gt_shim.shim_selftest_gt(OPS["gt_mul"][0], 65 | 1 << 8, p, 144, 1, p, 72) == -3


def test_host_line_steps(shim):
    """line_dbl_step / line_add_step (the wrappers the device runs), then the same rows through the forms the lane-distributed kernels run —
    line_dbl_step_fast, line_dbl_step_ws, line_add_step_ws —, which have no one-lane kernel on the device"""
    check_lines(host_backend(shim))
    form = lambda k: (lambda name, stress, rows: _run(lambda op, *a: shim.shim_line_steps(k, *a), name, stress, rows))
    fast, ws_dbl, ws_add = form(0), form(1), form(2)
    check_lines(lambda name, s, rows: (fast if name == "line_dbl" else ws_add)(name, s, rows))
    check_lines(lambda name, s, rows: (ws_dbl if name == "line_dbl" else ws_add)(name, s, rows))


def test_host_line_transcription_is_the_miller_loops_step(shim):
    """the transcription above is the function the loop uses: its 68 lines are those of shim_miller_lines, and folded they give the model's Miller loop"""
    shim.shim_miller_lines.argtypes = [C.c_void_p] * 3
    for Pa, Q in ((M.g1_mul(M.G1_GEN, 3), M.g2_mul(M.G2_GEN, 5)), (M.g1_mul(M.G1_GEN, 7), U.off_subgroup_points()["T2"][0])):
        Rp, lines = (Q[0], Q[1], (1, 0)), []
        for bit in X_BITS:
            Rp, l = line_dbl(Rp); lines.append(l)
            if bit == "1":
                Rp, l = line_add(Rp, Q); lines.append(l)
        assert len(lines) == 68
        ev = [(l[0], M.f2_mul_fp(l[1], Pa[0]), M.f2_mul_fp(l[2], Pa[1])) for l in lines]
        pw, qw, out = np.ascontiguousarray(enc_fp(list(Pa)).reshape(-1)), np.ascontiguousarray(enc_f2(list(Q)).reshape(-1)), np.zeros((68, 36), np.uint64)
        shim.shim_miller_lines(pw.ctypes.data_as(C.c_void_p), qw.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        mismatch(out, cols(ev, enc_f2), [("line %d" % i,) for i in range(68)], "the Miller loop's lines")
        f, it = M.F12_ONE, iter(ev)
        for bit in X_BITS:
            f = M.f12_mul_by_014(M.f12_mul(f, f), *next(it))
            if bit == "1":
                f = M.f12_mul_by_014(f, *next(it))
        assert M.f12_conj(f) == M.multi_miller_loop([Pa], [Q])


def test_host_refuses_what_it_cannot_run(shim):
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data_as(C.c_void_p)
    assert shim.shim_selftest_arith(OPS["fp2h_mul"][0], 1, p, 24, 1, p, 12) == -3          # a lane exchange: device only
    assert shim.shim_selftest_arith(OPS["fp_mul"][0], 1, p, 11, 1, p, 6) == -3             # not the op's row shape
    assert shim.shim_selftest_arith(999, 1, p, 6, 1, p, 6) == -3


# ---- the GPU half ----
@pytest.mark.gpu
def test_gpu_fp_and_fs(twin):
    check_fp(gpu_backend(twin))


@pytest.mark.gpu
def test_gpu_fp_and_fs_lazy_operands(twin):
    check_fp_lazy(gpu_backend(twin))


@pytest.mark.gpu
def test_gpu_fp2_one_lane_and_lane_pairs(twin):
    """the lane-pair forms (DPP exchanges of fp2_pair.hip.h / fs2_pair.hip.h: one row per lane pair, so the two pairs of a quad hold different rows) and
    the inversions of fp_inv.hip.h exist on the device only; their operands are those the host half runs through the one-lane forms"""
    check_f2(gpu_backend(twin), F2_HOST + F2_DEVICE)


@pytest.mark.gpu
def test_gpu_fr(twin):
    check_fr(gpu_backend(twin))


@pytest.mark.gpu
def test_gpu_fp12(twin):
    check_f12(gpu_backend(twin))


@pytest.mark.gpu
def test_gpu_group_law_g1(twin):
    """G1 over both fields, one lane per point.  (G2 with one lane per point has a host build only — see selftest_kernels.hip.h; on the device G2 runs
    through the lane-pair and four-lane forms of test_gpu_group_law_shared_lanes.)"""
    check_group(gpu_backend(twin), 1, G1_HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("g", [1, 2])
def test_gpu_group_law_shared_lanes(twin, g):
    """ec29_two_lane.hip.h (two lanes per G1 point, four per G2 point), xyzz_phi and xyzz_to_affine: the chains of the one-lane test, P + P, P + (-P) and
    the identity partway among them, so the special branch is taken by some rows of a wave and not by their neighbours"""
    check_group(gpu_backend(twin), g, G1_DEVICE if g == 1 else G2_DEVICE)


# Time limits of the GT tests: a call is one launch of at most 67 groups; the longest chain, gt_final_exp, is some 400 lane-group products and squarings
# (milliseconds on the device).  What a test spends is the model's expectations (seconds, built once per table and shared with the host half) and the
# first call's start-up, so 120 s is a limit only a hung kernel reaches.
@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("family", GT_FAMILIES)
def test_gpu_gt_ops(twin, family):
    """the six-lane wrappers behind GT_GROUP_PROLOGUE, every table at 1, 3 and 10 groups per wave: GtLanesDev's slots, ballots and early lane exits"""
    check_gt(gpu_backend(twin), family, GT_GROUPS)


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_gpu_line_steps(twin):
    check_lines(gpu_backend(twin))


@pytest.mark.gpu
def test_gpu_gt_refuses_other_group_counts(twin):
    z = np.zeros(256, np.uint64)
    p = z.ctypes.data_as(C.c_void_p)
    op = OPS["gt_conj"][0]
    for G in range(0, 12):
        assert twin.dgpu_selftest_arith(op, 1 | G << 8, p, 72, 0, p, 72) == (0 if G in GT_GROUPS else -3), G
    assert twin.dgpu_selftest_arith(op, 65 | 1 << 8, p, 72, 0, p, 72) == -3
    assert twin.dgpu_selftest_arith(op, 1 | 3 << 8, p, 71, 0, p, 72) == -3
    assert twin.dgpu_selftest_arith(OPS["fp_mul"][0], 1 | 1 << 8, p, 12, 0, p, 6) == -3          # the plain ops take no G


@pytest.mark.gpu
def test_gpu_refuses_unknown_ops_and_shapes(twin):
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data_as(C.c_void_p)
    assert twin.dgpu_selftest_arith(999, 1, p, 6, 1, p, 6) == -3
    assert twin.dgpu_selftest_arith(OPS["fp_mul"][0], 1, p, 11, 1, p, 6) == -3
    assert twin.dgpu_selftest_arith(OPS["fr_batch_inv"][0], 17, p, 68, 1, p, 68) == -3
    assert twin.dgpu_selftest_arith(OPS["fp_mul"][0], 1, p, 12, 0, p, 6) == 0
