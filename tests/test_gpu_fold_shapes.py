"""GPU (-m gpu): the fold with prepared doubling chains (dgpu_g*_fold_prepare, dgpu_fold_prepare_pair, dgpu_g*_fold_apply;
crypto_amd/csrc/fold_kernels.hip.h) where its launch shapes change — every row of every call bit for bit what the CPU oracle's mul, add and
to_affine return (an identity row: zero words and the flag set).

Where the shapes change (crypto_amd/csrc/k_fixed.hip launch_fold_apply / launch_fold_chain, k_fold_tree):
  n <= 256      k_fold_tree<.., 64>: a block per point, 64 groups of leaves
  n > 256       k_fold_tree<.., 16>: four points per block, 16 groups each; the last block of a call with n % 4 != 0 is padded with points that
                are not live (they follow every barrier and write nothing)
  T             the number of set bits of the split scalar (G1: k1 and k2 of the GLV split, G2: four base-|x| digits): ceil(T / GPP) leaf rounds,
                then a reduction over min(T, GPP) groups rounded up to a power of two, groups past T holding the identity.  The scalars here are
                BUILT from their split, with T at 0, 1, 2, 3, GPP - 1, GPP, GPP + 1, 2 GPP - 1, 2 GPP, 2 GPP + 1 and the maximum, the set bits all
                in one half / digit or spread unevenly over them (each construction asserts its own split: util.glv_split / util.gls4_split, which
                tests/test_gpu_off_subgroup.py and tests/test_abi_host.py pin to the library's)
  prepare_pair  G1 blocks of 32 points first (blocks1 = ceil(2 n1 / 64)), then G2 blocks of four points: sizes with a partly filled G1 block in
                front of the G2 blocks, on both sides of 32, and with the 16-group form behind both
Planted at the first and last row and at every row of the last block of four: identity points, identity addends, both, an addend equal to minus
the product (the identity comes out) and to the product (the last addition doubles); every apply is repeated without addends (addend_xy = NULL)."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu
R, LAM, X = U.R, U.GLV_LAMBDA, U.GLS_X
T_LIST = {16: (0, 1, 2, 3, 15, 16, 17, 31, 32, 33), 64: (0, 1, 2, 3, 63, 64, 65, 127, 128, 129)}
T_SHORT = (0, 1, 3, 17)                                  # (3: the smallest T whose group count is not a power of two)
SIZES = [("g1", n) for n in (37, 255, 256, 257, 258, 259, 260, 1023, 1025, 4099)] + [("g2", n) for n in (37, 255, 256, 257, 258, 259, 260, 1023, 1025)]
FULL_AT = (37, 257, 258, 259)                             # the sizes that run every T of their form
p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)


def groups(curve):
    return (O.G1, "g1") if curve == "g1" else (O.G2, "g2")


# ---- scalars built from their split ------------------------------------------------------------------------------------------------------------
def with_bits(rng, count, width):
    """an integer below 2^width with exactly `count` set bits"""
    return sum(1 << int(b) for b in rng.choice(width, size=count, replace=False))


def g1_scalar(rng, t1, t2):
    """c = k1 + k2 lambda with t1 set bits in k1 and t2 in k2 (both below 2^127 < lambda, so that c < r and the split is unique)"""
    k1, k2 = with_bits(rng, t1, 127), with_bits(rng, t2, 127)
    c = k1 + k2 * LAM
    assert c < R and U.glv_split(c) == (k1, k2) and bin(k1).count("1") + bin(k2).count("1") == t1 + t2
    return c


def g2_scalar(rng, ts):
    """c = sum d_j |x|^j with ts[j] set bits in d_j (all below 2^63 < |x|, so that c < r and the digits are unique)"""
    d = [with_bits(rng, t, 63) for t in ts]
    c = sum(v * X ** j for j, v in enumerate(d))
    assert c < R and U.gls4_split(c) == d and sum(bin(v).count("1") for v in d) == sum(ts)
    return c


def spreads(g2, T):
    """how T set bits are laid over the halves (G1) / digits (G2): all in the first, all in the last, unevenly over all of them (two ways where T does not
    fit one part)"""
    parts, cap = (4, 63) if g2 else (2, 127)
    out = []
    if T <= cap:
        out += [(T,) + (0,) * (parts - 1), (0,) * (parts - 1) + (T,)]
    for w in ((0.1, 0.4, 0.15, 0.35) if g2 else (0.3, 0.7),) + (((0.4, 0.1, 0.3, 0.2) if g2 else (0.65, 0.35),) if T > cap else ()):
        if T < 2:
            break
        s = [int(T * x) for x in w]
        while sum(s) < T:                                 # the rest one by one to the part that has least (the last of them)
            s[max(j for j in range(parts) if s[j] == min(s))] += 1
        assert sum(s) == T and max(s) <= cap
        out.append(tuple(s))
    return sorted(set(out))


def scalar_list(g2, gpp, full, seed):
    """[(label, c)]: every T of the form under test in every spread (full) or T in {0, 1, 3, 17} (not full), the maximum, seeded random scalars, and
    (full) r, r + 5, 2^256 - 1, which the entry point reduces before it splits them"""
    rng = np.random.default_rng(seed)
    make = (lambda s: g2_scalar(rng, s)) if g2 else (lambda s: g1_scalar(rng, *s))
    out = []
    for T in (T_LIST[gpp] if full else T_SHORT):
        for s in spreads(g2, T):
            out.append(("T=%d %s" % (T, s), make(s)))
    top = (63,) * 4 if g2 else (127, 127)                 # d_j = 2^63 - 1 (T = 252), k1 = k2 = 2^127 - 1 (T = 254)
    out.append(("T=%d max" % sum(top), make(top)))
    assert out[-1][1] == (sum((2 ** 63 - 1) * X ** j for j in range(4)) if g2 else (2 ** 127 - 1) * (1 + LAM))
    for k in range(4 if full else 2):
        out.append(("random %d" % k, int.from_bytes(rng.bytes(40), "little") % R))
    if full:
        out += [("r", R), ("r + 5", R + 5), ("2^256 - 1", 2 ** 256 - 1)]
    return out


def leaf_count(g2, c):
    return sum(bin(v).count("1") for v in (U.gls4_split(c) if g2 else U.glv_split(c)))


def test_scalar_lists_hit_every_leaf_count():
    """(no device work) the lists contain what the module's docstring says: every T of both forms, in one part and spread"""
    for g2 in (False, True):
        for gpp in (16, 64):
            ts = [leaf_count(g2, c) for _, c in scalar_list(g2, gpp, True, 1)]
            assert set(T_LIST[gpp]) | {252 if g2 else 254} <= set(ts)
            assert all(ts.count(T) >= 2 for T in T_LIST[gpp] if T >= 2)
        assert set(T_SHORT) | {252 if g2 else 254} <= {leaf_count(g2, c) for _, c in scalar_list(g2, 16, False, 1)}


# ---- the calls ---------------------------------------------------------------------------------------------------------------------------------
def limbs(v):
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def prepare(g, P):
    h = C.c_uint64(0)
    assert getattr(lib(), "dgpu_%s_fold_prepare" % g)(p(P), len(P), C.byref(h)) == 0
    return h.value


def apply(g, h, c, A, n, words):
    out = np.zeros((n, words), np.uint64); inf = np.zeros(n, np.uint8)
    assert getattr(lib(), "dgpu_%s_fold_apply" % g)(h, p(limbs(c)), p(A), p(out), p(inf)) == 0
    return out, inf


def free(h):
    assert lib().dgpu_fold_free(h) == 0


def check(got, want, what):
    """every row and every identity flag; reports which rows differ (their pattern names the fault: the last block, one lane group, ...)"""
    bad = U.first_bad(got[0], got[1], want[0], want[1])
    assert len(bad) == 0, (what, [int(i) for i in bad])
    assert (~want[0].any(axis=1) == want[1].astype(bool)).all(), what                 # (the expectation itself: identity rows are zero words with the flag set)


def points(G, n, seed):
    return np.ascontiguousarray(U.seq_bases(G, n, seed, threads=16)[0]), np.ascontiguousarray(U.seq_bases(G, n, seed + 500, threads=16)[0])


def identity_jac(G):
    return G.mul(G.generator(), O.int_to_limbs(0, 4), inf=True)


# ---- 1. sizes x leaf counts x planted rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,n", SIZES)
def test_fold_rows_vs_oracle(curve, n):
    """one prepare per size, one apply per scalar with addends and one without; the planted rows take each class of addend in turn as the scalars
    run (ordinary, identity, minus the product, the product); a second handle of the same set with identity points at the planted rows serves a
    few of the scalars.  Sizes on both sides of 256 and of a block of four; FULL_AT run every leaf count of their form, the others T_SHORT."""
    G, g = groups(curve)
    g2 = curve == "g2"
    P, A = points(G, n, 7000 + n + (100000 if g2 else 0))
    planted = sorted({0, n - 1} | set(range(4 * ((n - 1) // 4), n)))                  # first row, last row, every row of the last block of four
    for i in {2, n // 2, n - 6} - set(planted):
        P[i] = 0                                                                      # identity points inside ordinary blocks
    A[n // 3] = 0
    full = n in FULL_AT
    cs = scalar_list(g2, 64 if n <= 256 else 16, full, 9000 + n)
    h = prepare(g, P)
    P_id = P.copy(); P_id[planted] = 0
    h_id = prepare(g, P_id)                                                           # the same set with identity points at the planted rows
    try:
        for s, (label, c) in enumerate(cs):
            cl = O.int_to_limbs(c % R, 4)
            jac = U.scaled_jac(G, P, None, cl)
            Ac = A.copy()
            for j, i in enumerate(planted):                                           # each class at each planted row as s runs
                cls = ("plain", "zero", "cancel", "double")[(j + s) % 4]
                if cls == "zero":
                    Ac[i] = 0
                elif cls == "double":
                    a, inf = G.to_affine(jac[i])
                    Ac[i] = 0 if inf else a                                           # A = c P: the last addition doubles (c P = O: the identity addend)
                elif cls == "cancel":
                    a, inf = G.to_affine(G.mul(P[i], O.int_to_limbs((R - c % R) % R, 4)))
                    Ac[i] = 0 if inf else a                                           # A = -(c P): the identity comes out
            want = U.plus_addends(G, jac, Ac, None)
            for j, i in enumerate(planted):
                if (j + s) % 4 == 2:
                    assert want[1][i] == 1, (label, i)                                # (the construction cancels)
            check(apply(g, h, c, Ac, n, G.AW), want, (curve, n, label, "addends"))
            check(apply(g, h, c, None, n, G.AW), U.plus_addends(G, jac, None, None), (curve, n, label, "no addends"))
            if s % 8 == 1 or label == "T=17 %s" % (spreads(g2, 17)[-1],):            # identity POINTS at the planted rows: with an addend, without, both
                jid = list(jac)
                for i in planted:
                    jid[i] = identity_jac(G)
                Aid = A.copy(); Aid[planted[s % 2::2]] = 0
                check(apply(g, h_id, c, Aid, n, G.AW), U.plus_addends(G, jid, Aid, None), (curve, n, label, "identity points"))
                check(apply(g, h_id, c, None, n, G.AW), U.plus_addends(G, jid, None, None), (curve, n, label, "identity points, no addends"))
    finally:
        free(h); free(h_id)


# ---- 2. both groups' chains in one launch ------------------------------------------------------------------------------------------------------
PAIRS = [(0, 5), (5, 0), (1, 1), (31, 3), (32, 4), (33, 5), (257, 259), (1000, 300)]


@pytest.mark.parametrize("plant", [True, False])
@pytest.mark.parametrize("n1,n2", PAIRS)
def test_prepare_pair_vs_oracle_and_single_prepares(n1, n2, plant):
    """dgpu_fold_prepare_pair's two handles, applied with two scalars each: the oracle's rows, and the rows the handles of dgpu_g1_fold_prepare /
    dgpu_g2_fold_prepare give.  plant: identity points at row 0 and row n - 1 of both sets (a set of one point is then all identity: the unplanted
    pass is what checks its chain).  The pair call comes first, on points no earlier call has seen: a chain that did not run leaves whatever the
    buffer held, never the table of these points."""
    sets = {}
    for g, n in (("g1", n1), ("g2", n2)):
        if n:
            G = groups(g)[0]
            P, A = points(G, n, 30000 + 1000 * n1 + n2 + (500000 if g == "g2" else 0) + (7 if plant else 0))
            if plant:
                P[0] = 0; P[n - 1] = 0
            sets[g] = (G, P, A)
    h1, h2 = C.c_uint64(123), C.c_uint64(456)
    assert lib().dgpu_fold_prepare_pair(p(sets["g1"][1]) if n1 else None, n1, C.byref(h1), p(sets["g2"][1]) if n2 else None, n2, C.byref(h2)) == 0
    handles = {"g1": h1.value, "g2": h2.value}
    assert (h1.value != 0) == (n1 != 0) and (h2.value != 0) == (n2 != 0)              # an empty set leaves its handle 0
    try:
        for g, (G, P, A) in sets.items():
            n = len(P)
            rng = np.random.default_rng(n1 * 1000 + n2)
            cs = [("random", int.from_bytes(rng.bytes(40), "little") % R),
                  ("T=17", g2_scalar(rng, (2, 7, 3, 5)) if g == "g2" else g1_scalar(rng, 5, 12))]
            single = prepare(g, P)
            try:
                for label, c in cs:
                    want = U.mul_add_oracle(G, P, None, O.int_to_limbs(c, 4), A, None)
                    if plant:
                        assert (want[0][0] == A[0]).all() and (want[0][n - 1] == A[n - 1]).all()
                    got = apply(g, handles[g], c, A, n, G.AW)
                    check(got, want, (g, n1, n2, label, "pair"))
                    check(apply(g, single, c, A, n, G.AW), got, (g, n1, n2, label, "single prepare"))
            finally:
                free(single)
    finally:
        for h in handles.values():
            if h:
                free(h)


def test_prepare_pair_of_two_empty_sets_is_refused():
    """include/dock_gpu.h: either set may be empty, not both (DGPU_E_BADARG, both handles 0)"""
    h1, h2 = C.c_uint64(123), C.c_uint64(456)
    assert lib().dgpu_fold_prepare_pair(None, 0, C.byref(h1), None, 0, C.byref(h2)) == -3
    assert h1.value == 0 and h2.value == 0
    pt = np.ascontiguousarray(O.G1.generator()[:12])
    assert lib().dgpu_fold_prepare_pair(p(pt), 0, C.byref(h1), None, 0, None) == -3


# ---- 3. one handle, two host threads -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,n", [("g1", 259), ("g2", 259), ("g1", 64), ("g2", 64)])
def test_two_threads_apply_on_one_handle(curve, n):
    """a handle serves any number of applies, from any thread: two host threads applying different scalars to one handle at the same time get the
    rows a single thread gets, which are the oracle's"""
    G, g = groups(curve)
    P, A = points(G, n, 41000 + n + (curve == "g2"))
    rng = np.random.default_rng(n)
    cs = [g2_scalar(rng, (9, 0, 20, 4)) if curve == "g2" else g1_scalar(rng, 30, 3), int.from_bytes(rng.bytes(40), "little") % R]
    h = prepare(g, P)
    try:
        alone = [apply(g, h, c, A, n, G.AW) for c in cs]
        for c, got in zip(cs, alone):
            check(got, U.mul_add_oracle(G, P, None, O.int_to_limbs(c, 4), A, None), (curve, n, hex(c)))
        start = threading.Barrier(2)
        wrong = []

        def work(k):
            start.wait()
            for it in range(12):
                out, inf = apply(g, h, cs[k], A, n, G.AW)
                if not ((out == alone[k][0]).all() and (inf == alone[k][1]).all()):
                    wrong.append((k, it, [int(i) for i in U.first_bad(out, inf, alone[k][0], alone[k][1])]))
        ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not wrong, wrong
    finally:
        free(h)
