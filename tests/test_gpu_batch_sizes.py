"""GPU (-m gpu): the batched scalings, the scaled Miller loop, the LegoGroth16 batch verifier and the two randomised checkers at the sizes where
their kernels change form — against the CPU oracle limb for limb, and (for the verifiers) accept / reject on batches with known discrete logs.

Where the forms change:
  dgpu_g1_scale_batch, dgpu_g1_mul_add_batch   k_g1_scale_oct (sixteen points per block) up to n = 4096, k_g1_scale_quad (sixteen per block) above
                                               (crypto_amd/csrc/k_fixed.hip launch_g1_scale_quad); the addend is added in both
  dgpu_g2_mul_add_batch                        k_mul_add_g2_gls: sixteen lanes per point, four points per block
  dgpu_multi_miller_loop_scaled                up to 8192 affine pairs the pipelined form (oct or quad scalings beside the chain of the Q_i), two calls
                                               (dgpu_g1_scale_batch, then the Miller loop) above or with bit 0 of dgpu_set_miller_pipeline clear
  dgpu_legogroth16_verify_batch                all of the above, plus two MSMs of n and n + n_pub + 1 terms (tree path up to 8192 terms, buckets above)
Edge scalars and identities sit at the first and last index and on both sides of every block and size border (BORDERS).

A batch verifier that gives two proofs the same weight accepts errors that cancel under equal weights (C_i + E with C_j - E, d_i swapped with d_j,
A_i + E with A_j - E where B_i = B_j): those batches are rejected at random batching scalars, and — the check that the construction cancels — accepted
at the scalar 1, where every weight is one."""
import ctypes as C
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd import legogroth16 as LG
from crypto_amd import pairing
from crypto_amd import fixed_base as FB
from crypto_amd._native import lib
from util import mul_add_oracle, first_bad      # (shared with tests/test_gpu_fold_shapes.py and tests/test_gpu_fixed_base.py)

pytestmark = pytest.mark.gpu
R = U.R
LAM = 0xAC45A4010001A40200000000FFFFFFFF                  # GLV: x^2 - 1
X = 0xD201000000010000                                    # GLS: |x|
GLV_EDGE = [0, 1, 2, LAM - 1, LAM, LAM + 1, 2 * LAM, LAM * LAM % R, R - 1, R, R + 5, (1 << 128) - 1, 1 << 128, (1 << 255) - 19, (1 << 256) - 1, 0x1234567]
GLS_EDGE = [X - 1, X, X + 1, X * X - 1, X * X, X * X + 1, X ** 3 - 1, X ** 3, X ** 3 + X, X * X - 2, X * X - 1 + X, 2 ** 64 - 1, 2 ** 64, 2 ** 128 - 1,
            2 ** 128, 2 ** 191, R - X, R - X * X, (X ** 3) * (R // X ** 3), R, R + 5, 2 ** 256 - 1, 0, 1, R - 1]
BORDERS = (16, 4096, 4112, 8192)                          # an oct / quad block; the oct / quad switch; the block behind it; the pipelined / two-call switch
G1_SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 4112, 4113, 20000]
G2_SIZES = [1, 3, 4, 5, 4097, 9000]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def lim(vals):
    """ints below 2^256 -> (n, 4) canonical limbs, NOT reduced mod r"""
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def ints(rng, k):
    return [int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1 for _ in range(k)]


def g1(k):
    return O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(k % R, 4)))[0]


def seq(G, n, seed):
    return O.G1.gen_seq(O.rand_scalars(seed, 1)[0], O.rand_scalars(seed + 1, 1)[0], n, threads=16) if G is O.G1 else \
        O.G2.gen_seq(O.rand_scalars(seed, 1)[0], O.rand_scalars(seed + 1, 1)[0], n, threads=16)


def runs(n, width):
    """start indices of runs of `width` entries that cover the first and the last index and both sides of every border below n"""
    return sorted({0, max(0, n - width)} | {b - width // 2 for b in BORDERS if b < n})


def plant(sc, values):
    n = len(sc)
    for a in runs(n, len(values)):
        for k, v in enumerate(values):
            if a + k < n:
                sc[a + k] = lim([v])[0]


def near(n, ends, border_offsets):
    """indices at the ends (offsets >= 0 from the first index, < 0 from one past the last) and at the given offsets from every border, inside [0, n)"""
    cand = {o if o >= 0 else n + o for o in ends} | {b + o for b in BORDERS for o in border_offsets}
    return sorted(i for i in cand if 0 <= i < n)


# ============================================ 1. dgpu_g1_scale_batch vs the oracle ============================================
def scale_abi(P, is_inf, sc, stride, neg):
    n = len(P)
    out = np.zeros((n, 12), np.uint64); oinf = np.zeros(n, np.uint8)
    assert lib().dgpu_g1_scale_batch(_p(P), _p(is_inf), _p(sc), stride, _p(neg), n, _p(out), _p(oinf)) == 0
    return out, oinf


@pytest.mark.parametrize("n", G1_SIZES)
def test_g1_scale_batch_vs_oracle(n):
    """per-point scalars, one scalar for all (scalar_stride = 0), mixed negate flags, identities as a flag and as zero words, the GLV edge scalars at
    the ends and on both sides of each border: every word and every flag what the oracle's double-and-add returns"""
    rng = np.random.default_rng(4100 + n)
    P = seq(O.G1, n, 300 + n)
    sc = O.rand_scalars(400 + n, n)
    sc[rng.integers(0, 4, n) == 0, 2:] = 0                              # short scalars: k2 = 0 in the split
    plant(sc, GLV_EDGE)
    inf = np.zeros(n, np.uint8)
    ids = near(n, (2, 3, -3, -2), (-2, 1))
    inf[ids[0::2]] = 1                                                  # identity by the flag (the words stay a curve point)
    P[ids[1::2]] = 0                                                    # identity by all-zero words
    oinf = (inf | ~P.any(axis=1)).astype(np.uint8)
    neg = rng.integers(0, 2, n).astype(np.uint8)
    neg[-1] = 1
    for what, s, stride, ng in (("per point, negate mixed", sc, 4, neg), ("per point", sc, 4, None),
                                ("one scalar lambda + 1", lim([LAM + 1]), 0, neg), ("one scalar", sc[n // 2].copy(), 0, neg)):
        got, ginf = scale_abi(P, inf, np.ascontiguousarray(s), stride, ng)
        want, winf = O.g1_scale_batch(P, s.reshape(-1) if stride == 0 else s, negate=ng, is_inf=oinf, threads=16)
        bad = first_bad(got, ginf, want, winf)
        assert len(bad) == 0, (what, bad)
        assert winf[ids].all() and ginf[ids].all(), what


# ============================================ 2. dgpu_g1 / g2_mul_add_batch vs the oracle ============================================
def mul_add_case(G, n, seed, edge):
    """points, scalars and addends with every class of addend at the ends and around the borders: identity by flag / by zero words, the product
    itself (the doubling branch), minus the product (the result is the identity), an ordinary point; identity points by flag / zero words"""
    P = seq(G, n, seed)
    A = seq(G, n, seed + 7)
    sc = O.rand_scalars(seed + 13, n)
    plant(sc, edge)
    p_inf = np.zeros(n, np.uint8); a_inf = np.zeros(n, np.uint8)
    cls = {}
    for k, i in enumerate(near(n, (0, 1, 2, 3, -4, -3, -2, -1), (-2, -1, 0, 1))):
        c = ("flag", "zero", "double", "cancel")[(k + n) % 4]
        if c == "flag":
            a_inf[i] = 1                                                # (the words stay a curve point)
        elif c == "zero":
            A[i] = 0
        else:
            k_i = O.limbs_to_int(sc[i]) % R
            e, einf = G.to_affine(G.mul(P[i], O.int_to_limbs(k_i if c == "double" else (R - k_i) % R, 4)))
            if einf:
                continue                                                # (a scalar 0 mod r: the addend stays an ordinary point)
            A[i] = e
        cls[i] = c
    rest = [i for i in range(min(n, 12)) if i not in cls] + [i for i in range(4100, min(n, 4104)) if i not in cls]
    for k, i in enumerate(rest[:4]):
        if k % 2:
            P[i] = 0
        else:
            p_inf[i] = 1
    return P, p_inf, sc, A, a_inf, cls


def mul_add_abi(G, P, p_inf, sc, A, a_inf):
    n = len(P)
    out = np.zeros((n, G.AW), np.uint64); oinf = np.zeros(n, np.uint8)
    fn = lib().dgpu_g1_mul_add_batch if G is O.G1 else lib().dgpu_g2_mul_add_batch
    assert fn(_p(P), _p(p_inf), _p(sc), 4, _p(A), _p(a_inf), n, _p(out), _p(oinf)) == 0
    return out, oinf


@pytest.mark.parametrize("gname,n", [("G1", n) for n in G1_SIZES] + [("G2", n) for n in G2_SIZES])
def test_mul_add_batch_vs_oracle(gname, n):
    """out_i = A_i + s_i P_i, every word and flag against the oracle's mul + add; G1 with the GLV edge scalars (oct and quad kernels, each with its
    addend), G2 with the GLS digit borders"""
    G = O.G1 if gname == "G1" else O.G2
    P, p_inf, sc, A, a_inf, cls = mul_add_case(G, n, 5000 + n + (0 if G is O.G1 else 50000), GLV_EDGE if G is O.G1 else GLS_EDGE)
    got, ginf = mul_add_abi(G, P, p_inf, sc, A, a_inf)
    want, winf = mul_add_oracle(G, P, p_inf, sc, A, a_inf)
    bad = first_bad(got, ginf, want, winf)
    assert len(bad) == 0, [(int(i), cls.get(int(i), "plain")) for i in bad]
    for i, c in cls.items():                                            # the classes did what they were built for
        if c == "cancel":
            assert ginf[i] and not got[i].any(), i
        if c in ("flag", "zero"):
            assert winf[i] == (O.limbs_to_int(sc[i]) % R == 0 or not P[i].any() or p_inf[i]), i
    # without addends: the plain scaling through the same kernels
    got0, ginf0 = mul_add_abi(G, P, p_inf, sc, None, None)
    want0, winf0 = mul_add_oracle(G, P, p_inf, sc, np.zeros_like(A), np.zeros(n, np.uint8))
    assert len(first_bad(got0, ginf0, want0, winf0)) == 0


# ============================================ 3. the scaled Miller loop vs the oracle ============================================
@pytest.mark.parametrize("n_prep", [0, 2])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8191, 8192, 8193])
def test_scaled_miller_loop_vs_oracle(n, n_prep, twin):
    """prod e([m_i] P_i, Q_i) x prod e(P'_j, prepared_j) limb for limb what the oracle's Miller loop returns on points the oracle scaled, in the
    pipelined form (up to 8192 pairs) and in the two-call form (forced with bit 0 of dgpu_set_miller_pipeline clear); zero scalars, the GLV edge
    scalars, identity points and skip flags, the last pair an ordinary one"""
    rng = np.random.default_rng(6100 + n + n_prep)
    P = seq(O.G1, n + n_prep, 610 + n)
    Q = seq(O.G2, n + n_prep, 620 + n)
    sc = O.rand_scalars(630 + n, n)
    sc[rng.integers(0, 5, n) == 0, 2:] = 0
    plant(sc, GLV_EDGE)
    sc[rng.integers(0, 50, n) == 0] = 0                                  # pairs that drop out
    sc[1] = 0
    ids = [i for i in near(n, (2, 3, -3), (-2, 1)) if i < n - 1]
    P[ids] = 0                                                          # identity points
    skip = (rng.integers(0, 7, n) == 0).astype(np.uint8)
    skip[n - 1] = 0
    sc[n - 1] = O.rand_scalars(640 + n, 1)[0]
    Pa = np.ascontiguousarray(P[:n])
    scaled, sinf = O.g1_scale_batch(Pa, sc, is_inf=(~Pa.any(axis=1)).astype(np.uint8), threads=16)
    osk = np.concatenate([skip | sinf, np.zeros(n_prep, np.uint8)])
    want = O.multi_miller_loop(np.concatenate([scaled, P[n:]]), Q, osk, threads=16)
    prep = pairing.G2Prepared(O.g2_prepare_batch(Q[n:], threads=2), np.zeros(n_prep, np.uint8)) if n_prep else None
    run = lambda: pairing.multi_miller_loop_scaled(Pa, sc, Q[:n], skip, P[n:] if n_prep else None, prep)
    got = run()
    assert (got == want).all(), "default form"
    try:
        assert lib().dgpu_set_miller_pipeline(30) == 0
        two = run()
    finally:
        lib().dgpu_set_miller_pipeline(31)
    assert (two == want).all(), "two-call form"


# ============================================ 4. dgpu_legogroth16_verify_batch accept / reject ============================================
_STMT = {}
N_MAX = 20000


def statement(n_pub):
    """N_MAX valid proofs of one key with n_pub public inputs each, made on the device from known discrete logs (any prefix is a valid batch)"""
    if n_pub in _STMT:
        return _STMT[n_pub]
    rng = np.random.default_rng(7000 + n_pub)
    al, be, ga, de = ints(rng, 4)
    gab = ints(rng, n_pub + 1)
    av, bv, dv = ints(rng, N_MAX), ints(rng, N_MAX), ints(rng, N_MAX)
    xs = [ints(rng, n_pub) for _ in range(N_MAX)]
    dinv = pow(de, R - 2, R)
    sv = [(gab[0] + sum(x * g for x, g in zip(xr, gab[1:]))) % R for xr in xs]
    cv = [((a * b - al * be - (s + d) * ga) * dinv) % R for a, b, d, s in zip(av, bv, dv, sv)]
    with FB.WindowTable(ca.G2, O.G2.generator()) as t2, FB.WindowTable(ca.G1, O.G1.generator()) as t1:
        A, _ = t1.multiply_many(lim(av)); Cc, _ = t1.multiply_many(lim(cv)); D, _ = t1.multiply_many(lim(dv)); K, _ = t1.multiply_many(lim([al] + gab))
        B, _ = t2.multiply_many(lim(bv)); V, _ = t2.multiply_many(lim([be, ga, de]))
    vk = LG.VerifyingKey(K[0], V[0], V[1], V[2], K[1:], O.G1.generator(), 0)
    pubs = lim([x for xr in xs for x in xr]).reshape(N_MAX, n_pub, 4)
    st = dict(pvk=LG.prepare_verifying_key(vk), A=A, B=B, C=Cc, D=D, pubs=pubs, av=av, bv=bv, cv=cv, dv=dv, sv=sv, k=(al * be, ga, dinv))
    _STMT[n_pub] = st
    return st


VERIFY_CASES = [(n, k) for n in (1024, 4096, 4097, 8192, 8193, 20000) for k in (0, 1, 5)] + [(8190, 3)]


@pytest.mark.parametrize("n,n_pub", VERIFY_CASES)
def test_batch_verifier_at_size(n, n_pub):
    """valid batches accepted for several batching scalars and for Montgomery inputs; one corrupted C, one wrong public input, an identity A rejected
    at the ends and around the borders; errors that cancel under equal weights rejected at random scalars and accepted at the scalar 1"""
    st = statement(n_pub)
    pvk = st["pvk"]
    rng = np.random.default_rng(8000 + n + n_pub)
    cols0 = {k: np.ascontiguousarray(st[k][:n]) for k in "ABCD"}
    pubs0 = np.ascontiguousarray(st["pubs"][:n])

    def verify(cols, pubs, rnd, mont=False):
        return LG.verify_proofs_batch_abi(pvk, None, None, rnd, montgomery=mont, packed=(cols["A"], cols["B"], cols["C"], cols["D"], pubs))

    def with_(**rows):
        c = {k: v.copy() for k, v in cols0.items()}
        for key, changes in rows.items():
            for i, v in changes:
                c[key][i] = v
        return c
    rnd = lambda: ints(rng, 1)[0] % (R - 3) + 2                         # (never 0 or 1)
    for r in (1, 2, rnd(), R - 1):
        assert verify(cols0, pubs0, r), r
    assert verify(cols0, O.fr_to_mont(pubs0), rnd(), mont=True)
    pos = sorted({p for p in (0, 15, 16, 4095, 4096, n - 1) if p < n})
    for p in pos:
        assert not verify(with_(C=[(p, g1(st["cv"][p] + 1))]), pubs0, rnd()), ("C", p)
        assert not verify(with_(A=[(p, np.zeros(12, np.uint64))]), pubs0, rnd()), ("identity A", p)
        if n_pub:
            wrong = pubs0.copy()
            j = p % n_pub
            wrong[p, j] = lim([(O.limbs_to_int(wrong[p, j]) + 1) % R])[0]
            assert not verify(cols0, wrong, rnd()), ("public input", p)
    pairs = [(i, j) for i, j in ((0, n - 1), (15, 16), (4095, 4096)) if j < n and i != j]
    e = ints(rng, 1)[0]
    al_be, ga, dinv = st["k"]
    for i, j in pairs:
        cases = {
            "C_i + E, C_j - E": with_(C=[(i, g1(st["cv"][i] + e)), (j, g1(st["cv"][j] - e))]),
            "d_i <-> d_j": with_(D=[(i, cols0["D"][j]), (j, cols0["D"][i])]),
        }
        # proof j re-made with B_j = B_i (a valid batch), then A_i + E, A_j - E
        cj = ((st["av"][j] * st["bv"][i] - al_be - (st["sv"][j] + st["dv"][j]) * ga) * dinv) % R
        shared = with_(B=[(j, cols0["B"][i])], C=[(j, g1(cj))])
        assert verify(shared, pubs0, rnd()), ("shared B", i, j)
        shared["A"][i] = g1(st["av"][i] + e); shared["A"][j] = g1(st["av"][j] - e)
        cases["A_i + E, A_j - E, B_i = B_j"] = shared
        for what, cols in cases.items():
            assert verify(cols, pubs0, 1), ("cancels under equal weights", what, i, j)
            for _ in range(2):
                assert not verify(cols, pubs0, rnd()), (what, i, j)
    if (n, n_pub) == (8193, 1):
        # the Python statement of the same check (its own scalings, MSMs and Miller loop) and the one-proof call agree with the batch call
        r = rnd()
        proofs = lambda cols: [{k.lower(): cols[k][t] for k in "ABCD"} for t in range(n)]
        pl = list(pubs0)
        assert LG.verify_proofs_batch_merged(pvk, proofs(cols0), pl, r)
        bad = with_(C=[(4096, g1(st["cv"][4096] + 1))])
        assert not LG.verify_proofs_batch_merged(pvk, proofs(bad), pl, r) and not verify(bad, pubs0, r)
        assert not LG.verify_proof_abi(pvk, proofs(bad)[4096], pubs0[4096]) and LG.verify_proof_abi(pvk, proofs(cols0)[4096], pubs0[4096])
        sw = with_(D=[(4095, cols0["D"][4096]), (4096, cols0["D"][4095])])
        assert not LG.verify_proofs_batch_merged(pvk, proofs(sw), pl, r) and not verify(sw, pubs0, r)
        assert not LG.verify_proof_abi(pvk, proofs(sw)[4095], pubs0[4095])


# ============================================ 5. the randomised checkers at size ============================================
@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("n", [4097, 8193])
def test_pairing_checker_at_size(n, lazy):
    """RandomizedPairingChecker over two add_multiple_sources equations, n + 1 and 3 + 1 pairs: lazy, all n + 5 pairs go through one scaled Miller
    loop (pipelined for n = 4097, two calls for 8193); eager, the n sources are scaled by k_g1_scale_quad.  True relation accepted; a wrong member,
    and a_i + E in one equation with a'_0 - E in the other (b_i = b'_0: cancels under equal weights) rejected"""
    rng = np.random.default_rng(9000 + n)
    xa, yb = ints(rng, n), ints(rng, n)
    x2 = ints(rng, 3)
    y2 = [yb[n - 1], yb[4096], ints(rng, 1)[0]]
    s1 = sum(x * y for x, y in zip(xa, yb)) % R
    s2 = sum(x * y for x, y in zip(x2, y2)) % R
    with FB.WindowTable(ca.G2, O.G2.generator()) as t2, FB.WindowTable(ca.G1, O.G1.generator()) as t1:
        a, _ = t1.multiply_many(lim(xa)); b, _ = t2.multiply_many(lim(yb))
        a2, _ = t1.multiply_many(lim(x2)); b2, _ = t2.multiply_many(lim(y2))
        c, _ = t1.multiply_many(lim([s1, s2]))
    d = O.G2.generator().reshape(1, 24)
    e = ints(rng, 1)[0]

    def check(r, a=a, a2=a2):
        chk = ca.RandomizedPairingChecker(r, lazy)
        chk.add_multiple_sources(a, b, c[:1], d)                         # prod e(a_i, b_i) == e(s1 G1, G2)
        chk.add_multiple_sources(a2, b2, c[1:], d)
        return chk.verify()
    r = ints(rng, 1)[0]
    assert check(r) and check(1)
    for i in (0, 4095, 4096, n - 1):
        bad = a.copy(); bad[i] = g1(xa[i] + 1)
        assert not check(r, a=bad), i
    for i, k in ((n - 1, 0), (4096, 1)):
        ba, ba2 = a.copy(), a2.copy()
        ba[i] = g1(xa[i] + e); ba2[k] = g1(x2[k] - e)
        assert check(1, ba, ba2), ("cancels under equal weights", i)
        assert not check(r, ba, ba2), i


def test_mult_checker_bucket_path():
    """RandomizedMultChecker.add_many over 8200 + 3 terms: the one MSM of verify() has more than 8192 terms (the bucket pipeline).  True claims
    accepted; a wrong scalar rejected; targets T_1 + E and T_2 - E (cancel under equal weights) rejected at a random scalar, accepted at 1"""
    from crypto_amd.mult_checker import RandomizedMultChecker
    rng = np.random.default_rng(9100)
    n = 8200
    ks, bs = ints(rng, n), ints(rng, n)
    k2, b2 = ints(rng, 3), ints(rng, 3)
    t1v = sum(k * s for k, s in zip(ks, bs)) % R
    t2v = sum(k * s for k, s in zip(k2, b2)) % R
    with FB.WindowTable(ca.G1, O.G1.generator()) as t1:
        pts, _ = t1.multiply_many(lim(ks)); pts2, _ = t1.multiply_many(lim(k2))
    e = ints(rng, 1)[0]

    def check(r, bs=bs, t1=t1v, t2=t2v):
        chk = RandomizedMultChecker(ca.G1, r)
        chk.add_many(pts, bs, g1(t1))
        chk.add_many(pts2, b2, g1(t2))
        assert len(chk) == n + 5
        return chk.verify()
    r = ints(rng, 1)[0]
    assert check(r) and check(1)
    for i in (0, 4096, 8192, n - 1):
        bad = list(bs); bad[i] = (bad[i] + 1) % R
        assert not check(r, bs=bad), i
    assert check(1, t1=t1v + e, t2=t2v - e)
    assert not check(r, t1=t1v + e, t2=t2v - e)
