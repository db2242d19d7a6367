"""CPU: the device code of the many-row small MSM (crypto_amd/csrc/many_fold.hip.h: the launch geometry with its row packing, the Horner step over the 16
super-window sums, the inversion and the normalisation to the ABI's representative) compiled for the host with the FP29_CHECK worst-case bound tracker
(tests/native/many_dev_host_shim.cpp) and checked against the big-integer model.  An assertion inside the shim fires whenever a lazy-limb overflow is
possible for SOME input of the same value classes, so a green run proves the new doubling chain (four xyzz_dbl_rounds between additions, sixteen times over) and
the normalisation overflow-free, not just right on these inputs."""
import ctypes as C
import os
import random
import subprocess
import numpy as np
import pytest
import bls12_381_model as M
import util as U

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "many_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libmany_dev_host_shim.so")
P = M.P
ONE = U.fp_abi(1)
NS = (1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(HERE, "..", "crypto_amd", "csrc", f) for f in ("many_fold.hip.h", "fp29.hip.h", "fp30s.hip.h", "fs2_pair.hip.h", "ec29.hip.h", "fp_safegcd.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.shim_many_tree_g1.restype = L.shim_many_tree_g2.restype = C.c_long
    for f in (L.shim_many_tree_g1, L.shim_many_tree_g2):
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    L.shim_many_geometry.argtypes = [C.c_size_t, C.c_void_p]
    return L


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


class Grp:
    def __init__(self, g):
        self.g = g
        if g == 1:
            self.add, self.neg, self.mul, self.gen, self.FW = M.g1_add, M.g1_neg, M.g1_mul, M.G1_GEN, 6
        else:
            self.add, self.neg, self.mul, self.gen, self.FW = M.g2_add, M.g2_neg, M.g2_mul, M.G2_GEN, 12

    def f_abi(self, v):
        return U.fp_abi(v) if self.g == 1 else np.concatenate([U.fp_abi(v[0]), U.fp_abi(v[1])])

    def f_int(self, w):
        return U.fp_int(w[:6]) if self.g == 1 else (U.fp_int(w[:6]), U.fp_int(w[6:12]))

    def fmul(self, a, b):
        return a * b % P if self.g == 1 else M.f2_mul(a, b)

    def one(self):
        return 1 if self.g == 1 else (1, 0)

    def zero(self):
        return 0 if self.g == 1 else (0, 0)

    def xyzz(self, pt, z):
        """the XYZZ words of pt with ZZ = z^2, ZZZ = z^3"""
        zz = self.fmul(z, z); zzz = self.fmul(zz, z)
        return np.concatenate([self.f_abi(self.fmul(pt[0], zz)), self.f_abi(self.fmul(pt[1], zzz)), self.f_abi(zz), self.f_abi(zzz)])

    def aff(self, pt):
        return np.concatenate([self.f_abi(pt[0]), self.f_abi(pt[1])])

    def rand_f(self, rng):
        return rng.randrange(1, P) if self.g == 1 else (rng.randrange(1, P), rng.randrange(P))

    def expect(self, pt):
        """the ABI's normalised Jacobian words: (x, y, 1), identity (1, 1, 0)"""
        if pt is None:
            return np.concatenate([self.f_abi(self.one()), self.f_abi(self.one()), self.f_abi(self.zero())])
        return np.concatenate([self.f_abi(pt[0]), self.f_abi(pt[1]), self.f_abi(self.one())])


def horner(G, sums):
    acc = None
    for v in range(15, -1, -1):
        if acc is not None:
            acc = G.mul(acc, 16)
        if sums[v] is not None:
            acc = G.add(acc, sums[v])
    return acc


@pytest.mark.parametrize("g", [1, 2])
def test_fold_horner_and_normalisation(shim, g):
    """window sums with identities, P with P (the addend equals 16 x the accumulator: the doubling inside the addition), P with -P (the accumulator
    becomes the identity in the middle of the chain and is doubled on), an all-identity row, a single window"""
    G = Grp(g)
    rng = random.Random(40 + g)
    fold = shim.shim_many_fold_g1 if g == 1 else shim.shim_many_fold_g2
    pts = [G.mul(G.gen, rng.randrange(1, M.R)) for _ in range(16)]
    cases = []
    cases.append(list(pts))
    cases.append([None] * 16)
    cases.append([pts[i] if i % 3 else None for i in range(16)])
    cases.append([pts[3] if i == 0 else None for i in range(16)])
    cases.append([pts[3] if i == 15 else None for i in range(16)])
    c = list(pts); c[14] = G.mul(c[15], 16); cases.append(c)                              # P with P at window 14
    c = list(pts); c[14] = G.neg(G.mul(c[15], 16)); cases.append(c)                       # P with -P: identity after window 14, then on
    c = [None] * 16; c[15] = pts[1]; c[14] = G.neg(G.mul(pts[1], 16)); cases.append(c)   # ... and nothing after it: an identity row
    c = list(pts); c[15] = None; c[14] = None; c[12] = G.mul(pts[13], 16); c[5] = G.neg(G.mul(horner(G, [None] * 6 + c[6:]), 16)); cases.append(c)
    cases.append([pts[7]] * 16)
    cases.append([G.gen if i in (0, 15) else None for i in range(16)])
    for k, sums in enumerate(cases):
        win = np.zeros((16, 4 * G.FW), np.uint64); inf = np.zeros(16, np.uint8)
        for v, s in enumerate(sums):
            if s is None:
                inf[v] = 1
                win[v] = rng.getrandbits(60)                                               # (an identity's coordinates are never read)
            else:
                win[v] = G.xyzz(s, G.rand_f(rng) if (k + v) % 2 else G.one())
        out = np.zeros(3 * G.FW, np.uint64)
        flag = fold(p_(win), p_(inf), p_(out))
        want = horner(G, sums)
        assert flag == (1 if want is None else 0), k
        assert (out == G.expect(want)).all(), k


def test_fp2_inversion(shim):
    rng = random.Random(9)
    vals = [(1, 0), (0, 1), (P - 1, P - 1), (2, P - 1), (1, 1)] + [(rng.randrange(P), rng.randrange(P)) for _ in range(60)]
    o = np.zeros(12, np.uint64)
    for a in vals:
        shim.shim_many_inv_g2(p_(np.concatenate([U.fp_abi(a[0]), U.fp_abi(a[1])])), p_(o))
        assert (U.fp_int(o[:6]), U.fp_int(o[6:])) == M.f2_inv(a), a


def test_geometry_covers_every_row_length(shim):
    """per_group in 2 .. 8; a segment is a power of two holding the row's groups; segments tile the block; at most 64 blocks per row"""
    g = np.zeros(4, np.int32)
    for n in list(range(1, 700)) + [1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192]:
        shim.shim_many_geometry(n, p_(g))
        pg, seg, rpb, nblk = (int(x) for x in g)
        L = 4 * n
        assert 2 <= pg <= 8 and 1 <= nblk <= 64 and seg & (seg - 1) == 0 and 2 <= seg <= 64 and rpb * seg == 64
        if nblk == 1:
            assert seg * pg >= L and (seg == 2 or (seg // 2) * pg < L)                      # the smallest power of two that holds the row
        else:
            assert seg == 64 and nblk * 64 * pg >= L and (nblk - 1) * 64 * pg < L
    for n, want in ((1, 32), (2, 16), (3, 8), (4, 8), (7, 4), (8, 4), (15, 2), (16, 2), (17, 1), (32, 1), (33, 1)):
        shim.shim_many_geometry(n, p_(g))
        assert g[2] == want, (n, g)                                                        # rows per block at the packing boundaries


@pytest.mark.parametrize("g,ns", [(1, NS), (2, (1, 3, 8, 17, 33, 129))])
def test_segmented_tree_row_packing(shim, g, ns):
    """the block of k_many_tree on the host: several rows per block, every leaf read exactly once, no fold crosses a row boundary (a row's sum is its own
    leaves' sum whatever its neighbours hold), identity leaves, P beside P and P beside -P inside a segment, rows that are padding"""
    G = Grp(g)
    rng = random.Random(70 + g)
    small = [None] + [G.mul(G.gen, k) for k in range(1, 12)]
    small += [G.neg(p) for p in small[1:]]
    tree = shim.shim_many_tree_g1 if g == 1 else shim.shim_many_tree_g2
    geo = np.zeros(4, np.int32)
    for n in ns:
        shim.shim_many_geometry(n, p_(geo))
        rpb = int(geo[2])
        L = 4 * n
        for rows in sorted({1, rpb, rpb + 1, 2 * rpb + 3} if n <= 33 else {2}):
            idx = [[rng.randrange(len(small)) for _ in range(L)] for _ in range(rows)]
            if L >= 4:
                idx[0][0] = idx[0][1] = 3; idx[0][2] = 3 + 11                                # P, P, -P next to each other
            if rows > 1:
                idx[1] = [0] * L                                                            # an all-identity row beside ordinary ones
            leaves = np.zeros((rows, L, 2 * G.FW), np.uint64)
            for r in range(rows):
                for l in range(L):
                    if small[idx[r][l]] is not None:
                        leaves[r, l] = G.aff(small[idx[r][l]])
            out = np.zeros((rows, 4 * G.FW), np.uint64); inf = np.full(rows, 9, np.uint8)
            reads = tree(p_(leaves), n, rows, p_(out), p_(inf))
            assert reads == rows * L, (n, rows, reads)                                      # every leaf exactly once (-1: one was skipped or read twice)
            for r in range(rows):
                want = None
                for l in range(L):
                    want = G.add(want, small[idx[r][l]])
                if want is None:
                    assert inf[r] == 1, (n, rows, r)
                    continue
                assert inf[r] == 0, (n, rows, r)
                X, Y, ZZ, ZZZ = (G.f_int(out[r][G.FW * k:G.FW * (k + 1)]) for k in range(4))
                if g == 1:
                    got = (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)
                else:
                    got = (M.f2_mul(X, M.f2_inv(ZZ)), M.f2_mul(Y, M.f2_inv(ZZZ)))
                assert got == want, (n, rows, r)
