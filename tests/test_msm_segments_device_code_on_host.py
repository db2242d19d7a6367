"""CPU: the device code of the segmented small MSM that does not depend on the device (crypto_amd/csrc/seg_layout.hip.h: the geometry of one segment and
the layout of a ragged batch over blocks of 64 groups with its descriptor array; many_fold.hip.h: the Horner fold over a window count, the inversion and the
normalisation to the ABI's representative) compiled for the host with the FP29_CHECK worst-case bound tracker (tests/native/seg_dev_host_shim.cpp) and checked
against the big-integer model.  The shim walks the descriptors the way k_seg_tree does — same accessors, same leaf and pairing functions — so the layout
properties hold for the kernel: every term lies in exactly one leaf of its own segment, no tree level pairs groups of two segments, widths are powers of two
at aligned offsets, a multi-block segment owns whole blocks.  An assertion inside the shim fires whenever a lazy-limb overflow is possible for SOME input of
the same value classes, so a green run proves the 252-doubling chain of the 64-window fold overflow-free, not just right on these inputs."""
import ctypes as C
import os
import random
import subprocess
import numpy as np
import pytest
import bls12_381_model as M
import util as U

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "seg_dev_host_shim.cpp")
SO = os.path.join(HERE, "native", "libseg_dev_host_shim.so")
P = M.P
NONE = 0xffffffff
WALK_ERR = {1: "a term read twice", 2: "a term never read", 3: "a tree level crosses a segment boundary", 4: "width / alignment", 5: "multi-block ownership",
            6: "first group of a segment", 7: "descriptor fields"}


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(HERE, "..", "crypto_amd", "csrc", f) for f in ("seg_layout.hip.h", "many_fold.hip.h", "fp29.hip.h", "fp30s.hip.h", "fs2_pair.hip.h", "ec29.hip.h", "fp_safegcd.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.shim_seg_geometry.argtypes = [C.c_size_t, C.c_void_p]
    L.shim_seg_walk.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    L.shim_seg_layout.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    L.shim_seg_layout.restype = C.c_size_t
    return L


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def geometry(shim, n):
    g = np.zeros(3, np.int32)
    shim.shim_seg_geometry(n, p_(g))
    return tuple(int(x) for x in g)


def check_batch(shim, lens, rng, s0=0, s1=None):
    """segments [s0, s1) of a batch with these lengths through the shim's walk (the kernel's use of the descriptors, on integers) and the
    descriptor array itself"""
    lens = [int(x) for x in lens]
    s1 = len(lens) if s1 is None else s1
    seg_end = np.cumsum(np.array(lens, np.uint64), dtype=np.uint64)
    N = int(seg_end[-1]) if len(lens) else 0
    val = np.array([rng.getrandbits(64) for _ in range(max(N, 1))], np.uint64)
    sums = np.full(len(lens), 0xdeadbeef, np.uint64)
    rc = shim.shim_seg_walk(p_(seg_end), s0, s1, p_(val), p_(sums))
    assert rc == 0, (WALK_ERR.get(rc, rc), lens[:12], s0, s1)
    lo = np.concatenate([[0], seg_end[:-1]]).astype(np.int64)
    for g in range(s0, s1):
        want = int(val[int(lo[g]):int(seg_end[g])].sum(dtype=np.uint64)) if lens[g] else 0
        assert int(sums[g]) == want, (g, lens[g])
    # the descriptors themselves: 64 per block, aligned power-of-two runs, whole blocks for multi-block segments, input order, nothing reserved
    cap = sum((n + 511) // 512 + 1 for n in lens[s0:s1]) + 1
    desc = np.zeros((cap * 64, 4), np.uint32)
    pslots = C.c_size_t(0)
    blocks = shim.shim_seg_layout(p_(seg_end), s0, s1, p_(desc), cap, C.byref(pslots))
    assert blocks <= cap
    desc = desc[:blocks * 64].reshape(blocks, 64, 4)
    order = []
    used = 0
    for b in range(blocks):
        gi = 0
        while gi < 64:
            seg, first, pack, pslot = (int(x) for x in desc[b, gi])
            n, pg, width, j, nblk, levels = pack & 0x3fff, pack >> 14 & 15, 1 << (pack >> 18 & 7), pack >> 21 & 15, (pack >> 25 & 15) + 1, 1 << (pack >> 29)
            assert levels == max([2] + [1 << (int(q) >> 18 & 7) for s_, q in zip(desc[b, :, 0], desc[b, :, 2]) if int(s_) != NONE])      # the block's widest segment
            assert width in (2, 4, 8, 16, 32, 64) and gi % width == 0
            if seg == NONE:
                gi += 2
                continue
            assert n == lens[s0 + seg] and first == int(lo[s0 + seg]) - int(lo[s0]) and (pg, width, nblk) == geometry(shim, n)
            assert (desc[b, gi:gi + width] == desc[b, gi]).all()
            if nblk > 1:
                assert width == 64 and gi == 0 and n > 512
            if j == 0:
                order.append(seg)
            used += width
            gi += width
    assert order == list(range(s1 - s0))                                      # every segment once, in input order
    assert int(pslots.value) == sum((n + 511) // 512 for n in lens[s0:s1] if n > 512)
    # no block is reserved for a short segment.  A block is closed only when the next segment (w groups) does not fit behind the groups in use (u) and the
    # alignment gaps (each smaller than the segment behind it, so less than u in all; the next one's less than w): 2 u + 2 w > 64, i.e. any two
    # neighbouring blocks hold more than 32 groups in use between them
    need = sum(geometry(shim, n)[1] * geometry(shim, n)[2] for n in lens[s0:s1])
    assert used == need and (blocks // 2) * 32 < need + 1
    return blocks


def test_geometry_of_every_length(shim):
    """per_group = clamp(ceil(n / 64), 2, 8); the width is the smallest power of two (>= 2) holding ceil(n / per_group) groups — rounded UP — and from 513
    terms on the segment owns ceil(n / 512) whole blocks"""
    for n in list(range(0, 601)) + [1023, 1024, 1025, 4095, 4096, 4097, 8190, 8191, 8192]:
        pg, width, nblk = geometry(shim, n)
        assert pg == min(8, max(2, -(-n // 64)))
        groups = -(-n // pg)
        if n <= 512:
            assert nblk == 1 and width >= max(groups, 2) and (width == 2 or width // 2 < groups) and width * pg >= n
        else:
            assert (pg, width) == (8, 64) and nblk == -(-n // 512) and nblk <= 16
    for n, want in ((0, 2), (1, 2), (2, 2), (4, 2), (5, 4), (8, 4), (9, 8), (31, 16), (32, 16), (33, 32), (64, 32), (65, 64), (128, 64), (129, 64), (512, 64)):
        assert geometry(shim, n)[1] == want, n


def test_layout_of_every_single_length(shim):
    rng = random.Random(11)
    for n in range(0, 601):
        assert check_batch(shim, [n], rng) == -(-max(n, 1) // 512)
    for n in (8190, 8191, 8192):                                              # the border of the small path's reach (8193 is the slow path's: never laid out)
        assert check_batch(shim, [n], rng) == 16
    for n in (513, 1024, 1025, 4096, 4097):
        check_batch(shim, [n, 3, n, 0, 5], rng)


def test_layout_of_equal_segments_packs_blocks(shim):
    """equal short segments fill their blocks completely: 64 / width per block"""
    rng = random.Random(12)
    for n, per_block in ((1, 32), (2, 32), (3, 32), (5, 16), (16, 8), (31, 4), (32, 4), (33, 2), (64, 2), (65, 1), (256, 1)):
        for nseg in (1, 2, 63, 64, 65, 300):
            assert check_batch(shim, [n] * nseg, rng) == -(-nseg // per_block), (n, nseg)


def test_layout_of_random_ragged_batches(shim):
    """240 seeded batches: lengths from every regime (empty, a few terms, around the width and block borders, up to 8192), empty segments first, last and
    in a row, and sub-ranges [s0, s1) as a chunked call lays them out"""
    rng = random.Random(13)
    pools = [(0, 1, 2, 3, 5), (0, 1, 5, 64, 65, 511, 512, 513, 4096), tuple(range(0, 70)), (0, 7, 8, 9, 31, 32, 33, 127, 128, 129, 8191, 8192)]
    for k in range(240):
        pool = pools[k % 4]
        nseg = rng.randrange(1, 90)
        lens = [rng.choice(pool) if rng.random() < 0.8 else rng.randrange(0, 1500) for _ in range(nseg)]
        if k % 3 == 0:
            lens[0] = 0
        if k % 3 == 1:
            lens[-1] = 0
        if k % 5 == 0 and nseg > 3:
            lens[nseg // 2] = lens[nseg // 2 + 1] = 0
        check_batch(shim, lens, rng)
        if nseg > 4:
            s0 = rng.randrange(1, nseg - 1)
            check_batch(shim, lens, rng, s0, rng.randrange(s0 + 1, nseg + 1))
    check_batch(shim, [0] * 70, rng)                                          # nothing but empty segments


class Grp:
    def __init__(self, g):
        self.g = g
        if g == 1:
            self.add, self.neg, self.mul, self.gen, self.FW = M.g1_add, M.g1_neg, M.g1_mul, M.G1_GEN, 6
        else:
            self.add, self.neg, self.mul, self.gen, self.FW = M.g2_add, M.g2_neg, M.g2_mul, M.G2_GEN, 12

    def f_abi(self, v):
        return U.fp_abi(v) if self.g == 1 else np.concatenate([U.fp_abi(v[0]), U.fp_abi(v[1])])

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

    def rand_f(self, rng):
        return rng.randrange(1, P) if self.g == 1 else (rng.randrange(1, P), rng.randrange(P))

    def expect(self, pt):
        """the ABI's normalised Jacobian words: (x, y, 1), identity (1, 1, 0)"""
        if pt is None:
            return np.concatenate([self.f_abi(self.one()), self.f_abi(self.one()), self.f_abi(self.zero())])
        return np.concatenate([self.f_abi(pt[0]), self.f_abi(pt[1]), self.f_abi(self.one())])


def horner(G, sums):
    acc = None
    for v in range(len(sums) - 1, -1, -1):
        if acc is not None:
            acc = G.mul(acc, 16)
        if sums[v] is not None:
            acc = G.add(acc, sums[v])
    return acc


@pytest.mark.parametrize("g", [1, 2])
def test_fold_over_64_windows(shim, g):
    """the 64-window Horner fold (four doublings between windows, none in front of the top one), the normalisation and the ABI words: identity window sums, an
    identity total, a total that equals a single window sum (top, bottom and middle window), P with P and P with -P inside the chain"""
    G = Grp(g)
    rng = random.Random(50 + g)
    fold = shim.shim_seg_fold_g1 if g == 1 else shim.shim_seg_fold_g2
    W = 64
    pts = [G.mul(G.gen, rng.randrange(1, M.R)) for _ in range(W)]
    cases = []
    cases.append(list(pts))
    cases.append([None] * W)                                                              # an identity total out of identities
    cases.append([pts[i] if i % 3 else None for i in range(W)])
    for only in (0, 31, 63):
        cases.append([pts[5] if i == only else None for i in range(W)])                  # a total that IS one window sum (x 16^only)
    c = list(pts); c[62] = G.mul(c[63], 16); cases.append(c)                              # P with P at window 62: the doubling inside the addition
    c = list(pts); c[62] = G.neg(G.mul(c[63], 16)); cases.append(c)                       # P with -P: the identity after window 62, then on
    c = [None] * W; c[63] = pts[1]; c[62] = G.neg(G.mul(pts[1], 16)); cases.append(c)    # ... and nothing after it: an identity total out of two points
    c = list(pts); c[20] = G.neg(G.mul(horner(G, [None] * 21 + c[21:]), 16)); cases.append(c)   # the identity in the middle of the chain
    c = [None] * W; c[2] = G.neg(pts[2]); c[0] = G.mul(pts[2], 256); cases.append(c)     # window 0 cancels 16^2 x window 2: the identity at the very last addition
    cases.append([pts[7]] * W)
    cases.append([G.gen if i in (0, 63) else None for i in range(W)])
    for k, sums in enumerate(cases):
        win = np.zeros((W, 4 * G.FW), np.uint64); inf = np.zeros(W, np.uint8)
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
