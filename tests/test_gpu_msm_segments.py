"""GPU (-m gpu): dgpu_msm_g*_segments — many small MSMs, each over its own bases, in one call (crypto_amd/csrc/seg_kernels.hip.h: one table launch over
all the bases of a chunk, the tree of the small path over ragged segments laid out by descriptors, short segments packed several to a block, then Horner +
normalisation per segment on the device or on the host's threads).  Bar: bit-exact.  EVERY segment of every case equals the single call dgpu_msm_g* on that
segment with the size threshold off, and the CPU oracle."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd._native import lib, DockGpuError
from test_gpu_msm import normalised

pytestmark = pytest.mark.gpu
CUR = {"G1": (ca.G1, O.G1), "G2": (ca.G2, O.G2)}
R = U.R
BADARG, TOO_SMALL = -3, -6


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)
    lib().dgpu_set_min_gpu_n(0)                              # the single calls the segments are compared with: threshold off
    yield
    lib().dgpu_set_min_gpu_n(0)


def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_BASES = {}


def pool(gname, n):
    """a prefix of 33024 bases per curve, generated once"""
    if gname not in _BASES:
        _BASES[gname] = U.seq_bases(CUR[gname][1], 33024, 7100 + len(gname), threads=16)[0]
    assert n <= len(_BASES[gname])
    return _BASES[gname][:n]


def ends(lens):
    return np.cumsum(np.array(lens, np.uint64), dtype=np.uint64)


def check(gname, bases, sc, lens, inf=None, montgomery=False, canon=None, what="", oracle=True):
    """the segmented call == the single call on every segment == the oracle on every segment; returns (rows, flags)"""
    curve, G = CUR[gname]
    se = ends(lens)
    got, flags = ca.msm_segments(curve, bases, sc, se, is_inf=inf, montgomery=montgomery, flags=True)
    assert got.shape == (len(lens), curve.JW)
    plain = sc if canon is None else canon
    lo = 0
    h = G.AW // 2
    one_x = np.zeros(h, np.uint64); one_x[:6] = U.fp_abi(1)
    ident = np.concatenate([one_x, one_x, np.zeros(h, np.uint64)])     # (1, 1, 0)
    for g, n in enumerate(lens):
        b, s = np.ascontiguousarray(bases[lo:lo + n]), np.ascontiguousarray(sc[lo:lo + n])
        fl = None if inf is None else np.ascontiguousarray(inf[lo:lo + n])
        if n:
            one = (ca.msm_unchecked if montgomery else ca.msm_bigint)(curve, b, s, fl)
            assert (got[g] == one).all(), (what, gname, g, n)
        assert flags[g] == (0 if got[g][G.AW:].any() else 1), (what, gname, g, n)
        if n == 0:
            assert (got[g] == ident).all() and flags[g] == 1, (what, gname, g)
        if oracle:
            f2 = np.zeros(n, np.uint8) if fl is None else fl.copy()
            if n:
                f2 |= (~b.any(axis=1)).astype(np.uint8)
            want = normalised(G, G.msm(b, np.ascontiguousarray(plain[lo:lo + n]), f2, threads=16)) if n else ident
            assert (got[g] == want).all(), (what, gname, g, n)
        lo += n
    return got, flags


@pytest.mark.parametrize("gname", ["G1", "G2"])
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33])
def test_equal_segments(gname, n):
    for nseg in (1, 2, 63, 64, 65, 1000):
        N = n * nseg
        check(gname, pool(gname, N), O.rand_scalars(9100 + 131 * n + nseg, N), [n] * nseg, what="equal")


RAGGED = [0, 1, 5, 64, 65, 511, 512, 513, 4096, 5, 0, 0, 1, 513, 64, 3, 0]


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_ragged_batch(gname):
    N = sum(RAGGED)
    check(gname, pool(gname, N), O.rand_scalars(9300, N), RAGGED, what="ragged")


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_reach_of_the_small_path(gname):
    """8192 terms is the last length the segment kernels serve; 8193 goes through the single-call driver inside the call, next to short ones"""
    for lens in ([3, 8192, 7, 1], [2, 8193, 0, 9, 8193, 4]):
        N = sum(lens)
        check(gname, pool(gname, N), O.rand_scalars(9400 + len(lens), N), lens, what="reach")


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_empty_segments(gname):
    for k, lens in enumerate(([0, 4, 9], [4, 9, 0], [4, 0, 0, 9], [0, 0, 7, 0, 0], [0], [0, 0, 0])):
        N = sum(lens)
        _, flags = check(gname, pool(gname, max(N, 1))[:N], O.rand_scalars(9500 + k, max(N, 1))[:N], lens, what="empty")
        assert [int(f) for f in flags] == [1 if n == 0 else 0 for n in lens]


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_chunk_boundaries_and_both_folds(twin, gname):
    """the development knob puts a chunk boundary between two short segments (5 7 3 | 9) and just before a multi-block segment (9 | 600 | 4 2), and forces
    either fold: the same words as the unchunked call with the automatic fold, whichever way"""
    lens = [5, 7, 3, 9, 600, 4, 2, 0, 15, 16]
    N = sum(lens)
    bases, sc = pool(gname, N), O.rand_scalars(9600, N)
    whole, wflags = check(gname, bases, sc, lens, what="unchunked")
    try:
        for fold in (1, 2):
            for chunk in (0, 15, 1, 31):
                assert twin.dgpu_set_msm_segments(fold, chunk) == 0
                got, flags = check(gname, bases, sc, lens, what="fold %d chunk %d" % (fold, chunk), oracle=(chunk == 15))
                assert (got == whole).all() and (flags == wflags).all(), (fold, chunk)
        # many segments, both folds (the automatic choice takes the device from a few dozen segments on)
        many = [3, 17, 0, 64] * 40
        N = sum(many)
        bases, sc = pool(gname, N), O.rand_scalars(9601, N)
        res = []
        for fold in (1, 2, 0):
            assert twin.dgpu_set_msm_segments(fold, 0) == 0
            res.append(check(gname, bases, sc, many, what="fold %d" % fold, oracle=(fold == 1)))
        assert (res[0][0] == res[1][0]).all() and (res[0][0] == res[2][0]).all() and (res[0][1] == res[1][1]).all()
    finally:
        twin.dgpu_set_msm_segments(0, 0)


def _negated(G, bases):
    """P_i = -P_{i-1} for odd i"""
    neg = bases.copy(); h = G.AW // 2
    for i in range(1, len(bases), 2):
        neg[i] = bases[i - 1]
        for k in range(h // 6):
            y = U.fp_int(neg[i][h + 6 * k:h + 6 * k + 6]); neg[i][h + 6 * k:h + 6 * k + 6] = U.fp_abi((U.P - y) % U.P)
    return neg


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_point_and_scalar_edge_cases(gname):
    curve, G = CUR[gname]
    lens = [6, 24, 1, 150, 2, 33, 64, 8]
    N = sum(lens)
    bases = pool(gname, N).copy()
    lim = lambda v: O.int_to_limbs(v, 4)
    sc = O.rand_scalars(9700, N)
    # identity bases by flag and by zero words
    inf = np.zeros(N, np.uint8); inf[::4] = 1
    zb = bases.copy(); zb[2::9] = 0
    check(gname, zb, sc, lens, inf=inf, what="identity bases")
    allinf = np.ones(N, np.uint8)
    _, flags = check(gname, bases, sc, lens, inf=allinf, what="all identity")
    assert flags.all()
    # zero scalars: a whole segment, and scattered
    z = sc.copy(); z[6:30] = 0; z[200::3] = 0
    _, flags = check(gname, bases, z, lens, what="zero scalars")
    assert flags[1] == 1
    # r - 1, r and 2^255 - 1 (the largest scalar the ABI accepts), the extreme nibbles
    e = sc.copy()
    e[0:6] = lim(R - 1); e[6:14] = lim(R); e[14:22] = lim((1 << 255) - 1)
    nib = lambda d: int(("%x" % d) * 63, 16) % (1 << 255)
    for k, d in enumerate((7, 8, 0xF, 9, 1)):
        e[31 + k:181:5] = lim(nib(d))
    e[181] = lim(R - 1); e[182] = lim(R)
    check(gname, bases, e, lens, what="r - 1, r, 2^255 - 1")
    # coinciding bases, and P with -P under equal scalars: the identity appears inside the tree
    same = bases.copy(); same[6:30] = bases[7]; same[31:181] = bases[40]
    check(gname, same, sc, lens, what="coinciding bases")
    neg = _negated(G, bases)
    pair = sc.copy(); pair[1::2] = pair[0:N - (N % 2):2]
    _, flags = check(gname, neg, pair, lens, what="P and -P")
    assert flags[0] == 1 and flags[1] == 1 and flags[6] == 1 and flags[7] == 1       # segments of whole pairs that start at an even term cancel
    # &[Fr] limbs
    mont = O.fr_to_mont(z)
    check(gname, bases, mont, lens, montgomery=True, canon=z, what="montgomery")


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_montgomery_scalars_across_chunks(twin, gname):
    """random full-width &[Fr] limbs over short and multi-block segments, unchunked and with the chunks cut so that the second and third start at a
    scalar offset (5 600 | 9 | 700 3): the conversion runs on each chunk's own slice"""
    lens = [5, 600, 9, 700, 3]
    N = sum(lens)
    bases, sc = pool(gname, N), O.rand_scalars(9750, N)
    mont = O.fr_to_mont(sc)
    whole, _ = check(gname, bases, mont, lens, montgomery=True, canon=sc, what="montgomery, one chunk")
    try:
        for fold in (1, 2):
            assert twin.dgpu_set_msm_segments(fold, 605) == 0
            got, _ = check(gname, bases, mont, lens, montgomery=True, canon=sc, what="montgomery, chunks, fold %d" % fold, oracle=False)
            assert (got == whole).all(), fold
    finally:
        twin.dgpu_set_msm_segments(0, 0)


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_bases_outside_the_prime_order_subgroup(gname):
    from test_gpu_off_subgroup import mixed
    lens = [1, 7, 0, 44, 65, 3, 520, 31]
    N = sum(lens)
    bases, inf = mixed(gname, N, 9800)
    check(gname, bases, O.rand_scalars(9801, N), lens, inf=inf, what="off subgroup")
    small = np.zeros((N, 4), np.uint64); small[:, 0] = np.arange(N) % 40              # multiples that meet the small orders
    check(gname, bases, small, lens, inf=inf, what="off subgroup, small scalars")


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_refusals(gname):
    curve, G = CUR[gname]
    lens = [4, 9, 0, 30, 2]
    N = sum(lens)
    bases, sc, se = pool(gname, N), O.rand_scalars(9900, N), ends(lens)
    fn = curve.fn("dgpu_msm_%s_segments")
    out = np.zeros((len(lens), curve.JW), np.uint64)
    good, _ = check(gname, bases, sc, lens, what="good")
    for at in (0, N - 1, 20):                                                       # the first scalar, the last, one of a middle segment
        bad = sc.copy(); bad[at, 3] |= np.uint64(1 << 63)
        assert fn(p_(bases), None, p_(bad), N, p_(se), len(lens), 0, p_(out), None) == BADARG, at
        assert fn(p_(bases), None, p_(sc), N, p_(se), len(lens), 0, p_(out), None) == 0      # the refused call left nothing behind
        assert (out == good).all()
    desc = np.array([4, 13, 12, 43, 45], np.uint64)
    assert fn(p_(bases), None, p_(sc), N, p_(desc), len(lens), 0, p_(out), None) == BADARG
    assert fn(p_(bases), None, p_(sc), N - 1, p_(se), len(lens), 0, p_(out), None) == BADARG
    assert fn(None, None, p_(sc), N, p_(se), len(lens), 0, p_(out), None) == BADARG
    assert fn(p_(bases), None, p_(sc), N, None, len(lens), 0, p_(out), None) == BADARG
    assert fn(None, None, None, 77, None, 0, 0, None, None) == 0                   # nseg = 0
    # the size threshold looks at the batch, not the segment
    one = [1] * 256
    b1, s1 = pool(gname, 256), O.rand_scalars(9901, 256)
    o1 = np.zeros((256, curve.JW), np.uint64)
    try:
        lib().dgpu_set_min_gpu_n(256)
        below = fn(p_(b1), None, p_(s1), 255, p_(ends(one[:255])), 255, 0, p_(o1), None)
        at = fn(p_(b1), None, p_(s1), 256, p_(ends(one)), 256, 0, p_(o1), None)
    finally:
        lib().dgpu_set_min_gpu_n(0)
    assert below == TOO_SMALL and at == 0
    want, _ = check(gname, b1, s1, one, what="256 one-term segments")
    assert (o1 == want).all()


def test_two_host_threads_and_no_allocation_on_a_repeated_shape():
    jobs = []
    for k, (gname, lens) in enumerate((("G1", [3, 70, 0, 600, 12] * 6), ("G2", [1, 2, 33, 513, 0, 8] * 5), ("G1", [16] * 256), ("G2", [64] * 34))):
        N = sum(lens)
        jobs.append((gname, pool(gname, N), O.rand_scalars(9950 + k, N), lens))
    want = [check(*j, what="serial")[0] for j in jobs]
    # (the serial calls above were each shape's first: a call that grows its slot sizes the idle slots with it, so whichever slot a thread is handed below has seen the shape)
    a0 = ca.device_alloc_count()
    for j, w in zip(jobs, want):
        assert (ca.msm_segments(CUR[j[0]][0], j[1], j[2], ends(j[3])) == w).all()
    assert ca.device_alloc_count() == a0

    def worker(t):
        return [(k, ca.msm_segments(CUR[jobs[k][0]][0], jobs[k][1], jobs[k][2], ends(jobs[k][3]))) for rep in range(3) for k in range(t, len(jobs), 2)]

    with ThreadPoolExecutor(2) as ex:
        for f in [ex.submit(worker, t) for t in range(2)]:
            for k, got in f.result():
                assert (got == want[k]).all(), k
    assert ca.device_alloc_count() == a0


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_saver_ciphertext_commitments(gname):
    """saver/src/encryption.rs:710-740: chunks + 2 = 34 MSMs, each over its own column of 64 ciphertexts, all with the same r_powers (replicated)"""
    nseg, n = 34, 64
    r_powers = O.rand_scalars(9990, n)
    sc = np.tile(r_powers, (nseg, 1))
    check(gname, pool(gname, nseg * n), sc, [n] * nseg, what="saver")


def test_wrapper_refuses_like_the_abi():
    sc = O.rand_scalars(9991, 10); sc[3, 3] |= np.uint64(1 << 63)
    with pytest.raises(DockGpuError):
        ca.msm_segments(ca.G1, pool("G1", 10), sc, [4, 10])
    assert ca.msm_segments(ca.G1, pool("G1", 10), sc, []).shape == (0, 18)
