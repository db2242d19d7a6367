"""Shared helpers for the tests: int <-> ABI limb conversion and fixture loading.
The oracle (oracle/) is test infrastructure; nothing in crypto_amd/ imports it."""
import json
import os
import numpy as np
import oracle_c as O
import bls12_381_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P, R = M.P, M.R
_RI = pow(M.FP_R, -1, P)


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def fp_abi(v):
    """canonical int -> 6 u64 Montgomery limbs (ark-ff layout)"""
    return O.int_to_limbs(v * M.FP_R % P, 6)


def fp_int(l):
    return O.limbs_to_int(l) * _RI % P


def g1_abi(pt):
    """model point (x, y) or None -> (12 u64, is_inf)"""
    if pt is None:
        return np.zeros(12, np.uint64), 1
    return np.concatenate([fp_abi(pt[0]), fp_abi(pt[1])]), 0


def g2_abi(pt):
    if pt is None:
        return np.zeros(24, np.uint64), 1
    return np.concatenate([fp_abi(pt[0][0]), fp_abi(pt[0][1]), fp_abi(pt[1][0]), fp_abi(pt[1][1])]), 0


def dec_g1(e):
    return None if e is None else (int(e[0], 16), int(e[1], 16))


def dec_g2(e):
    return None if e is None else ((int(e[0][0], 16), int(e[0][1], 16)), (int(e[1][0], 16), int(e[1][1], 16)))


def jac_to_model(G, jac):
    """Jacobian limbs -> model affine point (ints) or None, via the oracle's to_affine"""
    a, inf = G.to_affine(np.ascontiguousarray(jac, dtype=np.uint64))
    if inf:
        return None
    v = [fp_int(a[6 * i:6 * i + 6]) for i in range(G.AW // 6)]
    return (v[0], v[1]) if G.AW == 12 else ((v[0], v[1]), (v[2], v[3]))


def case_arrays(case):
    """fixture MSM case -> (bases ABI array, is_inf, scalars array, expected model point)"""
    g2 = case["group"] == "G2"
    enc, dec = (g2_abi, dec_g2) if g2 else (g1_abi, dec_g1)
    pts = [enc(dec(b)) for b in case["bases"]]
    w = 24 if g2 else 12
    bases = np.stack([p[0] for p in pts]) if pts else np.zeros((0, w), np.uint64)
    inf = np.array([p[1] for p in pts], dtype=np.uint8)
    sc = np.stack([O.int_to_limbs(int(s, 16), 4) for s in case["scalars"]]) if case["scalars"] else np.zeros((0, 4), np.uint64)
    return bases, inf, sc, dec(case["expected"])


def f12_abi(vals):
    return np.concatenate([fp_abi(int(v, 16) if isinstance(v, str) else v) for v in vals])


def f12_ints(limbs):
    return [fp_int(limbs[6 * i:6 * i + 6]) for i in range(12)]


def seq_bases(G, n, seed, threads=8):
    """P_i = (k0 + i d) G with known dlogs; returns (bases, k0, d)"""
    k0 = O.rand_scalars(seed, 1)[0]
    d = O.rand_scalars(seed + 1, 1)[0]
    return G.gen_seq(k0, d, n, threads=threads), O.limbs_to_int(k0), O.limbs_to_int(d)


def closed_form(G, scalars, k0, d):
    """(sum s_i (k0 + i d)) * generator as a model point, computed by the oracle's double-and-add"""
    sv = [O.limbs_to_int(x) for x in scalars]
    tot = (sum(sv) * k0 + sum(i * s for i, s in enumerate(sv)) * d) % R
    return jac_to_model(G, G.mul(G.generator(), O.int_to_limbs(tot, 4)))


import contextlib


@contextlib.contextmanager
def bucket_pipeline():
    """Inside the block MSMs of up to 8192 terms on plain bases run the Pippenger bucket pipeline (sort, k_accumulate, fix-up, reduction) instead of
    the bucket-free tree path that serves them since round 4 (dgpu_set_small_msm_max): tests that are ABOUT windows, chunks and buckets use it."""
    from crypto_amd._native import lib
    assert lib().dgpu_set_small_msm_max(0) == 0
    try:
        yield
    finally:
        lib().dgpu_set_small_msm_max(8192)


def on_both_paths(fn):
    """fn() on the tree path (the default for n <= 8192) and on the bucket pipeline; returns both results"""
    a = fn()
    with bucket_pipeline():
        b = fn()
    return a, b


# ---- points of the curves outside the prime-order subgroups (tests/test_gpu_off_subgroup.py) ----------------------------------------------------
H1 = 0x396C8C005555E1568C00AAAB0000AAAB          # #E(Fp) = H1 * R       (y^2 = x^3 + 4)
H2 = 0x5D543A95414E7F1091D50792876A202CD91DE4547085ABAA68A205B2E5A7DDFA628F1CB4D9E82EF21537E293A6691AE1616EC6E786F0C70CF1C38E31C7238E5   # #E'(Fp2) = H2 * R
GLV_LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF   # lambda^2 + lambda + 1 = 0 mod R: the host's split of the G1 scalings (k mod R = k1 + k2 lambda)


def glv_split(k):
    """(k1, k2) with k mod R = k1 + k2 GLV_LAMBDA, k1 < GLV_LAMBDA (what the G1 scaling kernels are fed with)"""
    k2, k1 = divmod(k % R, GLV_LAMBDA)
    return k1, k2


GLS_X = 0xD201000000010000                        # |x| of BLS12-381: the base of the host's split of the G2 scalings (k mod R = d0 + d1 |x| + d2 |x|^2 + d3 |x|^3)


def gls4_split(k):
    """[d0, d1, d2, d3] with k mod R = sum d_j GLS_X^j, d0 .. d2 < GLS_X (what the G2 scaling and fold kernels are fed with)"""
    k %= R
    d = []
    for _ in range(3):
        k, rem = divmod(k, GLS_X)
        d.append(rem)
    return d + [k]


def small_primes_dividing(n, bound=1 << 16):
    out, p = [], 2
    while p < bound:
        if n % p == 0:
            out.append(p)
            while n % p == 0:
                n //= p
        p += 1
    return out


def fp_sqrt(a):
    s = pow(a % P, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def fp2_sqrt(a):
    """a square root in Fp2 (p = 3 mod 4), None if there is none"""
    a1 = M.f2_pow(a, (P - 3) // 4)
    alpha = M.f2_mul(a1, M.f2_mul(a1, a))
    x0 = M.f2_mul(a1, a)
    if alpha == (P - 1, 0):
        x = M.f2_mul((0, 1), x0)
    else:
        x = M.f2_mul(M.f2_pow(M.f2_add(M.F2_ONE, alpha), (P - 1) // 2), x0)
    return x if M.f2_sqr(x) == a else None


def g1_lift(x):
    y = fp_sqrt(x ** 3 + 4)
    return None if y is None else (x % P, y)


def g2_lift(x):
    y = fp2_sqrt(M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.B_TWIST))
    return None if y is None else (x, y)


def _first(lift, xs, ok):
    for x in xs:
        pt = lift(x)
        if pt is not None and ok(pt):
            return pt
    raise AssertionError("no point found")


def _order_ell(mul, pt, n, ell):
    """a point of order exactly ell from pt (n: the group order): the ell-part of pt, then times ell until the next step would be the identity"""
    while n % ell == 0:
        n //= ell
    q = mul(pt, n)
    if q is None:
        return None
    while mul(q, ell) is not None:
        q = mul(q, ell)
    return q


def off_subgroup_points():
    """Model points (ints) outside the prime-order subgroups, with the order each is built to have (None: a multiple of R, not R itself):
    G1: S = (0, 2) and -S (order 3: every point with x = 0 is 3-torsion), T (order divisible by R and by a cofactor prime), S11 (order 11);
    G2: T2 (like T), S2 (order ELL2, the smallest prime dividing the G2 cofactor)."""
    global _OFF
    if _OFF is None:
        S = (0, 2)
        T = _first(g1_lift, range(1, 100), lambda t: M.g1_mul(t, R) is not None)
        S11 = _order_ell(M.g1_mul, _first(g1_lift, range(1, 100), lambda t: _order_ell(M.g1_mul, t, H1 * R, 11) is not None), H1 * R, 11)
        ell2 = small_primes_dividing(H2)[0]
        T2 = _first(g2_lift, ((a, 1) for a in range(100)), lambda t: M.g2_mul(t, R) is not None)
        S2 = _order_ell(M.g2_mul, _first(g2_lift, ((a, 1) for a in range(100)), lambda t: _order_ell(M.g2_mul, t, H2 * R, ell2) is not None), H2 * R, ell2)
        _OFF = {"S": (S, 3), "-S": (M.g1_neg(S), 3), "T": (T, None), "S11": (S11, 11), "T2": (T2, None), "S2": (S2, ell2)}
    return _OFF


_OFF = None


def jac_abi(G, aff):
    """affine ABI words -> the oracle's Jacobian (Z = one)"""
    one = O.fp_to_mont(np.array([[1, 0, 0, 0, 0, 0]], np.uint64)).reshape(-1)
    z = np.zeros(G.AW // 2, np.uint64); z[:6] = one
    return np.concatenate([np.asarray(aff, np.uint64), z])


def plus_multiples(G, bases, e, T_abi, threads=8):
    """B_i = bases_i + e_i T (affine ABI words; e_i = 0 leaves the base as it is), on `threads` host threads"""
    from concurrent.futures import ThreadPoolExecutor
    out = np.array(bases, dtype=np.uint64, copy=True)
    mult = {}
    for k in sorted(set(int(v) for v in e) - {0}):
        mult[k] = G.mul(T_abi, O.int_to_limbs(k, 4))
    idx = np.nonzero(np.asarray(e))[0]

    def work(part):
        for i in part:
            a, inf = G.to_affine(G.add(jac_abi(G, out[i]), mult[int(e[i])]))
            assert not inf
            out[i] = a
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, np.array_split(idx, threads)))
    return out


# ---- every row of a batched scaling against the oracle's double-and-add, on a pool of host threads ---------------------------------------------
def pmap(fn, items):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(fn, items))


def scaled_jac(G, P, p_inf, sc):
    """the oracle's s_i P_i (Jacobian), one scalar per point or ((4,) limbs) one for all; identity points by the flag or by all-zero words"""
    sc = np.asarray(sc, np.uint64)
    pid = ~P.any(axis=1) if p_inf is None else (np.asarray(p_inf, bool) | ~P.any(axis=1))
    return pmap(lambda i: G.mul(P[i], sc if sc.ndim == 1 else sc[i], inf=bool(pid[i])), range(len(P)))


def plus_addends(G, jac, A, a_inf):
    """(rows, flags) of jac_i + A_i as affine ABI words (A None: no addends; identity addends by the flag or by all-zero words); an identity row is
    zero words with the flag set"""
    n = len(jac)
    aid = np.ones(n, bool) if A is None else (~A.any(axis=1) if a_inf is None else (np.asarray(a_inf, bool) | ~A.any(axis=1)))

    def one(i):
        e = jac[i] if aid[i] else G.add(jac[i], jac_abi(G, A[i]))
        a, inf = G.to_affine(e)
        return (np.zeros(G.AW, np.uint64) if inf else a), inf
    res = pmap(one, range(n))
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.uint8)


def mul_add_oracle(G, P, p_inf, sc, A, a_inf):
    """out_i = A_i + s_i P_i by the oracle's mul, add and to_affine: (rows, identity flags)"""
    return plus_addends(G, scaled_jac(G, P, p_inf, sc), A, a_inf)


def first_bad(got, got_inf, want, want_inf):
    """the first rows (at most eight) whose words or identity flag differ"""
    return np.nonzero((got != want).any(axis=1) | (np.asarray(got_inf) != np.asarray(want_inf)))[0][:8]


# ---- the signed radix-2^c recoding of the bucket MSMs (crypto_amd/csrc/digit_codes.hip.h, ps_digits.hip.h) as a big-integer model, and the scalars that
# ---- reach its edges (tests/test_digit_codes_device_code_on_host.py, tests/test_gpu_window_edges.py) -----------------------------------------------------
def window_shape(c):
    """(W, B, M, t): windows, largest digit 2^(c-1), the window mask 2^c - 1, and the scalar bits the top window holds (0: it receives a carry only)"""
    W = 255 // c + 1
    return W, 1 << (c - 1), (1 << c) - 1, 255 - (W - 1) * c


def signed_digits(s, c):
    """the W = 255 // c + 1 digits d_w in [-(B - 1), B], B = 2^(c-1), with sum d_w 2^(c w) = s mod 2^255: a window value above B becomes negative and
    carries one into the next window; the top window holds fewer than c bits and never carries out"""
    W, B, M, _ = window_shape(c)
    s &= (1 << 255) - 1
    out, carry = [], 0
    for w in range(W):
        v = ((s >> (c * w)) & M) + carry
        carry = 1 if v > B else 0
        out.append(v - (carry << c))
    assert carry == 0 and all(-(B - 1) <= d <= B for d in out) and sum(d << (c * w) for w, d in enumerate(out)) == s
    return out


def digit_code(d, bits):
    """the stored spelling of a digit: (|d| - 1) | sign << top bit, all-ones for zero"""
    return (1 << bits) - 1 if d == 0 else (abs(d) - 1) | ((1 << (bits - 1)) if d < 0 else 0)


def ps_part_log(NB):
    """log2 of the buckets per partition of the two-level sort for a set of NB buckets (sort_launch.hip.h ps_part_log)"""
    lg = (NB - 1).bit_length()
    return min(max(lg - 10, 5), 11)


def edge_named(c):
    """the scalars built to put an extreme digit into every window"""
    W, B, M, t = window_shape(c)
    return {
        "maxpos": sum(B << (c * w) for w in range(W - 1)),                                        # every digit +B, the top digit 0
        "minneg": (B + 1) + sum(B << (c * w) for w in range(1, W - 1)),                           # every digit -(B - 1), the top digit +1 out of the carry alone
        "topmax": (((1 << t) - 1) << (c * (W - 1))) + ((B + 1) << (c * (W - 2))),                 # the top digit 2^t: its largest (B at c = 8 and 16, the bare carry at 15 and 17)
        "zero_carry": (B + 1) + (M << c),                                                         # -(B - 1), then 2^c - 1 plus the carry: a zero digit that carries, then +1
        "all_ones": (1 << 255) - 1,                                                               # -1, zeros that each pass the carry on, 2^t
    }


def edge_scalars(c, n_random=0, seed=0, part_logs=None):
    """the edge family of window width c as a list of distinct integers below 2^255: edge_named(c) first, then 0, 1, r - 1, r, r + 1, 2^254, 2^255 - 2,
    the single-digit probes d 2^(c w), the partition borders of the sort (part_logs: the partition widths to border, default that of the shared bucket set
    of a table) and n_random seeded 255-bit values"""
    import random
    W, B, M, t = window_shape(c)
    out = list(edge_named(c).values()) + [0, 1, R - 1, R, R + 1, 1 << 254, (1 << 255) - 2]
    for w in (0, 1, W - 2):
        out += [d << (c * w) for d in (1, 2, B - 1, B, B + 1, M)]
    if t > 0:
        out += [d << (c * (W - 1)) for d in (1, (1 << t) - 1)]
    for k in range(c - 1):                                                                        # one bit of the bucket index at a time (2^k + 1), and all below it (2^k)
        out += [(1 << k) << c, ((1 << k) + 1) << c]
    for pl in ([ps_part_log(B)] if part_logs is None else part_logs):
        for w in (0, W - 2):
            out += [(m1 + 1) << (c * w) for m1 in ((1 << pl) - 1, 1 << pl, B - (1 << pl) - 1, B - (1 << pl))]
    rng = random.Random(1000 * c + seed)
    out += [rng.getrandbits(255) for _ in range(n_random)]
    assert all(0 <= v < 1 << 255 for v in out)
    return list(dict.fromkeys(out))


def edge_coverage_missing(scalars, c, part_log=None, per_window=False):
    """what a vector of integer scalars leaves out of the edge conditions of width c (an empty list: all are met):
    digit +B and digit -(B - 1) in every window below the top, the top window's largest digit 2^t, a zero digit that carries, and the first and last bucket of
    the first and last partition of the sort (buckets 0, 2^pl - 1, B - 2^pl, B - 1; pl = part_log, default that of a table's shared set: in any window;
    per_window: in window 0 and in window W - 2, where every window has a bucket set of its own)"""
    W, B, M, t = window_shape(c)
    pl = ps_part_log(B) if part_log is None else part_log
    seen = [set() for _ in range(W)]
    zero_carry = False
    for s in scalars:
        for w, d in enumerate(signed_digits(s, c)):
            seen[w].add(d)
            zero_carry |= d == 0 and ((s & ((1 << 255) - 1)) >> (c * w)) & M == M
    miss = []
    for w in range(W - 1):
        miss += [("+B", w)] * (B not in seen[w]) + [("-(B-1)", w)] * (-(B - 1) not in seen[w])
    miss += [("top", 1 << t)] * ((1 << t) not in seen[W - 1]) + [("zero digit that carries",)] * (not zero_carry)
    borders = (0, (1 << pl) - 1, B - (1 << pl), B - 1)
    for ws in ([[0], [W - 2]] if per_window else [list(range(W))]):
        have = set(abs(d) - 1 for w in ws for d in seen[w] if d)
        miss += [("bucket", ws[0], b) for b in borders if b not in have]
    return miss


# ---- the chunking of the accumulate stage (crypto_amd/csrc/msm_kernels.hip.h K5 / K6, dyn_chunk.hip.h) as a model: which buckets chunk borders cut, and which
# ---- of the three folds puts each together again (tests/test_acc_layout.py, tests/test_gpu_heavy_buckets.py) ---------------------------------------------
HEAVY_CHUNKS = 16           # a bucket of at least 16 chunk lengths of terms is heavy (dyn[DYN_HEAVY] = 16 CH)
HEAVY_RANGE = 512           # a heavy bucket of more pieces than this is folded range by range, the ranges cut at multiples of 512 chunk indices


def closed_form_dlogs(G, scalars, dlogs):
    """(sum s_i dlog_i) * generator as a model point: closed_form for bases that repeat (scalars: integers or limbs; dlogs: one integer per term)"""
    tot = sum((s if isinstance(s, int) else O.limbs_to_int(s)) * k for s, k in zip(scalars, dlogs)) % R
    return jac_to_model(G, G.mul(G.generator(), O.int_to_limbs(tot, 4)))


class AccBucket:
    """one occupied bucket of an AccLayout: terms, the chunks t0 .. t1 that hold its first and last term, pieces = t1 - t0 + 1, cls (below), and for a
    `multi` bucket ranges = [(k, pieces of range k)] for k = t0 // 512 .. t1 // 512"""
    __slots__ = ("b", "terms", "t0", "t1", "pieces", "cls", "ranges")

    def __repr__(self):
        return "AccBucket(b=%d, terms=%d, t0=%d, t1=%d, pieces=%d, cls=%s, ranges=%s)" % (self.b, self.terms, self.t0, self.t1, self.pieces, self.cls, self.ranges)


class AccLayout:
    """what acc_layout returns: ch, E (sorted pairs), T = ceil(E / ch) chunks, off[0 .. NB] (numpy, off[NB] = E), buckets {index: AccBucket} of the occupied
    ones, heavy = the indices with at least 16 ch terms (class heavy or multi), multi = those of more than 512 pieces"""

    def chunk_slots(self, t):
        """(head_b, tail_b) of chunk t as k_accumulate leaves them: the bucket cut on the chunk's left border (its sum goes to the head slot, also when it is
        cut on the right as well) and the one cut on the right border only (tail slot); None where the slot stays empty"""
        start, end = t * self.ch, min((t + 1) * self.ch, self.E)
        assert start < end
        first = int(np.searchsorted(self.off, start, side="right")) - 1          # the largest b with off[b] <= start
        last = int(np.searchsorted(self.off, end - 1, side="right")) - 1
        head = first if self.off[first] < start else None
        tail = last if self.off[last + 1] > end and not (last == first and head is not None) else None
        return head, tail


def acc_layout(scalars, c, ch, shared, identity_rows=()):
    """The sorted list of an MSM over integer `scalars` at window width c, cut into chunks of ch terms: every non-zero signed digit d of window w is one
    term of bucket w B + |d| - 1 (shared: of bucket |d| - 1 — the one bucket set of a table), buckets in index order.  identity_rows: terms the sort drops
    (rows whose base is an identity, on the routes whose sort sees the bases).  Classes, as the kernels take them: `direct` = one piece (k_accumulate writes
    the bucket itself), `fixup` = cut, fewer than 16 ch terms (one lane of k_fixup), `heavy` = at least 16 ch terms, at most 512 pieces (one block of
    k_fixup_heavy), `multi` = more pieces (k_fixup_heavy_ranges / _join)."""
    from collections import Counter
    W, B, _, _ = window_shape(c)
    NB = B if shared else W * B
    skip = set(identity_rows)
    cnt = np.zeros(NB, np.int64)
    for s, k in Counter(s for i, s in enumerate(scalars) if s and i not in skip).items():
        for w, d in enumerate(signed_digits(s, c)):
            if d:
                cnt[(0 if shared else w * B) + abs(d) - 1] += k
    L = AccLayout()
    L.c, L.ch, L.shared, L.NB = c, ch, shared, NB
    L.off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    L.E = int(L.off[NB])
    L.T = (L.E + ch - 1) // ch
    L.buckets, L.heavy, L.multi = {}, [], []
    for b in np.nonzero(cnt)[0].tolist():
        k = AccBucket()
        k.b, k.terms = b, int(cnt[b])
        k.t0, k.t1 = int(L.off[b]) // ch, (int(L.off[b + 1]) - 1) // ch
        k.pieces = k.t1 - k.t0 + 1
        k.ranges = None
        if k.terms >= HEAVY_CHUNKS * ch:
            L.heavy.append(b)
            k.cls = "multi" if k.pieces > HEAVY_RANGE else "heavy"
            if k.cls == "multi":
                L.multi.append(b)
                k.ranges = [(r, min((r + 1) * HEAVY_RANGE - 1, k.t1) - max(r * HEAVY_RANGE, k.t0) + 1) for r in range(k.t0 // HEAVY_RANGE, k.t1 // HEAVY_RANGE + 1)]
        else:
            k.cls = "direct" if k.pieces == 1 else "fixup"
        L.buckets[b] = k
    return L


# ---- the sort stage of the bucket MSMs as a model (crypto_amd/csrc/psort_kernels.hip.h, sort_kernels.hip.h; the hooks dgpu_selftest_psort / _sort_sweep / _scan /
# ---- _dyn_chunk of include/dock_gpu_dev.h; tests/test_gpu_sort_stage.py, tests/test_sort_stage_host.py) ------------------------------------------------------
SORT_GUARD = 64                      # DGPU_SELFTEST_GUARD: words behind every output buffer of the hooks
SORT_SENTINEL = 0xA5A5A5A5           # DGPU_SELFTEST_SENTINEL: what the hooks fill outputs and guards with before the launch
RESIDENT_ACC_LANES = 131072          # the lanes k_accumulate keeps resident (dyn_chunk.hip.h)


def scalar_words(vals):
    """integers below 2^256 -> (n, 8) little-endian 32-bit words, the layout the kernels read"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint32).reshape(-1, 8).copy()


def signed_digit_matrix(scalars, c):
    """signed_digits for a whole vector at once: (n, W) int64 (bit 255 is masked, as the kernels do).  The windows come from the bit matrix of the scalars, the
    carry runs window by window over all rows; a sample of rows is compared with signed_digits itself"""
    W, B, M, _ = window_shape(c)
    n = len(scalars)
    raw = np.frombuffer(b"".join((int(s) & ((1 << 255) - 1)).to_bytes(32, "little") for s in scalars), dtype=np.uint8).reshape(n, 32)
    bits = np.unpackbits(raw, axis=1, bitorder="little")
    bits = np.concatenate([bits, np.zeros((n, W * c - 256), np.uint8)], axis=1) if W * c > 256 else bits[:, :W * c]
    win = bits.reshape(n, W, c).astype(np.int64) @ (1 << np.arange(c, dtype=np.int64))
    D = np.zeros((n, W), np.int64)
    carry = np.zeros(n, np.int64)
    for w in range(W):
        v = win[:, w] + carry
        carry = (v > B).astype(np.int64)
        D[:, w] = v - (carry << c)
    assert not carry.any()
    for i in sorted(set(list(range(min(n, 24))) + [n - 1, n // 2, n // 3])):
        assert D[i].tolist() == signed_digits(int(scalars[i]), c), i
    return D


def sort_model(scalars, c, key_wstride, val_base, val_wstride, idflag=None, flag_base=0):
    """What the sort of the (bucket, term) pairs of integer `scalars` at width c must produce: (pairs, counts).  pairs: (E, 2) int64, sorted by (key, val), one
    row per non-zero signed digit d of window w of row i: key = w key_wstride + |d| - 1 (key_wstride = 0: the one bucket set of a table; B: a set per window),
    val = (val_base + w val_wstride + i) | sign << 31.  Rows with idflag[flag_base + i] != 0 are dropped.  counts: terms per bucket, NB = B or W B entries."""
    W, B, _, _ = window_shape(c)
    assert key_wstride in (0, B)
    NB = W * B if key_wstride else B
    n = len(scalars)
    D = signed_digit_matrix(scalars, c)
    live = np.ones(n, bool) if idflag is None else (np.asarray(idflag)[flag_base:flag_base + n] == 0)
    on = (D != 0) & live[:, None]
    i_idx, w_idx = np.nonzero(on)
    d = D[i_idx, w_idx]
    key = w_idx.astype(np.int64) * key_wstride + np.abs(d) - 1
    val = (val_base + w_idx.astype(np.int64) * val_wstride + i_idx) | ((d < 0).astype(np.int64) << 31)
    assert ((val & 0x7FFFFFFF) == val_base + w_idx * val_wstride + i_idx).all()          # the index stays below the sign bit
    order = np.lexsort((val, key))
    pairs = np.stack([key[order], val[order]], axis=1)
    counts = np.bincount(key, minlength=NB).astype(np.int64)
    assert len(counts) == NB
    return pairs, counts


def dyn_chunk_model(E, fixed_ch, min_chunk, max_chunks, lanes_per_chunk, T_max, nb_shared, trace=None):
    """(ch, T, heavy, E, 0): the chunking of the accumulation for E sorted pairs, in unbounded integers, from the description of choose_chunk (dock_core.hip):
    the shortest chunk of min_chunk terms, doubled (up to 4096) while there are more than max_chunks chunks; once the launch exceeds one round of the chip's
    resident lanes the chunk count is snapped to whole rounds (rounded to nearest, at least one) and the length follows, if it lies in 16 .. 4096; on a shared
    bucket set of nb_shared buckets ONE round is taken when the average run is at least half that round's chunk and the chunk is at most 4096.  A forced
    length (fixed_ch) is kept.  On the device (k_dyn_chunk) there are never more chunks than T_max partial slots (T_max = 0: no cap); a bucket is heavy from
    16 chunk lengths on.  trace: a set that receives the names of the branches taken."""
    t = trace if trace is not None else set()
    ceil = lambda a, b: -(-a // b)
    ch = fixed_ch
    if ch:
        t.add("fixed")
    else:
        ch = min_chunk
        while E // ch > max_chunks and ch < 4096:
            ch *= 2
            t.add("doubled")
        if E // ch > max_chunks:
            t.add("doubling stopped at 4096")
        resident = RESIDENT_ACC_LANES // lanes_per_chunk
        chunks = ceil(E, ch)
        if chunks > resident:
            rounds = max(1, (2 * chunks + resident) // (2 * resident))          # chunks / resident rounded to nearest, halves up
            t.add("rounds up" if rounds * resident >= chunks else "rounds down")
            length = ceil(E, rounds * resident)
            if 16 <= length <= 4096:
                ch = length
                t.add("snapped")
            else:
                t.add("len below 16" if length < 16 else "len above 4096")
        else:
            t.add("one round or less")
        if nb_shared:
            run, one = E // nb_shared, ceil(E, resident)
            if one > ch and 2 * run >= one and one <= 4096:
                ch = one
                t.add("shared: one round")
            else:
                t.add("shared: " + ("one <= ch" if one <= ch else "short runs" if 2 * run < one else "one > 4096"))
    if T_max and ceil(E, ch) > T_max:
        ch = ceil(E, T_max)
        t.add("T_max binds")
    elif T_max:
        t.add("T_max free")
    return ch, ceil(E, ch), 16 * ch, E, 0


def check_sort(off, entries, NB, cap, pairs, counts, what=""):
    """The device's off[NB + 1 + guard] and entries[cap + guard] (cap = n W slots) against sort_model's (pairs, counts): off starts at 0, never decreases and
    ends at E; bucket by bucket the multiset of entries equals the model's (the order inside a bucket is the arrival order of LDS atomics); every slot from E
    on and every guard word still holds the sentinel."""
    off = np.asarray(off, np.uint32).astype(np.int64)
    entries = np.asarray(entries, np.uint32).astype(np.int64)
    E = len(pairs)
    assert len(off) == NB + 1 + SORT_GUARD and len(entries) == cap + SORT_GUARD and E <= cap, what
    assert off[0] == 0, (what, off[:4])
    sizes = np.diff(off[:NB + 1])
    assert (sizes >= 0).all(), (what, "off decreases at", np.nonzero(sizes < 0)[0][:8])
    assert off[NB] == E, (what, "off[NB]", int(off[NB]), "model", E)
    assert (sizes == counts).all(), (what, "bucket sizes differ at", np.nonzero(sizes != counts)[0][:8])
    assert (off[NB + 1:] == SORT_SENTINEL).all(), (what, "guard of off[] written")
    assert (entries[E:] == SORT_SENTINEL).all(), (what, "entries[] written at or past E", (E + np.nonzero(entries[E:] != SORT_SENTINEL)[0][:8]).tolist())
    key = np.repeat(np.arange(NB, dtype=np.int64), sizes)
    order = np.lexsort((entries[:E], key))
    got = np.stack([key[order], entries[:E][order]], axis=1)
    bad = np.nonzero((got != pairs).any(axis=1))[0]
    assert len(bad) == 0, (what, "first differing pairs (device, model)", got[bad[:4]].tolist(), pairs[bad[:4]].tolist())
