"""GPU (-m gpu): the folds that put a bucket together again after chunk borders cut it (msm_kernels.hip.h K6), at their thresholds and range borders.
k_accumulate gives every lane a chunk of CH sorted terms; a bucket that spans several chunks is left in pieces (the tail slot of its first chunk, the head
slots of the following ones) and folded by k_fixup (fewer than 16 CH terms: one lane), by k_fixup_heavy (at least 16 CH terms, at most 512 pieces: one
block, strided sums and block_tree_fold) or, beyond 512 pieces, range by range (k_fixup_heavy_ranges cuts at multiples of 512 chunk indices into slot
2 k + (k == k0), k_fixup_heavy_join folds the ranges).  Uniformly random scalars make no heavy bucket at all, so every count and offset here is chosen:
a scalar v < B puts digit v into window 0 and nothing elsewhere, v 2^(c w) moves it to window w, and with one term per (bucket, term) pair the number
of terms of every bucket, the order of the buckets and the offset of every run are what the case lists (fillers of fewer than 16 CH terms set the offsets).
Bases are points with known discrete logarithms (util.seq_bases), distinct within a bucket unless the case says otherwise, the expected point is
util.closed_form (util.closed_form_dlogs where bases repeat) and the comparison is exact: a piece that is dropped, doubled or folded into the wrong bucket
moves the sum by a non-zero multiple of known logarithms.
Every case asserts, BEFORE it compares points, (1) with the model util.acc_layout (tests/test_acc_layout.py checks it on the CPU) that it holds the structure
it is named after, and (2) with dgpu_dev_get_acc_last that the device ran the model's chunk length, chunk count, heavy-bucket count and multi-range count:
a change of the chunk rule would otherwise turn every case into a k_fixup case unnoticed.  Unless a case says otherwise the chunk is forced to 16 terms
(the smallest: the smallest cases), the window width is fixed and the pipeline is the bucket pipeline; all three knobs are restored in `finally`.
Each call prints one line `acc <case>: CH T heavy multi` (pytest -s shows them)."""
import contextlib
import ctypes as C
import random
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu

CH = 16
NP = (1 << 17) + 77          # the smallest size at which the plain pipeline takes the partition sort, off a tile multiple (tests/test_gpu_window_edges.py)
N_G2 = 24600                 # the longest G2 case: two long buckets side by side
PIECES = (16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512)
CURVES = {"G1": (ca.G1, O.G1), "G2": (ca.G2, O.G2)}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)


@pytest.fixture(scope="module")
def base_sets():
    """one set of bases per curve, shared by the cases (each takes a prefix) and never written to: {name: (bases, k0, d)}"""
    return {"G1": U.seq_bases(O.G1, NP, 9101, threads=16), "G2": U.seq_bases(O.G2, N_G2, 9105, threads=16)}


def limbs(ints):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(-1, 4).copy()


@contextlib.contextmanager
def knobs(c, ch):
    """the bucket pipeline at window width c with chunks of ch terms (0: the device's own rule)"""
    L = lib()
    try:
        with U.bucket_pipeline():
            assert L.dgpu_set_window_bits(c) == 0 and L.dgpu_set_chunk(ch) == 0
            yield
    finally:
        L.dgpu_set_chunk(0)
        L.dgpu_set_window_bits(0)


def acc_last():
    w = np.zeros(6, np.uint32)
    assert lib().dgpu_dev_get_acc_last(w.ctypes.data_as(C.c_void_p)) == 0
    return dict(zip(("ch", "T", "thr", "E", "multi", "heavy"), (int(v) for v in w)))


def model_words(lay):
    return {"ch": lay.ch, "T": lay.T, "thr": 16 * lay.ch, "E": lay.E, "multi": len(lay.multi), "heavy": len(lay.heavy)}


def confirm_route(lay, name):
    got = acc_last()
    print("acc %s: CH %d T %d heavy %d multi %d" % (name, got["ch"], got["T"], got["heavy"], got["multi"]))
    assert got == model_words(lay), name


def single_window(counts, c, per_window=None):
    """counts[j] terms for the j-th digit value in turn: v = j + 1 in window 0 up to the window's last value below B, then window 1, ... -> (scalars in bucket
    order, the bucket index w B + v - 1 of every j)"""
    B = 1 << (c - 1)
    per = B - 1 if per_window is None else per_window
    sc, idx = [], []
    for j, k in enumerate(counts):
        w, m = divmod(j, per)
        sc += [(m + 1) << (c * w)] * k
        idx.append(w * B + m)
    return sc, idx


def shuffled(sc, seed, n=None):
    """the scalars at seeded rows of a vector of n (default: as many) terms, zeros elsewhere: the sort has to bring every run together"""
    n = len(sc) if n is None else n
    rows = random.Random(seed).sample(range(n), len(sc))
    out = [0] * n
    for r, s in zip(rows, sc):
        out[r] = s
    return out


def run_handle(gname, base_sets, ints, lay, name, offset=0):
    """the MSM of `ints` over the first bases of the set on a plain resident handle; the route, then the point"""
    curve, G = CURVES[gname]
    bases, k0, d = base_sets[gname]
    db = ca.DeviceBases(curve, bases[:len(ints)])
    assert db.table_shape() is None
    sc = limbs(ints)
    r = db.msm_bigint(sc)
    confirm_route(lay, name)
    assert U.jac_to_model(G, r) == U.closed_form(G, sc, k0, d), name
    db.free()


# ---- the accessor itself ------------------------------------------------------------------------------------------------------------------------
FRESH_PROCESS = r"""
import ctypes as C, numpy as np
import torch
import oracle_c as O, util as U, crypto_amd as ca
ca.init(0)
w = np.zeros(6, np.uint32); p = w.ctypes.data_as(C.c_void_p)
with ca.twin() as T:
    assert T.dgpu_dev_get_acc_last(p) == -3                      # no call has taken a slot yet
    bases, k0, d = U.seq_bases(O.G1, 300, 9901)
    db = ca.DeviceBases(ca.G1, bases)                            # takes a slot and reserves every slot's workspace: nothing accumulated
    assert T.dgpu_dev_get_acc_last(p) == -3
    sc = np.zeros((300, 4), np.uint64); sc[:, 0] = 1
    r = db.msm_bigint(sc)                                        # the bucket-free small path: still nothing
    assert T.dgpu_dev_get_acc_last(p) == -3 and not w.any()
    with U.bucket_pipeline():
        assert (db.msm_bigint(sc) == r).all()
    assert T.dgpu_dev_get_acc_last(p) == 0 and w.tolist() == [16, 19, 256, 300, 0, 1], w      # 300 terms in one bucket: 19 chunks of 16, one heavy bucket
    assert T.dgpu_dev_get_acc_last(None) == -3
    db.free()
print("acc_last ok")
"""


def test_accessor_refuses_until_an_accumulation_has_run():
    """in a process of its own (the answer depends on everything the process did before): DGPU_E_BADARG before the first call, after an upload and after an MSM
    on the small path; the six words after the first bucket MSM"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "oracle"), os.path.join(root, "tests"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", FRESH_PROCESS], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "acc_last ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]


# ---- a. the heavy threshold ------------------------------------------------------------------------------------------------------------------
def threshold_counts(ch):
    """buckets of 16 ch - 1, 16 ch, 16 ch + 1 terms at the start offsets 0, 1, ch - 1 modulo ch (and 16 ch + 2 at ch - 1: the one way to 18 pieces), each with
    a cut bucket of fewer than 16 ch terms directly in front (it starts on a chunk border and ends where the offset says) and directly behind"""
    counts, marks, pos = [], [], 0

    def add(k):
        nonlocal pos
        counts.append(k); pos += k
    for extra, offsets in ((-1, (0, 1, ch - 1)), (0, (0, 1, ch - 1)), (1, (0, 1, ch - 1)), (2, (ch - 1,))):
        for o in offsets:
            if pos % ch:
                add(ch - pos % ch)                          # (ends on a chunk border)
            add(ch + o if o else 2 * ch)
            marks.append((len(counts), extra, o))
            add(16 * ch + extra)
            add(2 * ch + 3)
    return counts, marks


@pytest.mark.parametrize("gname,ch", [("G1", 16), ("G1", 128), ("G2", 16)])
def test_heavy_threshold(gname, ch, base_sets, twin):
    """16 CH - 1 terms: k_fixup (k_fixup_pair in G2) walks 16 or 17 pieces on one lane, the most it ever does; 16 CH and 16 CH + 1: k_fixup_heavy folds 16, 17
    or 18.  A chunk then holds the head slot of a heavy bucket and the tail slot of its one-lane neighbour, another the neighbour's head slot and the heavy
    bucket's tail slot.  With chunks of 16 and of 128 terms."""
    c = 8
    counts, marks = threshold_counts(ch)
    sc, idx = single_window(counts, c)
    ints = shuffled(sc, 9200 + ch)
    lay = U.acc_layout(ints, c, ch, shared=False)
    want_pieces = {(-1, 0): 16, (-1, 1): 16, (-1, ch - 1): 17, (0, 0): 16, (0, 1): 17, (0, ch - 1): 17, (1, 0): 17, (1, 1): 17, (1, ch - 1): 17, (2, ch - 1): 18}
    shared_front = shared_behind = 0
    for j, extra, o in marks:
        front, x, behind = lay.buckets[idx[j - 1]], lay.buckets[idx[j]], lay.buckets[idx[j + 1]]
        assert x.terms == 16 * ch + extra and lay.off[x.b] % ch == o and x.pieces == want_pieces[(extra, o)], (extra, o, x)
        assert x.cls == ("fixup" if extra < 0 else "heavy") and front.cls == "fixup" and behind.cls == "fixup", (extra, o)
        if extra >= 0 and o:
            assert lay.chunk_slots(x.t0) == (front.b, x.b); shared_front += 1
        if extra >= 0 and lay.off[x.b + 1] % ch:
            assert lay.chunk_slots(x.t1) == (x.b, behind.b); shared_behind += 1
    assert shared_front >= 4 and shared_behind >= 4 and len(lay.heavy) == 7 and lay.multi == []
    with knobs(c, ch):
        run_handle(gname, base_sets, ints, lay, "a.threshold %s ch=%d" % (gname, ch))


# ---- b. the piece counts of the block tree ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_block_tree_piece_counts(gname, base_sets, twin):
    """one call per piece count p on either side of every power of two block_tree_fold's `s2 >= items` compares against (a block holds 256 points in G1, 128
    lane pairs in G2) and of the strided loop's wrap: a bucket of p pieces that starts on a chunk border (its last piece one term where that is still heavy)
    and, from 18 pieces on, a second one whose first and last piece hold one term each"""
    c = 8
    curve, G = CURVES[gname]
    bases, k0, d = base_sets[gname]
    with knobs(c, CH):
        db = ca.DeviceBases(curve, bases[:2 * CH * 512 + 4 * CH])
        for p in PIECES:
            n_a = CH * (p - 1) + 1 if CH * (p - 1) + 1 >= 16 * CH else CH * p
            counts = [CH, n_a]
            if p >= 18:
                end = CH + n_a
                counts += [(CH - 1 - end) % CH or CH, CH * (p - 2) + 2]
            sc, idx = single_window(counts, c)
            ints = shuffled(sc, 9300 + p)
            lay = U.acc_layout(ints, c, CH, shared=False)
            xs = [lay.buckets[idx[j]] for j in range(1, len(counts), 2)]
            assert all(x.cls == "heavy" and x.pieces == p for x in xs) and len(lay.heavy) == len(xs) and lay.multi == [], (p, xs)
            assert lay.off[xs[0].b] % CH == 0 and (len(xs) == 1 or (lay.off[xs[1].b] % CH == CH - 1 and lay.off[xs[1].b + 1] % CH == 1)), p
            lm = limbs(ints)
            r = db.msm_bigint(lm)
            confirm_route(lay, "b.pieces %s p=%d" % (gname, p))
            assert U.jac_to_model(G, r) == U.closed_form(G, lm, k0, d), p
        db.free()


# ---- c. the range border ---------------------------------------------------------------------------------------------------------------------------
RANGE_BORDER = {   # name: (counts, the bucket the case is about, (terms, t0, t1, pieces, class), ranges)
    "512 pieces, aligned": ([8192], 0, (8192, 0, 511, 512, "heavy"), None),
    "8192 terms from offset 1": ([1, 8192], 1, (8192, 0, 512, 513, "multi"), [(0, 512), (1, 1)]),
    "8193 terms, aligned": ([8193], 0, (8193, 0, 512, 513, "multi"), [(0, 512), (1, 1)]),
    "300 pieces across chunk 512": ([200] * 32 + [4800], 32, (4800, 400, 699, 300, "heavy"), None),      # the class goes by pieces, not by crossing a range border
}


@pytest.mark.parametrize("case", list(RANGE_BORDER))
def test_range_border(case, base_sets, twin):
    c = 8
    counts, j, want, ranges = RANGE_BORDER[case]
    sc, idx = single_window(counts, c)
    ints = shuffled(sc, 9400 + len(counts))
    lay = U.acc_layout(ints, c, CH, shared=False)
    x = lay.buckets[idx[j]]
    assert (x.terms, x.t0, x.t1, x.pieces, x.cls) == want and x.ranges == ranges and lay.heavy == [x.b] and lay.multi == ([x.b] if ranges else [])
    with knobs(c, CH):
        run_handle("G1", base_sets, ints, lay, "c.border " + case)


# ---- d. the layout of the ranges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_two_long_buckets_in_one_range(gname, base_sets, twin):
    """A ends and B starts inside range 1 (slots 2 and 3 of the range sums): A's last range holds one piece (t1 = 512), B's first range holds one piece
    (t0 = 1023).  In G1 a third bucket, C, spans three ranges, the middle one wholly inside it."""
    c = 8
    counts = [5, 8191] + [255] * 32 + [24] + [8196]                       # A = terms 5 .. 8195, B = terms 16380 .. 24575
    if gname == "G1":
        counts += [250, 250, 250, 250, 24, 16968]                        # C = terms 25600 .. 42567: chunks 1600 .. 2660
    sc, idx = single_window(counts, c)
    ints = shuffled(sc, 9500)
    lay = U.acc_layout(ints, c, CH, shared=False)
    A, B = lay.buckets[idx[1]], lay.buckets[idx[35]]
    assert (A.t0, A.t1, A.ranges) == (0, 512, [(0, 512), (1, 1)]) and (B.t0, B.t1, B.ranges) == (1023, 1535, [(1, 1), (2, 512)])
    assert A.t1 // U.HEAVY_RANGE == B.t0 // U.HEAVY_RANGE == 1
    if gname == "G1":
        Cb = lay.buckets[idx[41]]
        assert (Cb.t0, Cb.t1, Cb.ranges) == (1600, 2660, [(3, 448), (4, 512), (5, 101)]) and lay.multi == [A.b, B.b, Cb.b] == lay.heavy
    else:
        assert lay.multi == [A.b, B.b] == lay.heavy
    with knobs(c, CH):
        run_handle(gname, base_sets, ints, lay, "d.ranges " + gname)


# ---- e. more work than blocks ------------------------------------------------------------------------------------------------------------------------
def spread(v, c, windows):
    return sum(v << (c * w) for w in range(windows))


def table_cases():
    """on the shared bucket set of a width-16 table v sum_w 2^(16 w) puts 16 entries per term into bucket v - 1: one chunk of 16.  A first term with scalar 1
    alone shifts every run to offset 1."""
    W = 16
    return {
        "520 heavy buckets": [1] + [spread(2 + j, 16, W) for j in range(520) for _ in range(16)],                      # k_fixup_heavy's 512 blocks go round twice
        "35 multi-range buckets": [1] + [spread(2 + j, 16, W) for j in range(35) for _ in range(513)],                 # more than the 32 rows of the range grid and the 32 join blocks
        "one bucket of 66 ranges": [1] + [spread(2, 16, W)] * (65 * 512 + 1),                                         # more than the 64 columns of the range grid
    }


@pytest.mark.parametrize("case", ["520 heavy buckets", "35 multi-range buckets", "one bucket of 66 ranges"])
def test_more_buckets_and_ranges_than_blocks_on_a_table(case, base_sets, twin):
    c = 16
    G, curve = O.G1, ca.G1
    bases, k0, d = base_sets["G1"]
    sc = table_cases()[case]
    assert all(0 < s < 1 << 255 for s in sc)                                           # (every MSM entry point refuses a scalar with bit 255 set)
    ints = shuffled(sc, 9600)
    lay = U.acc_layout(ints, c, CH, shared=True)
    if case == "520 heavy buckets":
        assert len(lay.heavy) == 520 > 512 and lay.multi == [] and all(lay.buckets[b].pieces == 17 for b in lay.heavy)
    elif case == "35 multi-range buckets":
        assert len(lay.multi) == 35 > 32 and lay.heavy == lay.multi and all(lay.buckets[b].pieces == 514 for b in lay.multi)
    else:
        assert lay.multi == [1] == lay.heavy and len(lay.buckets[1].ranges) == 66 > 64 and lay.buckets[1].ranges[0] == (0, 512) and lay.buckets[1].ranges[-1] == (65, 2)
    with knobs(0, CH):
        tab = ca.DeviceBases(curve, bases[:len(ints)]).precompute(c)
        assert tab.table_shape() == (len(ints), 16, 16)
        lm = limbs(ints)
        r = tab.msm_bigint(lm)
        confirm_route(lay, "e.table " + case)
        assert U.jac_to_model(G, r) == U.closed_form(G, lm, k0, d)
        tab.free()


def test_more_heavy_buckets_than_blocks_on_the_plain_pipeline(base_sets, twin):
    """v (1 + 2^c) fills windows 0 and 1 per term: 260 values of 256 terms are 520 heavy buckets of the plain pipeline's per-window sets"""
    c = 10
    sc = [1] + [spread(1 + j, c, 2) for j in range(260) for _ in range(256)]
    ints = shuffled(sc, 9650)
    lay = U.acc_layout(ints, c, CH, shared=False)
    assert len(lay.heavy) == 520 > 512 and lay.multi == [] and sorted(set(lay.buckets[b].pieces for b in lay.heavy)) == [17]
    with knobs(c, CH):
        run_handle("G1", base_sets, ints, lay, "e.plain 520 heavy buckets")


# ---- f. sums that degenerate -------------------------------------------------------------------------------------------------------------------------
DEGENERATE = {   # name: per bucket (the heavy one, then the multi-range one) the numbers of +P and of -P terms
    "all the same base": ((512, 0), (8208, 0)),
    "as many +P as -P": ((256, 256), (4104, 4104)),
    "more +P than -P": ((300, 212), (5000, 3208)),
}


@pytest.mark.parametrize("case", list(DEGENERATE))
def test_one_base_per_bucket(case, base_sets, twin):
    """Every term of the heavy bucket (digit 1) is +-P, every term of the multi-range bucket (digit 2) is +-Q, with aligned counts: every piece is a multiple of
    16 P, so the additions of fold_pieces, block_tree_fold and the join meet equal and opposite operands, and with as many -P as +P the bucket's sum is the
    identity and bucket_inf has to say so.  -P is the negative digit of 2^c - v, whose carry also lands every such term in window 1's first bucket (one bucket
    of P's and Q's).  The order inside a bucket is the arrival order of the sort's atomics: only what holds in every order is asserted — the sum."""
    c = 8
    G, curve = O.G1, ca.G1
    bases, k0, d = base_sets["G1"]
    (hp, hn), (mp, mn) = DEGENERATE[case]
    sc = [1] * hp + [(1 << c) - 1] * hn + [2] * mp + [(1 << c) - 2] * mn
    rows = [0] * (hp + hn) + [1] * (mp + mn)
    order = random.Random(9700).sample(range(len(sc)), len(sc))
    sc, rows = [sc[i] for i in order], [rows[i] for i in order]
    lay = U.acc_layout(sc, c, CH, shared=False)
    h, m = lay.buckets[0], lay.buckets[1]
    assert (h.terms, h.cls, h.pieces) == (512, "heavy", 32) and (m.terms, m.cls, m.pieces) == (8208, "multi", 513) and lay.off[1] % CH == 0
    assert (128 in lay.buckets) == (hn + mn > 0) and (hn + mn == 0 or lay.buckets[128].terms == hn + mn)
    with knobs(c, CH):
        db = ca.DeviceBases(curve, bases[rows])
        r = db.msm_bigint(limbs(sc))
        confirm_route(lay, "f.one base " + case)
        assert U.jac_to_model(G, r) == U.closed_form_dlogs(G, sc, [k0 + i * d for i in rows]), case
        db.free()


@pytest.mark.parametrize("route", ["handle", "one-shot"])
def test_identity_rows_inside_a_heavy_bucket(route, base_sets, twin):
    """600 terms of one bucket, 40 of them on bases flagged as the identity and 40 on all-zero words.  On a resident handle the sort sees the bases and drops
    those rows (520 terms are left: still heavy); the one-shot call sorts while its bases are still on their way, the rows stay in the list and k_accumulate
    passes over them."""
    c = 8
    G, curve = O.G1, ca.G1
    bases0, k0, d = base_sets["G1"]
    sc = shuffled([1] * 600 + [2] * 37, 9750)
    n = len(sc)
    in_heavy = [i for i, s in enumerate(sc) if s == 1]
    flagged, zeroed = in_heavy[5:45], in_heavy[300:340]
    inf = np.zeros(n, np.uint8); inf[flagged] = 1
    bases = bases0[:n].copy(); bases[zeroed] = 0
    live = list(sc)
    for i in flagged + zeroed:
        live[i] = 0
    lay = U.acc_layout(sc, c, CH, shared=False, identity_rows=flagged + zeroed if route == "handle" else ())
    assert lay.heavy == [0] and lay.buckets[0].terms == (520 if route == "handle" else 600) and lay.multi == []
    with knobs(c, CH):
        if route == "handle":
            db = ca.DeviceBases(curve, bases, inf)
            r = db.msm_bigint(limbs(sc))
            db.free()
        else:
            r = ca.msm_bigint(curve, bases, limbs(sc), inf)
        confirm_route(lay, "f.identity rows " + route)
        assert U.jac_to_model(G, r) == U.closed_form(G, limbs(live), k0, d)


# ---- g. the other routes to the same kernels ---------------------------------------------------------------------------------------------------------
MIX = [5, 16 * CH - 1, 16 * CH, 16 * CH + 1, CH - 5, 512 * CH, 512 * CH + 1, 1, 500 * CH]


def assert_mix(lay, idx):
    """the threshold and the borders in small: one term short of heavy, exactly heavy, one more; 512 pieces from a chunk border (chunks 49 .. 560); 513 pieces
    (561 .. 1073: ranges 1 and 2, the last piece one term); 501 pieces from that same chunk on, across chunk 1536"""
    k = [lay.buckets[b] for b in idx]
    assert [x.cls for x in k] == ["direct", "fixup", "heavy", "heavy", "direct", "heavy", "multi", "direct", "heavy"]
    assert (k[5].t0, k[5].pieces) == (49, 512) and (k[6].t0, k[6].t1, k[6].ranges) == (561, 1073, [(1, 463), (2, 50)]) and (k[8].t0, k[8].t1, k[8].pieces) == (1073, 1573, 501)


def test_partition_sort_route(base_sets, twin):
    """the plain pipeline from 2^17 terms on: the partition sort with one bucket set per window in the key; the case's terms sit at seeded rows, every other
    scalar is zero"""
    c = 16
    sc, idx = single_window(MIX, c)
    ints = shuffled(sc, 9800, NP)
    lay = U.acc_layout(ints, c, CH, shared=False)
    assert_mix(lay, idx)
    with knobs(c, CH):
        run_handle("G1", base_sets, ints, lay, "g.partition sort")


def test_table_route(base_sets, twin):
    """a table: the shared bucket set, the chunk rule's nb_shared argument, the heavy list made by the table's own sort"""
    c = 16
    G, curve = O.G1, ca.G1
    bases, k0, d = base_sets["G1"]
    sc, idx = single_window(MIX, c)
    ints = shuffled(sc, 9810)
    lay = U.acc_layout(ints, c, CH, shared=True)
    assert_mix(lay, idx)
    with knobs(0, CH):
        tab = ca.DeviceBases(curve, bases[:len(ints)]).precompute(c)
        lm = limbs(ints)
        r = tab.msm_bigint(lm)
        confirm_route(lay, "g.table")
        assert U.jac_to_model(G, r) == U.closed_form(G, lm, k0, d)
        tab.free()


def test_shared_sort_route_with_shifted_rows(base_sets, twin):
    """SortedScalars made for a table of N rows, used by a table of the rows 37 .. N - 1 (RowMap): the chunking and the heavy list are derived from off[]
    (launch_dyn_chunk, k_flag_heavy) and the SKIP_ID instance of k_accumulate passes over the entries of rows 0 .. 36 and over identity rows, some of each
    inside the heavy and the multi-range bucket.  The list holds every row, so the layout is that of all scalars."""
    c, shift = 16, 37
    G, curve = O.G1, ca.G1
    bases, k0, d = base_sets["G1"]
    sc, idx = single_window(MIX, c)
    ints = shuffled(sc, 9820)
    N = len(ints)
    lay = U.acc_layout(ints, c, CH, shared=True)
    assert_mix(lay, idx)
    v_heavy, v_multi = idx[5] + 1, idx[6] + 1
    assert any(ints[i] == v_heavy for i in range(shift)) and any(ints[i] == v_multi for i in range(shift))
    ident = [i for i in range(shift, N) if ints[i] == v_heavy][10:30] + [i for i in range(shift, N) if ints[i] == v_multi][100:140]
    inf = np.zeros(N, np.uint8); inf[ident] = 1
    live = [0 if i < shift or inf[i] else s for i, s in enumerate(ints)]
    with knobs(0, CH):
        full = ca.DeviceBases(curve, bases[:N]).precompute(c)
        part = ca.DeviceBases(curve, bases[shift:N], inf[shift:]).precompute(c)
        ds = ca.DeviceScalars(limbs(ints))
        srt = ca.SortedScalars(full, ds, N)
        r = part.msm_sorted(srt, row_shift=shift)
        confirm_route(lay, "g.shared sort, shifted rows")
        assert U.jac_to_model(G, r) == U.closed_form(G, limbs(live), k0, d)
        srt.free(); ds.free(); part.free(); full.free()


def test_the_devices_own_chunk_rule(base_sets, twin):
    """no forced chunk: the model takes CH from the accessor, and the case only has to hold at least one heavy and one multi-range bucket at that CH"""
    c = 8
    G, curve = O.G1, ca.G1
    bases, k0, d = base_sets["G1"]
    sc, _ = single_window(MIX, c)
    ints = shuffled(sc, 9830)
    lm = limbs(ints)
    with knobs(c, 0):
        db = ca.DeviceBases(curve, bases[:len(ints)])
        r = db.msm_bigint(lm)
        got = acc_last()
        lay = U.acc_layout(ints, c, got["ch"], shared=False)
        assert len(lay.multi) >= 1 and len(lay.heavy) > len(lay.multi)
        confirm_route(lay, "g.own chunk rule")
        assert U.jac_to_model(G, r) == U.closed_form(G, lm, k0, d)
        db.free()
