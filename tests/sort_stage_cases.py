"""The inputs of tests/test_gpu_sort_stage.py, built on the host: every builder ASSERTS that its vector reaches the branch of the sort kernels it is named
after (crypto_amd/csrc/psort_kernels.hip.h, sort_kernels.hip.h) before anything is launched.  tests/test_sort_stage_host.py runs the same builders without a
GPU, so a case that stops reaching its branch fails on every machine.  Each builder returns a dict: sc (integer scalars), c, mode ("shared": the one bucket
set of a table, key_wstride = 0; "window": a set per window, key_wstride = B) and whatever else the case fixes."""
import random
import numpy as np
import util as U

PS_TILE, PS_DIRECT_CAP, PS_WC_TILE, PS_WC_MIN_PAIRS = 512, 16384, 16384, 65536       # sort_launch.hip.h
PSORT_SHAPES = [(16, 16), (17, 16), (20, 13), (18, 15), (19, 14)]                    # <16, 16>, <17, 16>, <20, 13> at compile time; the others at run time
PSORT_SIZES = [1539, 4173, 8192, 8249]
MODES = ["shared", "window"]
G1_RULE = dict(min_chunk=16, max_chunks=300000, lanes_per_chunk=1)                   # acc_geometry (msm_driver.hip.h)
G2_RULE = dict(min_chunk=32, max_chunks=150000, lanes_per_chunk=2)


def geometry(c, mode):
    """(W, B, key_wstride, NB, part_log, P) as msm_device_ranges ("window") and pre_sort ("shared") compute them"""
    W, B, _, _ = U.window_shape(c)
    NB = B if mode == "shared" else W * B
    pl = U.ps_part_log(NB)
    return W, B, (0 if mode == "shared" else B), NB, pl, (NB + (1 << pl) - 1) >> pl


def tile_of_block(b, ntiles):
    """ps_tile_of_block: blocks go round the eight XCDs, each XCD takes consecutive tiles; the tiles past a multiple of eight go straight"""
    per = ntiles >> 3
    return (b & 7) * per + (b >> 3) if b < (per << 3) else b


def partition_loads(case):
    """pairs per partition of the case's sort"""
    W, B, kws, NB, pl, P = geometry(case["c"], case["mode"])
    return np.bincount(case["pairs"][:, 0] >> pl, minlength=P)


def finish(case, val_base=0, val_wstride=None, idflag=None, flag_base=0):
    """adds the model's pairs and counts (util.sort_model) and the value spelling: a table's rows are val_wstride = n apart, the plain pipeline's are 0 apart"""
    W, B, kws, NB, pl, P = geometry(case["c"], case["mode"])
    n = len(case["sc"])
    case.update(n=n, W=W, B=B, key_wstride=kws, NB=NB, part_log=pl, P=P, val_base=val_base, idflag=idflag, flag_base=flag_base,
                val_wstride=(n if case["mode"] == "shared" else 0) if val_wstride is None else val_wstride)
    case["pairs"], case["counts"] = U.sort_model(case["sc"], case["c"], kws, case["val_base"], case["val_wstride"], idflag, flag_base)
    assert n * W // P < PS_WC_MIN_PAIRS                      # every case is far below the size at which the product itself takes write combining
    return case


_SHAPE = {}


def shape_case(c, mode, n):
    """edge scalars of both partition widths of width c padded with seeded random values.  n = 1539: 4 tiles, fewer than 8, the tile map is the identity;
    4173: 9 tiles, one past a multiple of eight (the eight blocks of the XCD round take one tile each, so the map is still the identity); 8192: exactly 16 full
    tiles, the first size at which the map permutes; 8249: 17 tiles, sixteen permuted, the last one straight and partly filled"""
    if (c, mode, n) in _SHAPE:
        return _SHAPE[(c, mode, n)]
    W, B, kws, NB, pl, P = geometry(c, mode)
    sc = U.edge_scalars(c, part_logs=sorted({U.ps_part_log(B), U.ps_part_log(W * B)}))
    assert len(sc) <= n
    rng = random.Random(100000 * c + n)
    sc = sc + [rng.getrandbits(255) for _ in range(n - len(sc))]
    rng.shuffle(sc)
    ntiles = (n + PS_TILE - 1) // PS_TILE
    tmap = [tile_of_block(b, ntiles) for b in range(ntiles)]
    assert sorted(tmap) == list(range(ntiles))
    assert {1539: ntiles == 4 and tmap == list(range(4)), 4173: ntiles == 9 and n % PS_TILE != 0 and tmap[8] == 8, 8192: ntiles == 16 and n % PS_TILE == 0 and tmap != list(range(16)),
            8249: ntiles == 17 and tmap[:16] != list(range(16)) and tmap[16] == 16}[n]
    assert U.edge_coverage_missing(sc, c, part_log=pl, per_window=(mode == "window")) == []
    assert (mode, c) != ("window", 18) or (P == 960 and P & (P - 1))                       # a partition count that is no power of two
    case = finish(dict(sc=sc, c=c, mode=mode))
    _SHAPE[(c, mode, n)] = case
    return case


HOT = ["equal", "alternating", "witness"]


def hot_case(kind, c, mode, n=4173):
    """lds_inc_agg: lanes of a wave that target the counter of the wave's first active lane are served by one atomic.  equal: every lane of every wave, in every
    window; alternating: two values lane by lane, so half the lanes share the first lane's counter and the others issue their own; witness: mostly 0 and 1
    (idle lanes and one hot bucket) with a few random rows"""
    rng = random.Random(7 * c + len(kind))
    a, b = rng.getrandbits(255), rng.getrandbits(255)
    if kind == "equal":
        sc = [a] * n
    elif kind == "alternating":
        sc = [a if i % 2 == 0 else b for i in range(n)]
    else:
        sc = [rng.getrandbits(255) if i % 97 == 5 else (i * 7 // 3) % 2 for i in range(n)]
    case = finish(dict(sc=sc, c=c, mode=mode))
    D = U.signed_digit_matrix(sc, c)
    if kind == "equal":
        assert (D == D[0]).all() and case["counts"].max() >= n and set(case["counts"].tolist()) <= {0} | {n * k for k in range(1, case["W"] + 1)}
    elif kind == "alternating":
        assert (D[0::2] == D[0]).all() and (D[1::2] == D[1]).all() and (D[0] != D[1]).any()
    else:
        small = sum(1 for s in sc if s < 2)
        assert small > 0.9 * n and 0 < sc.count(0) and case["counts"][0] >= sc.count(1) > n // 3 and len(case["pairs"]) < n * case["W"] // 4
    return case


def _partition0_rows(k, rng):
    """k scalars sum d_w 2^(16 w) with every d_w in 1 .. 32: sixteen pairs each, all of bucket < 32 (no carries: 32 <= B; the top window holds bits 240 .. 254)"""
    return [sum(rng.randint(1, 32) << (16 * w) for w in range(16)) for _ in range(k)]


def direct_cap_case(target):
    """shared set at c = 16 (partitions of 32 buckets): partition 0 holds exactly `target` pairs (16384 = PS_DIRECT_CAP: everything staged; 16385: one slot
    goes straight to memory; 32768, 41600: most of the partition does; in the write-combining form: one full tile, one pair more, two full tiles, two and a
    tail), partition 1 and the last partition hold a few rows, so that a neighbour starts at lo != 0"""
    rng = random.Random(target)
    full, rest = divmod(target, 16)
    sc = _partition0_rows(full, rng) + [rng.randint(1, 32) for _ in range(rest)]
    B = 1 << 15
    sc += [33, 40, 64, 64 << 16] + [B, B - 1, (B - 5) << 32]                     # buckets 32 .. 63: partition 1; buckets B - 32 .. B - 1: the last partition
    rng.shuffle(sc)
    case = finish(dict(sc=sc, c=16, mode="shared"))
    loads = partition_loads(case)
    assert case["part_log"] == 5 and case["P"] == 1024
    assert loads[0] == target and loads[1] == 4 and loads[-1] == 3 and loads.sum() == target + 7 == len(case["pairs"])
    assert {16384: target == PS_DIRECT_CAP == PS_WC_TILE, 16385: target == PS_DIRECT_CAP + 1, 32768: target == 2 * PS_WC_TILE, 41600: 2 * PS_WC_TILE < target < 3 * PS_WC_TILE}[target]
    return case


def direct_cap_window_case():
    """a set per window at c = 16 (partitions of 512 buckets): 16500 rows with values 1 .. 512 are 16500 pairs in partition 0 of window 0, past PS_DIRECT_CAP"""
    rng = random.Random(16500)
    B = 1 << 15
    sc = [rng.randint(1, 512) for _ in range(16500)] + [513, 1024, B << 16, (B - 1) << (16 * 14), 3 << (16 * 15), (B - 1) << 240]
    rng.shuffle(sc)
    case = finish(dict(sc=sc, c=16, mode="window"))
    loads = partition_loads(case)
    assert case["part_log"] == 9 and case["P"] == 1024
    assert loads[0] == 16500 > PS_DIRECT_CAP and loads[1] == 2 and loads[-1] == 1          # (the top window holds 15 bits: its digit B - 1 is bucket B - 2 of window 15, in the last partition of all)
    return case


def sparse_partitions_case():
    """uniform scalars at c = 20 with a set per window: 3328 partitions for 54 k pairs, most hold a handful, and those of the top window past its 15 bits hold
    none (lo == hi)"""
    case = dict(shape_case(20, "window", 4173))
    loads = partition_loads(case)
    assert case["P"] == 3328 and (loads == 0).sum() > 200 and np.median(loads[loads > 0]) < 64 and loads.max() < PS_WC_TILE
    return case


FILTERS = ["none", "row0", "last", "tile", "scattered"]


def filter_case(kind, n=1539):
    """the identity filter of a table's sort (c = 17, shared set) with every offset off zero: flag_base = val_base = 37, val_wstride = n + 37.  The 37 bytes in
    front of the call's rows are set, so a kernel that forgot flag_base would drop rows 0 .. 36"""
    base = shape_case(17, "shared", n)
    if kind == "none":
        flags = None
    else:
        flags = np.zeros(37 + n, np.uint8)
        flags[:37] = 1
        rows = {"row0": [0], "last": [n - 1], "tile": list(range(PS_TILE, 2 * PS_TILE)), "scattered": random.Random(n).sample(range(n), n // 10)}[kind]
        flags[37 + np.array(rows)] = 1
        assert kind != "tile" or (flags[37 + PS_TILE:37 + 2 * PS_TILE].all() and not flags[37 + PS_TILE - 1] and not flags[37 + 2 * PS_TILE])
    case = finish(dict(sc=base["sc"], c=17, mode="shared"), val_base=37, val_wstride=n + 37, idflag=flags, flag_base=37)
    if flags is not None:
        kept = finish(dict(sc=base["sc"], c=17, mode="shared"), val_base=37, val_wstride=n + 37)
        assert len(case["pairs"]) < len(kept["pairs"])                                   # the dropped rows had pairs
    return case


BAD = ["clean", "bit255", "bit255 in an identity row"]


def bad_case(kind, n=1539):
    """the bad word as k_ps_count1 reads it: set when ANY row below n has bit 255 set, live or not; the pairs are those of the masked scalar"""
    sc = list(shape_case(16, "shared", n)["sc"])
    row = 700
    flags = np.zeros(n, np.uint8)
    flags[[3, row if kind == BAD[2] else 4]] = 1
    if kind != "clean":
        assert sc[row] != 0
        sc[row] |= 1 << 255
    case = finish(dict(sc=sc, c=16, mode="shared"), idflag=flags)
    case["want_bad"] = int(any(s >> 255 for s in sc))
    assert case["want_bad"] == (kind != "clean")
    return case


HEAVY = ["at the threshold", "more than the list holds", "threshold from the chunk rule"]


def heavy_case(kind, c, mode, thr):
    """single-digit rows in window 0 (value v -> bucket v - 1).  at the threshold: buckets of thr - 1, thr and thr + 1 terms, the last two are heavy; more
    than the list holds: nine heavy buckets for a list of four; every case has a crowd of light buckets around them"""
    if kind == HEAVY[1]:
        loads = {3 + 11 * k: thr + k for k in range(9)}
        cap = 4
    else:
        loads = {5: thr - 1, 9: thr, 70: thr + 1}
        cap = 8
    sc = [v for v, k in loads.items() for _ in range(k)] + list(range(100, 400))
    random.Random(thr).shuffle(sc)
    case = finish(dict(sc=sc, c=c, mode=mode))
    case["heavy_cap"], case["thr"] = cap, thr
    case["want_heavy"] = sorted(int(b) for b in np.nonzero(case["counts"] >= thr)[0])
    assert case["want_heavy"] == sorted(v - 1 for v, k in loads.items() if k >= thr) and len(case["want_heavy"]) == (9 if kind == HEAVY[1] else 2)
    assert kind == HEAVY[1] or sorted(case["counts"][[4, 8, 69]].tolist()) == [thr - 1, thr, thr + 1]
    return case


SWEEP_WIDTHS = [7, 12, 13, 16, 17, 22]


def sweep_geometry(c):
    """(W, B, NB, wide, RANGES, rb_log, grid) of plain_geometry's sweeps"""
    W, B, _, _ = U.window_shape(c)
    R = 1
    while (B // R) * 4 > 64 * 1024 or W * R < 256:
        if B // R <= 64:
            break
        R *= 2
    return W, B, W * B, c > 16, R, (B // R - 1).bit_length(), 8 * ((W + 7) // 8) * R


def sweep_case(c, n=1539):
    """the per-window sweeps: 2-byte codes up to c = 16 and 4-byte codes above; one bucket range (c = 7) and many; W off a multiple of eight, so that padding
    blocks of the XCD-aware block map run; n off a multiple of eight, so that padding codes are swept"""
    W, B, NB, wide, R, rb, grid = sweep_geometry(c)
    sc = U.edge_scalars(c, part_logs=[U.ps_part_log(W * B)])
    rng = random.Random(31 * c)
    sc = sc + [rng.getrandbits(255) for _ in range(n - len(sc))]
    rng.shuffle(sc)
    assert len(sc) == n and n % 8 and (grid > W * R) == (c in (7, 12, 13, 22)) and wide == (c in (17, 22))
    assert {7: R == 1, 12: R > 1, 13: R > 1, 16: R > 1, 17: R > 1, 22: R == 128}[c] and (B >> rb) == R
    flags = np.zeros(n, np.uint8)
    flags[[0, n - 1] + rng.sample(range(1, n - 1), n // 9)] = 1
    case = dict(sc=sc, c=c, mode="window", flags=flags)
    finish(case)
    case["pairs_flagged"], case["counts_flagged"] = U.sort_model(sc, c, B, 0, 0, flags, 0)
    assert len(case["pairs_flagged"]) < len(case["pairs"])
    return case


SCAN_SIZES = [1, 4095, 4096, 4097, 4096 * 1024 - 1, 4096 * 1024, 4096 * 1024 + 1, 4096 * 2048 + 5]


def scan_case(NB):
    """counters for launch_scan with a total below 2^32.  Up to 4097: dense; beyond: zeros with sparse spikes (and the very first and last counter set), so
    that the sum in front of every later block is large and a carry lost between two rounds of k_scan_sums (1024 block sums a round) moves the result"""
    rng = np.random.default_rng(NB)
    if NB <= 4097:
        cnt = rng.integers(0, 1 << 19, NB, dtype=np.int64)
    else:
        cnt = np.zeros(NB, np.int64)
        cnt[rng.integers(0, NB, 3000)] = rng.integers(1, 1 << 20, 3000)
        cnt[0], cnt[NB - 1], cnt[4096 * 1024 - 2] = 77, 99, 5
        if NB > 4096 * 1024:
            cnt[4096 * 1024] = 3
    blocks = (NB + 4095) // 4096
    assert cnt.sum() < 1 << 32
    assert {1: blocks == 1, 4095: blocks == 1, 4096: blocks == 1, 4097: blocks == 2, 4096 * 1024 - 1: blocks == 1024, 4096 * 1024: blocks == 1024,
            4096 * 1024 + 1: blocks == 1025, 4096 * 2048 + 5: blocks == 2049}[NB]
    if blocks > 1024:                       # a second round of k_scan_sums whose carry is not zero; from 2049 blocks a third, whose carry is the sum of two
        assert cnt[:4096 * 1024].sum() > 0 and cnt[4096 * 1024:].sum() > 0
    if blocks > 2048:
        assert cnt[4096 * 1024:4096 * 2048].sum() > 0 and cnt[4096 * 2048:].sum() > 0
    return cnt


def chunk_rule_table(rule):
    """[(E, fixed_ch, T_max, nb_shared)] around every branch of the chunk rule for one curve's parameters (G1_RULE / G2_RULE)"""
    m, mc, lanes = rule["min_chunk"], rule["max_chunks"], rule["lanes_per_chunk"]
    r = U.RESIDENT_ACC_LANES // lanes
    Es = {0, 1, 2, 15, 16, 17, (1 << 32) - 1, (1 << 32) - 4096, (1 << 32) - 4097, (1 << 32) - 4095, (1 << 31) - 1, 1 << 31}
    ch = m
    while ch <= 4096:                                        # E / ch == max_chunks, one term less, and the first E with one chunk more — at every doubling
        Es |= {mc * ch + d for d in (-1, 0, ch - 1, ch, ch + 1)}
        ch *= 2
    Es |= {r * m + d for d in (-1, 0, 1, m)}                 # chunks == resident, and one more
    for k in (3, 5, 7):                                      # chunks / resident at x.5: the first count that rounds up, and the last that rounds down
        Es |= {m * (k * r // 2) + d for d in (-m, -m + 1, -1, 0, 1, m)}
    Es |= {24 * r, 32 * r - 1, 32 * r, 32 * r + 1}           # two rounds of 12 (below 16: refused), of exactly 16, of 17
    Es |= {4096 * 3 * r + d for d in (-1, 0, 1)}             # three rounds of exactly 4096, and one term more: 4097 is refused
    Es |= {48 * r + d for d in (-1, 0, 1)}                   # (shared set of 2 r buckets) 2 * run == one == 48, and one term less: run = 23
    Es |= {4096 * r + d for d in (-1, 0, 1)}                 # one == 4096 and 4097
    rows = []
    for E in sorted(Es):
        assert 0 <= E < 1 << 32
        for nb in (0, 1 << 15, 1 << 16, 2 * r):
            rows.append((E, 0, 0, nb))
            # the partial slots acc_geometry reserves for the largest E of the call: the rule without the run-length term on Emax = the next power of two
            Emax = max(1 << 16, 1 << max(E - 1, 1).bit_length()) if E < 1 << 31 else (1 << 32) - 1
            T_max = U.dyn_chunk_model(Emax, 0, m, mc, lanes, 0, 0)[1]
            rows.append((E, 0, T_max, nb))
        if E <= 1 << 27:
            rows += [(E, 0, 1, 0), (E, 0, 1000, 1 << 16), (E, 16, 7, 0)]         # a cap that binds, also on a forced length
        rows += [(E, f, 0, nb) for f in (16, 19, 4096) for nb in (0, 1 << 16)]
    return rows


CHUNK_BRANCHES = ["fixed", "doubled", "doubling stopped at 4096", "rounds up", "rounds down", "snapped", "len below 16", "len above 4096", "one round or less",
                  "shared: one round", "shared: one <= ch", "shared: short runs", "shared: one > 4096", "T_max binds", "T_max free"]
