"""GPU (-m gpu): the window edges of the bucket MSMs.  Every bucket MSM recodes its scalars into signed radix-2^c digits, sorts the (bucket, term) pairs
— per-window sweeps (sort_kernels.hip.h) or the two-level partition sort (psort_kernels.hip.h) — and reduces the bucket set; uniformly random scalars reach
the edges of all three only by chance.  Here the scalars are util.edge_scalars(c): digit +B (the one bucket whose index has the top bit set: the top
marginal class, the last partition, the last lane of the reduction) and digit -(B - 1) in every window below the top, the largest digit of the top window
(B itself at c = 8 and 16, from a scalar in [r, 2^255); the bare carry at c = 15 and 17, where the top window holds no scalar bits), a zero digit that
carries, single buckets at chosen indices (one set bit of the index at a time), the first and last bucket of the first and last partition — at every window
width the pipelines accept, widths 17, 19 and 21 of the tables included (17 is DGPU_TABLE_C_WITNESS with its own compile-time sort kernels).
Bases are points with known discrete logarithms k0 + i d (util.seq_bases) and the expected point is one double-and-add of the oracle (util.closed_form): a
term in the wrong bucket or window moves the sum by a non-zero multiple of its own base.  Every case first asserts, with the model util.signed_digits,
that its vector does occupy the digits and buckets it is about.  All comparisons are exact."""
import random
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu

N = 1539                                        # three 512-scalar sort tiles plus 3
ANCHORS = (0, 511, 512, 1023, 1024, 1538)       # first / last lanes of the tiles, the last term
NP = (1 << 17) + 77                             # the smallest size at which the plain pipeline takes the partition sort, off a tile multiple
OFF = 513                                       # a handle offset that is no tile multiple


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)


@pytest.fixture(scope="module")
def base_sets():
    """one set of N bases per curve (and a second one in G1), shared by the cases and never written to: {name: (bases, k0, d)}"""
    return {"G1": U.seq_bases(O.G1, N, 8101, threads=16), "G1b": U.seq_bases(O.G1, N, 8103, threads=16), "G2": U.seq_bases(O.G2, N, 8105, threads=16)}


@pytest.fixture(scope="module")
def big_g1():
    return U.seq_bases(O.G1, NP + OFF, 8201, threads=16)


def limbs(ints):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(-1, 4).copy()


def to_ints(sc):
    return [int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 for a, b, c, d in sc.tolist()]


class EdgeCase:
    """the two scalar vectors of a case of n terms at width c: the edge family at `anchors` and at seeded other indices; `probe`: every other scalar 0 (a
    few dozen isolated buckets), `mixed`: the others random.  Three more rows carry edge scalars on identity bases: ident[0] is flagged, ident[1] has
    all-zero words, ident[2] both."""

    def __init__(self, c, n, seed, anchors=ANCHORS, part_logs=None):
        self.c, self.n = c, n
        fam = U.edge_scalars(c, part_logs=part_logs)
        rng = random.Random(seed)
        free = sorted(set(rng.sample(range(n), len(fam) + 3 + len(anchors))) - set(anchors))       # (more than enough distinct indices off the anchors)
        rng.shuffle(free)
        pos = list(anchors) + free[:len(fam) - len(anchors)]
        assert len(pos) == len(fam) and len(set(pos)) == len(pos)
        self.pos = pos
        self.ident = free[len(fam):len(fam) + 3]
        named = U.edge_named(c)
        self.probe = [0] * n
        self.mixed = to_ints(O.rand_scalars(seed, n))
        for v in (self.probe, self.mixed):
            for p, s in zip(pos, fam):
                v[p] = s
            for j, key in zip(self.ident, ("maxpos", "minneg", "topmax")):
                v[j] = named[key]
        self.inf = np.zeros(n, np.uint8)
        self.inf[self.ident[0]] = 1; self.inf[self.ident[2]] = 1

    def bases(self, bases):
        b = bases.copy()
        b[self.ident[1]] = 0; b[self.ident[2]] = 0
        return b

    def live(self, ints):
        """the scalars with zeros where the base is an identity: what the expected sum and the coverage are taken over"""
        out = list(ints)
        for j in self.ident:
            out[j] = 0
        return out

    def vectors(self):
        return (("probe", self.probe), ("mixed", self.mixed))

    def assert_coverage(self, part_log=None, per_window=False):
        """both vectors occupy every edge of width c on rows whose base is not an identity (taken over the rows that hold the family: more rows only add)"""
        for name, v in self.vectors():
            live = self.live(v)
            assert U.edge_coverage_missing([live[p] for p in self.pos], self.c, part_log, per_window) == [], name


def curve_of(gname):
    return (ca.G1, O.G1) if gname.startswith("G1") else (ca.G2, O.G2)


def mont(ints):
    """the scalars as field elements in Montgomery form (a value in [r, 2^255) is the element s mod r)"""
    return O.fr_to_mont(limbs([s % U.R for s in ints]))


@pytest.mark.parametrize("gname,c", [("G1", c) for c in range(16, 23)] + [("G2", 17), ("G2", 20)])
def test_table_pipeline_at_every_width(gname, c, base_sets):
    """precomputed-multiples tables: the shared bucket set of 2^(c-1) buckets, the partition sort with its run-time and its three compile-time shapes,
    the bit-marginal reduction.  The closed form on both vectors; the same limbs from the plain handle, the Montgomery-scalar call and resident scalars."""
    curve, G = curve_of(gname)
    bases0, k0, d = base_sets[gname]
    ec = EdgeCase(c, N, 8300 + c)
    ec.assert_coverage()
    bases = ec.bases(bases0)
    tab = ca.DeviceBases(curve, bases, ec.inf).precompute(c)
    assert tab.table_shape() == (N, c, 255 // c + 1)
    plain = ca.DeviceBases(curve, bases, ec.inf)
    assert plain.table_shape() is None
    for name, ints in ec.vectors():
        sc = limbs(ints)
        r = tab.msm_bigint(sc)
        assert U.jac_to_model(G, r) == U.closed_form(G, limbs(ec.live(ints)), k0, d), name
        assert (plain.msm_bigint(sc) == r).all(), name
        assert (tab.msm_bigint(mont(ints), montgomery=True) == r).all(), name
        ds = ca.DeviceScalars(sc)
        assert (tab.msm_resident(ds) == r).all(), name
        ds.free()
    tab.free(); plain.free()


def test_one_sort_serves_the_width_17_tables(base_sets):
    """the prover's arrangement at DGPU_TABLE_C_WITNESS: ONE sorted scalar list (made for the first G1 table, no identity filter) serves that table, a second
    G1 table with identity rows and the G2 table; each result equals the table's own msm_resident limb for limb, and the closed form of its own bases"""
    c = ca.TABLE_C_WITNESS
    assert c == 17
    ec = EdgeCase(c, N, 8400)
    ec.assert_coverage()
    none = np.zeros(N, np.uint8)
    sets = [("G1", base_sets["G1"][0], none, False), ("G1b", ec.bases(base_sets["G1b"][0]), ec.inf, True), ("G2", ec.bases(base_sets["G2"][0]), ec.inf, True)]
    tabs = [ca.DeviceBases(curve_of(g)[0], b, inf).precompute(c) for g, b, inf, _ in sets]
    assert all(t.table_shape() == (N, 17, 16) for t in tabs) and tabs[0].same_table_shape(tabs[1]) and tabs[0].same_table_shape(tabs[2])
    for name, ints in ec.vectors():
        ds = ca.DeviceScalars(limbs(ints))
        srt = ca.SortedScalars(tabs[0], ds, N)
        for (g, _, _, has_ident), t in zip(sets, tabs):
            G = curve_of(g)[1]
            r = t.msm_sorted(srt)
            assert (r == t.msm_resident(ds)).all(), (name, g)
            _, k0, d = base_sets[g]
            assert U.jac_to_model(G, r) == U.closed_form(G, limbs(ec.live(ints) if has_ident else ints), k0, d), (name, g)
        srt.free(); ds.free()
    for t in tabs:
        t.free()


@pytest.mark.parametrize("gname,c", [("G1", c) for c in range(7, 19)] + [("G2", 8), ("G2", 15), ("G2", 16)])
def test_plain_pipeline_sweeps_at_every_width(gname, c, base_sets, twin):
    """the plain pipeline below 2^17 terms: stored digit codes (2 bytes up to c = 16, 4 above), per-window LDS sweeps over bucket ranges, one bucket set per
    window.  The family also borders every power-of-two bucket range of 32 buckets and more, whichever split the sweeps take."""
    curve, G = curve_of(gname)
    bases0, k0, d = base_sets[gname]
    ec = EdgeCase(c, N, 8500 + c, part_logs=range(5, c - 1))
    ec.assert_coverage()
    bases = ec.bases(bases0)
    with U.bucket_pipeline():
        assert lib().dgpu_set_window_bits(c) == 0
        try:
            for name, ints in ec.vectors():
                r = ca.msm_bigint(curve, bases, limbs(ints), ec.inf)
                assert U.jac_to_model(G, r) == U.closed_form(G, limbs(ec.live(ints)), k0, d), name
        finally:
            lib().dgpu_set_window_bits(0)


@pytest.mark.parametrize("c", [16, 17, 18, 19])
def test_plain_pipeline_partition_sort(c, big_g1, twin):
    """the plain pipeline from 2^17 terms on: the partition sort with key = w B + |digit| - 1 over W B buckets — the compile-time shapes <16, 16> and <17, 16>
    with a bucket set per window, and the run-time form at c = 18 and 19 (wider sets need several GB of workspace for no other code path).  The edge family
    sits at the borders of the 512-scalar tiles, the last, partial tile included, the rest is random.  One-shot call on the first NP bases, and the same
    vector on a resident handle from base 513 on (the closed form of the shifted pairing)."""
    G, curve = O.G1, ca.G1
    bases, k0, d = big_g1
    W, B, _, _ = U.window_shape(c)
    plain_log = U.ps_part_log(W * B)
    tiles = (1, 2, 3, 128, 129, 255, 256)
    anchors = [0] + [t * 512 - 1 for t in tiles] + [t * 512 for t in tiles] + [t * 512 + 1 for t in (128, 256)] + [NP - 39, NP - 2, NP - 1]
    ec = EdgeCase(c, NP, 8600 + c, anchors=tuple(anchors), part_logs=[U.ps_part_log(B), plain_log])
    ints = ec.mixed
    for j in ec.ident:                                       # (no identity bases in this case: those rows keep their edge scalars on ordinary bases)
        assert ints[j] != 0
    at_edges = [ints[p] for p in ec.pos]
    assert U.edge_coverage_missing(at_edges, c, part_log=plain_log, per_window=True) == [] and U.edge_coverage_missing(at_edges, c) == []
    sc = limbs(ints)
    assert lib().dgpu_set_window_bits(c) == 0
    try:
        ca.bases_cache_clear()                               # (a first sighting: the one-shot call stays on the plain pipeline)
        r = ca.msm_bigint(curve, bases[:NP], sc)
        assert U.jac_to_model(G, r) == U.closed_form(G, sc, k0, d)
        db = ca.DeviceBases(curve, bases)
        assert db.table_shape() is None
        r = db.msm_bigint(sc, offset=OFF)
        assert U.jac_to_model(G, r) == U.closed_form(G, sc, k0 + OFF * d, d)
        db.free()
    finally:
        lib().dgpu_set_window_bits(0)
        ca.bases_cache_clear()


def test_plain_pipeline_forced_width_22_takes_the_sweeps(big_g1, twin):
    """a forced width of 22 at 2^17 terms and more: the partition sort's scatter would need 245 KB of LDS for its 12288 partitions (sort_launch.hip.h
    ps_scatter_lds_bytes, plain_psort_fits; tests/test_sort_stage_host.py has the arithmetic), a launch that cannot run — plain_geometry leaves the shape to the
    sweeps.  The stage timers show the route, the closed form the point."""
    G, curve, c = O.G1, ca.G1, 22
    bases, k0, d = big_g1
    W, B, _, _ = U.window_shape(c)
    ec = EdgeCase(c, NP, 8600 + c, part_logs=[U.ps_part_log(B), U.ps_part_log(W * B)])
    ints = ec.mixed
    assert U.edge_coverage_missing([ints[p] for p in ec.pos], c, part_log=U.ps_part_log(W * B), per_window=True) == []
    sc = limbs(ints)
    assert lib().dgpu_set_window_bits(c) == 0
    try:
        ca.bases_cache_clear()
        ca.prof.enable(True); ca.prof.reset()
        r = ca.msm_bigint(curve, bases[:NP], sc)
        stages = ca.prof.read()
        assert U.jac_to_model(G, r) == U.closed_form(G, sc, k0, d)
        assert "msm.count" in stages and "msm.scatter" in stages and "msm.psort" not in stages, sorted(stages)
    finally:
        ca.prof.enable(False)
        lib().dgpu_set_window_bits(0)
        ca.bases_cache_clear()
