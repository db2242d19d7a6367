"""MSM and Miller-loop kernels on curve points OUTSIDE the prime-order subgroups.

arkworks' `VariableBaseMSM::msm_bigint` / `msm_unchecked` and `Pairing::multi_miller_loop` take any `Affine` (points deserialised with
`Validate::No` included), and the drop-in MSM path (the resident-bases cache) does no subgroup test.  Bases of small order also make the
special cases of the bucket additions (a sum that becomes the identity partway and goes on, P + P, P + (-P)) happen in nearly every bucket.

The points (tests/util.py off_subgroup_points): in G1 S = (0, 2) of order 3 (every point with x = 0 is 3-torsion; its x words are all zero
and its y words are not, so a kernel that decides "identity" from x alone is wrong on it), -S, T of large order outside G1, S11 of order 11;
in G2 T2 of large order outside G2 and S2 of order 13 (the smallest prime of the G2 cofactor).  Bulk bases B_i = G_i + e_i S with known
discrete logs for G_i give a closed form for every size: sum s_i B_i = (sum s_i k_i) G + ((sum s_i e_i) mod 3) S.

The scaled Miller loop (dgpu_multi_miller_loop_scaled) keeps its contract "P in G1": its scaling computes k1 P + k2 phi(P) for the host's GLV
split (k1, k2) of m, which is [m] P in G1 only.  For P = +-S, phi(S) = S, so the scaled point is ((k1 + k2) mod 3) S: a pair whose split
is non-zero can still become the identity ON THE DEVICE, which the line-product kernels must treat as the neutral line.  Those tests pin the
pipelined and the two-call form against each other and against the oracle fed ((k1 + k2) mod 3) P, not against arkworks' double-and-add.

Low-order Q is out of scope: the doubling chain of a Q of small order can pass through the identity, and arkworks' line formulas have no
special case for that.  Only Q of large order outside G2 (T2) is tested.

The tests without the gpu mark check the constructions themselves (orders, the closed form, the oracle against the big-integer model)."""
import ctypes as C
import numpy as np
import pytest
import oracle_c as O
import util as U
import bls12_381_model as M

gpu = pytest.mark.gpu
FP_ONE = O.fp_to_mont(np.array([[1, 0, 0, 0, 0, 0]], np.uint64)).reshape(-1)


def pts():
    """the constructed points as ABI words (12 / 24 u64) and their orders"""
    off = U.off_subgroup_points()
    a = {k: (U.g2_abi(p)[0] if k in ("T2", "S2") else U.g1_abi(p)[0]) for k, (p, _) in off.items()}
    return a, {k: o for k, (_, o) in off.items()}


def group(gname):
    import crypto_amd as ca
    return (ca.G1, O.G1) if gname == "G1" else (ca.G2, O.G2)


def normalised(G, jac):
    """oracle result -> the ABI's canonical Jacobian triple (affine, Z = one / identity: one, one, 0)"""
    a, inf = G.to_affine(jac)
    h = G.AW // 2
    z = np.zeros(h, np.uint64)
    if inf:
        x = np.zeros(h, np.uint64); x[:6] = FP_ONE
        return np.concatenate([x, x, z])
    z[:6] = FP_ONE
    return np.concatenate([a, z])


def affine_abi(G, aff):
    """affine ABI words of a point that is not the identity -> the ABI's canonical Jacobian triple"""
    return U.jac_abi(G, aff)


def bulk(gname, n, seed, threads=16):
    """B_i = G_i + e_i T with G_i = (k0 + i d) G, T = S (G1, e_i < 3) or S2 (G2, e_i < 13); returns (bases, k0, d, e, T, ell)"""
    _, G = group(gname)
    a, orders = pts()
    tname = "S" if gname == "G1" else "S2"
    ell = orders[tname]
    g, k0, d = U.seq_bases(G, n, seed, threads=threads)
    e = np.random.default_rng(seed).integers(0, ell, n)
    return U.plus_multiples(G, g, e, a[tname], threads=8), k0, d, e, a[tname], ell


def closed_form(G, sc, k0, d, e, T, ell, extra_g=0):
    """(sum s_i (k0 + i d) + extra_g) G + ((sum s_i e_i) mod ell) T as the ABI's canonical Jacobian triple"""
    sv = [O.limbs_to_int(x) for x in sc]
    tot = (sum(sv) * k0 + sum(i * s for i, s in enumerate(sv)) * d + extra_g) % U.R
    et = sum(s * int(x) for s, x in zip(sv, e)) % ell
    return normalised(G, G.add(G.mul(G.generator(), O.int_to_limbs(tot, 4)), G.mul(T, O.int_to_limbs(et, 4))))


def mixed(gname, n, seed):
    """bulk bases with the other constructed points planted: T, S11 (G1) / T2 (G2), +-S, duplicates, a flagged identity"""
    bases, k0, d, e, T, ell = bulk(gname, n, seed)
    a, _ = pts()
    inf = np.zeros(n, np.uint8)
    plant = ["T", "S11", "S", "-S", "S", "S"] if gname == "G1" else ["T2", "S2", "S2", "T2"]
    for j, name in enumerate(plant):
        if 1 + 7 * j < n:
            bases[(1 + 7 * j) % n] = a[name]
    if n > 40:
        bases[40:44] = bases[1]                         # the same off-subgroup point four times
        inf[n - 1] = 1
    return bases, inf


def every_path(gname, bases, sc, inf=None, table_bits=16):
    """the MSM of (bases, sc) through every entry point: (name, normalised Jacobian words)"""
    import crypto_amd as ca
    curve, _ = group(gname)
    n = min(len(bases), len(sc))
    out = [("one-shot", ca.msm_bigint(curve, bases, sc, inf))]
    if n <= 8192:
        with U.bucket_pipeline():
            out.append(("buckets", ca.msm_bigint(curve, bases, sc, inf)))
    out.append(("montgomery", ca.msm_unchecked(curve, bases, O.fr_to_mont(sc), inf)))
    out.append(("strided", ca.msm_strided(curve, ca.to_affine_structs(curve, bases, inf), sc)))
    db = ca.DeviceBases(curve, bases, inf)
    out.append(("handle", db.msm_bigint(sc)))
    db.precompute(table_bits)
    out.append(("table", db.msm_bigint(sc)))
    db.free()
    return out


def assert_all(results, want, what):
    for name, got in results:
        assert (got == want).all(), (what, name)


# ============================================ constructions, on the CPU ============================================
def test_constructed_points_have_their_orders():
    a, orders = pts()
    off = U.off_subgroup_points()
    assert off["S"][0] == (0, 2) and not a["S"][:6].any() and a["S"][6:].any()
    assert off["-S"][0] == M.g1_neg((0, 2))
    for name, (p, o) in off.items():
        G, mul, on = (O.G2, M.g2_mul, M.g2_on_curve) if name in ("T2", "S2") else (O.G1, M.g1_mul, M.g1_on_curve)
        assert on(p) and G.on_curve(a[name]), name
        if o is None:
            # large order outside the subgroup: [r] T != O (oracle and model), [#E] T = O
            assert not G.to_affine(G.mul(a[name], O.int_to_limbs(U.R, 4)))[1], name
            assert mul(p, U.R) is not None and mul(p, (U.H1 if G is O.G1 else U.H2) * U.R) is None, name
        else:
            assert mul(p, o) is None and all(mul(p, k) is not None for k in range(1, o)), name
            assert G.to_affine(G.mul(a[name], O.int_to_limbs(o, 4)))[1], name
            assert not G.to_affine(G.mul(a[name], O.int_to_limbs(o - 1, 4)))[1], name
    assert orders["S2"] == 13 == U.small_primes_dividing(U.H2)[0] and 11 in U.small_primes_dividing(U.H1)
    # 2 S = -S, and phi(S) = (beta * 0, 2) = S: the GLV scaling maps S to ((k1 + k2) mod 3) S
    assert M.g1_mul(off["S"][0], 2) == off["-S"][0]
    # (0, +-sqrt(4 (1 + u))) does not exist in Fp2: the G2 cofactor has no factor 3
    assert U.fp2_sqrt(M.B_TWIST) is None and U.H2 % 3 != 0


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_oracle_msm_on_off_subgroup_bases_equals_the_model(gname):
    """the yardstick itself: the oracle's Pippenger on the constructed points = the big-integer model's plain sum of products"""
    _, G = group(gname)
    off = U.off_subgroup_points()
    names = ["S", "-S", "T", "S11", "S", "S"] if gname == "G1" else ["T2", "S2", "S2", "T2"]
    F = M._FpOps if gname == "G1" else M._Fp2Ops
    enc = U.g1_abi if gname == "G1" else U.g2_abi
    mpts = [off[k][0] for k in names]
    bases = np.stack([enc(p)[0] for p in mpts])
    for seed in range(3):
        sc = O.rand_scalars(700 + seed, len(bases))
        if seed == 2:
            sc[:] = sc[0]
        want = M.naive_msm(F, mpts, [O.limbs_to_int(s) for s in sc])
        assert U.jac_to_model(G, G.msm(bases, sc)) == want, seed


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_bulk_bases_closed_form_on_cpu(gname):
    _, G = group(gname)
    bases, k0, d, e, T, ell = bulk(gname, 300, 41)
    assert all(G.on_curve(b) for b in bases) and len(set(e.tolist())) == ell
    sc = O.rand_scalars(42, 300)
    assert (normalised(G, G.msm(bases, sc, threads=8)) == closed_form(G, sc, k0, d, e, T, ell)).all()


def test_oracle_miller_loop_and_prepare_on_off_subgroup_points_equal_the_model():
    off = U.off_subgroup_points()
    a, _ = pts()
    g1, g2 = O.G1.generator(), O.G2.generator()
    mg1 = (U.fp_int(g1[:6]), U.fp_int(g1[6:]))
    mg2 = ((U.fp_int(g2[:6]), U.fp_int(g2[6:12])), (U.fp_int(g2[12:18]), U.fp_int(g2[18:])))
    flat = lambda f: [x for f6 in f for f2 in f6 for x in f2]
    f = O.multi_miller_loop(a["S"].reshape(1, 12), g2.reshape(1, 24))
    assert U.f12_ints(f) == flat(M.multi_miller_loop([off["S"][0]], [mg2]))
    assert not (f == O.fp12_one()).all()                     # px = 0 alone is not the neutral line
    f = O.multi_miller_loop(g1.reshape(1, 12), a["T2"].reshape(1, 24))
    assert U.f12_ints(f) == flat(M.multi_miller_loop([mg1], [off["T2"][0]]))
    co = O.g2_prepare(a["T2"]).reshape(68, 3, 12)
    mco = M.g2_prepare(off["T2"][0])
    assert len(mco) == 68
    for s in range(68):
        for c in range(3):
            assert [U.fp_int(co[s, c, :6]), U.fp_int(co[s, c, 6:])] == list(mco[s][c]), (s, c)


def killing_scalars(rng, count, kill=True):
    """scalars m < r whose GLV split (k1, k2) is non-zero and has k1 + k2 = 0 mod 3 (kill) / != 0 mod 3"""
    out = []
    while len(out) < count:
        m = int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) % U.R
        k1, k2 = U.glv_split(m)
        if (k1 or k2) and ((k1 + k2) % 3 == 0) == kill:
            out.append(m)
    return out


def test_glv_split_of_the_chosen_scalars_is_the_hosts():
    """the Python split used to choose the scalars of the scaled Miller-loop tests is the library's (dgpu_selftest_glv_decompose)"""
    from crypto_amd._native import dev_lib
    rng = np.random.default_rng(5)
    for kill in (True, False):
        for m in killing_scalars(rng, 20, kill):
            k1, k2 = U.glv_split(m)
            assert (k1 + k2 * U.GLV_LAMBDA - m) % U.R == 0 and ((k1 + k2) % 3 == 0) == kill
            a = O.int_to_limbs(m, 4); h1 = np.zeros(2, np.uint64); h2 = np.zeros(2, np.uint64)
            assert dev_lib().dgpu_selftest_glv_decompose(a.ctypes.data_as(C.c_void_p), h1.ctypes.data_as(C.c_void_p), h2.ctypes.data_as(C.c_void_p)) == 0
            assert (O.limbs_to_int(h1), O.limbs_to_int(h2)) == (k1, k2)


# ============================================ MSM ============================================
@pytest.fixture
def dev():
    import torch
    import crypto_amd as ca
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)


@gpu
@pytest.mark.parametrize("gname,n", [("G1", 1), ("G1", 2), ("G1", 3), ("G1", 64), ("G1", 600), ("G1", 8191), ("G1", 8192), ("G1", 8193), ("G1", (1 << 16) + 3),
                                     ("G2", 1), ("G2", 2), ("G2", 3), ("G2", 64), ("G2", 600), ("G2", 4096)])
def test_msm_on_off_subgroup_bases_equals_the_oracle(gname, n, dev):
    """both sides of the tree <-> bucket switch, every entry point, against the oracle word for word"""
    _, G = group(gname)
    bases, inf = mixed(gname, n, 100 + n)
    sc = O.rand_scalars(200 + n, n)
    want = normalised(G, G.msm(bases, sc, inf, threads=16))
    assert_all(every_path(gname, bases, sc, inf, 16 if gname == "G1" else 0), want, n)


@gpu
@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_msm_on_off_subgroup_bases_2p17_closed_form(gname, dev):
    import crypto_amd as ca
    curve, G = group(gname)
    n = 1 << 17
    bases, k0, d, e, T, ell = bulk(gname, n, 300)
    sc = O.rand_scalars(301, n)
    want = closed_form(G, sc, k0, d, e, T, ell)
    assert (ca.msm_bigint(curve, bases, sc) == want).all()
    db = ca.DeviceBases(curve, bases)
    assert (db.msm_bigint(sc) == want).all()
    off = 1000
    # &bases[off..]: the closed form with the first `off` scalars zero
    assert (db.msm_bigint(sc[:n - off], offset=off) == closed_form(G, np.concatenate([np.zeros((off, 4), np.uint64), sc[:n - off]]), k0, d, e, T, ell)).all()
    db.precompute(20 if gname == "G1" else 0)
    assert (db.msm_bigint(sc) == want).all()
    db.free()


@gpu
@pytest.mark.parametrize("c", [7, 10, 13, 16])
def test_any_window_width_on_off_subgroup_bases(c, twin, dev):
    """every window width and chunk length of the bucket pipeline (as test_gpu_msm.test_any_window_width_same_point) on off-subgroup bases"""
    import crypto_amd as ca
    from crypto_amd._native import lib
    G = O.G1
    bases, inf = mixed("G1", 9001, 31)
    sc = O.rand_scalars(32, 9001)
    refs = {n: normalised(G, G.msm(bases[:n], sc[:n], inf[:n], threads=16)) for n in (5000, 9001)}
    lib().dgpu_set_window_bits(c)
    try:
        for ch in (16, 128):
            assert lib().dgpu_set_chunk(ch) == 0
            assert (ca.msm_bigint(ca.G1, bases, sc, inf) == refs[9001]).all(), ch
            with U.bucket_pipeline():
                assert (ca.msm_bigint(ca.G1, bases[:5000], sc[:5000], inf[:5000]) == refs[5000]).all(), ch
    finally:
        lib().dgpu_set_window_bits(0)
        lib().dgpu_set_chunk(0)


@gpu
@pytest.mark.parametrize("gname,n", [("G1", 5000), ("G1", 40000), ("G2", 5000)])
def test_cache_on_an_off_subgroup_key(gname, n, dev):
    """the drop-in path does no subgroup test: first call one-shot, second fills, third hits, then sub-slices of the resident entry"""
    import crypto_amd as ca
    curve, G = group(gname)
    bases, inf = mixed(gname, n, 400 + n)
    st = ca.to_affine_structs(curve, bases, inf)
    ca.bases_cache_clear()
    ca.bases_cache(min_n=1 << 12, verify=24)
    try:
        s0 = ca.bases_cache_stats()
        for call in range(3):
            sc = O.rand_scalars(500 + call, n)
            assert (ca.msm_strided(curve, st, sc) == normalised(G, G.msm(bases, sc, inf, threads=16))).all(), call
        s1 = ca.bases_cache_stats()
        # (the second call counts as a hit that fills the entry, the third as a hit on it)
        assert s1["misses"] - s0["misses"] == 1 and s1["fills"] - s0["fills"] == 1 and s1["hits"] - s0["hits"] == 2, (s0, s1)
        for lo, hi in ((1, n), (7, n - 500)):
            got = ca.msm_strided(curve, st[lo:hi], sc)
            assert (got == normalised(G, G.msm(bases[lo:hi], sc[:hi - lo], inf[lo:hi], threads=16))).all(), (lo, hi)
        assert ca.bases_cache_stats()["hits"] - s1["hits"] == 2
    finally:
        ca.bases_cache_clear()
        ca.bases_cache(min_n=1 << 16, verify=ca.CACHE_VERIFY_FULL)


def cancelling(gname, n, seed, m):
    """bases B_i = G_i + e_i T (i < n - 1) and B_{n-1} = G; scalars with (sum s_i e_i) mod ell = m and the subgroup part cancelled:
    the MSM is exactly m T"""
    _, G = group(gname)
    bases, k0, d, e, T, ell = bulk(gname, n, seed)
    bases[n - 1] = G.generator(); e[n - 1] = 0
    sv = [O.limbs_to_int(x) for x in O.rand_scalars(seed + 1, n)]
    sv[n - 1] = 0
    if n > 1:
        j = next((i for i in range(n - 1) if e[i]), None)
        if j is None:
            j = 0; e[0] = 1; bases[0] = U.plus_multiples(G, bases[:1], np.ones(1, int), T)[0]
        et = sum(s * int(x) for s, x in zip(sv, e)) % ell
        sv[j] += (m - et) * pow(int(e[j]), -1, ell) % ell
        assert sum(s * int(x) for s, x in zip(sv, e)) % ell == m
        sv[n - 1] = -sum(s * (k0 + i * d) for i, s in enumerate(sv[:n - 1])) % U.R
    return bases, np.stack([O.int_to_limbs(s, 4) for s in sv]), T, ell, (k0, d, e)


@gpu
@pytest.mark.parametrize("gname,n", [("G1", 3), ("G1", 600), ("G1", 8193), ("G1", (1 << 16) + 3), ("G2", 3), ("G2", 600), ("G2", 8193)])
def test_msm_results_that_cancel(gname, n, dev):
    """the subgroup part cancels: the result is exactly T, -T (T = S, S2); both cancel: the identity (Z = 0 and the oracle's flag); the T part
    cancels: a point of the subgroup equal to the closed form"""
    _, G = group(gname)
    for m in (1, -1, 0):
        bases, sc, T, ell, _ = cancelling(gname, n, 600 + n, m % 3 if gname == "G1" else m % 13)
        want_aff = T if m == 1 else (U.g1_abi(M.g1_neg(U.off_subgroup_points()["S"][0]))[0] if gname == "G1" else U.g2_abi(M.g2_neg(U.off_subgroup_points()["S2"][0]))[0])
        want = normalised(G, G.msm(bases[:0], sc[:0])) if m == 0 else affine_abi(G, want_aff)
        if n <= 1 << 16:
            assert (normalised(G, G.msm(bases, sc, threads=16)) == want).all(), m
        res = every_path(gname, bases, sc, None, 16 if gname == "G1" else 0)
        assert_all(res, want, (n, m))
        if m == 0:
            assert all(G.to_affine(r)[1] and not r[G.AW:].any() for _, r in res)
        else:
            assert all((r[:G.AW] == want_aff).all() for _, r in res)
    # the T part cancels, the subgroup part does not
    bases, k0, d, e, T, ell = bulk(gname, n, 700 + n)
    sv = [O.limbs_to_int(x) for x in O.rand_scalars(701 + n, n)]
    j = next(i for i in range(n) if e[i])
    sv[j] += -sum(s * int(x) for s, x in zip(sv, e)) * pow(int(e[j]), -1, ell) % ell
    if sv[j] >= U.R:
        sv[j] -= ell
    assert sum(s * int(x) for s, x in zip(sv, e)) % ell == 0
    sc = np.stack([O.int_to_limbs(s, 4) for s in sv])
    want = closed_form(G, sc, k0, d, e, T, ell)
    assert_all(every_path(gname, bases, sc, None, 16 if gname == "G1" else 0), want, (n, "T part"))


@gpu
@pytest.mark.parametrize("gname,n", [("G1", 3), ("G1", 600), ("G1", 8193), ("G1", 70000), ("G2", 600), ("G2", 8193)])
def test_msm_with_every_base_of_small_order(gname, n, dev):
    """every base S (S2), then S and -S alternating: the special cases of the bucket additions in nearly every bucket of every window"""
    _, G = group(gname)
    a, orders = pts()
    T = a["S" if gname == "G1" else "S2"]
    ell = orders["S" if gname == "G1" else "S2"]
    Tn = U.g1_abi(M.g1_neg(U.off_subgroup_points()["S"][0]))[0] if gname == "G1" else U.g2_abi(M.g2_neg(U.off_subgroup_points()["S2"][0]))[0]
    sc = O.rand_scalars(800 + n, n)
    sv = [O.limbs_to_int(x) for x in sc]
    for alt in (False, True):
        bases = np.stack([T] * n)
        if alt:
            bases[1::2] = Tn
        m = sum(s if (i % 2 == 0 or not alt) else -s for i, s in enumerate(sv)) % ell
        want = normalised(G, G.mul(T, O.int_to_limbs(m, 4)))
        if n <= 8193:
            assert (normalised(G, G.msm(bases, sc, threads=16)) == want).all()
        assert_all(every_path(gname, bases, sc, None, 16 if gname == "G1" else 0), want, (n, alt))


# ============================================ Miller loop ============================================
def miller_operands(n, seed, p_off=True, q_off=False):
    """subgroup pairs with S, -S, T, S11 planted as P (p_off) and T2 as Q (q_off)"""
    a, _ = pts()
    ps = O.G1.gen_seq(O.rand_scalars(seed, 1)[0], O.rand_scalars(seed + 1, 1)[0], n, threads=16)
    qs = O.G2.gen_seq(O.rand_scalars(seed + 2, 1)[0], O.rand_scalars(seed + 3, 1)[0], n, threads=16)
    if p_off:
        for j, name in enumerate(["S", "-S", "T", "S11", "S"]):
            ps[(5 * j) % n] = a[name]
    if q_off:
        for j in range(3):
            qs[(3 + 11 * j) % n] = a["T2"]
    return ps, qs


@gpu
@pytest.mark.parametrize("n", [1, 3, 70, 1024])
@pytest.mark.parametrize("side", ["P", "Q", "both"])
def test_miller_loop_off_subgroup_every_entry_point(n, side, dev):
    """raw Fp12 limb for limb against the oracle: affine, prepared, mixed affine / prepared, segmented"""
    import crypto_amd as ca
    from crypto_amd import pairing
    ps, qs = miller_operands(n, 40 + n, side != "Q", side != "P")
    if n >= 70:
        ps[60] = 0                                          # an identity member beside them
    skip = np.array([0 if p.any() else 1 for p in ps], np.uint8)
    ref = O.multi_miller_loop(ps, qs, skip, threads=16)
    if n == 1 and side == "P":
        assert not (ref == O.fp12_one()).all()             # P = S: not the neutral line
    assert (ca.multi_miller_loop(ps, qs) == ref).all()
    pc = pairing.G2Prepared.from_affine(qs)
    for i in range(min(n, 20)):
        assert (pc.coeffs[i] == O.g2_prepare(qs[i]).reshape(-1)).all(), i     # T2's coefficients too
    assert (pairing.multi_miller_loop(ps, pc) == ref).all()
    cut = max(1, n // 3)
    if n > 1:
        assert (pairing.multi_miller_loop(ps, [qs[:cut], pc[cut:]]) == ref).all()
        assert (pairing.multi_miller_loop(ps, [pc[:cut], qs[cut:]]) == ref).all()
    segs = pairing.multi_miller_loops([(ps[:cut], qs[:cut]), (ps[cut:], qs[cut:])])
    assert (segs[0] == O.multi_miller_loop(ps[:cut], qs[:cut], skip[:cut], threads=16)).all()
    assert (segs[1] == (O.multi_miller_loop(ps[cut:], qs[cut:], skip[cut:], threads=16) if n > cut else O.fp12_one())).all()


@gpu
@pytest.mark.parametrize("n", [1, 3, 130, 1024, 9000])
def test_every_form_of_the_miller_kernels_off_subgroup(n, twin, dev):
    """all 32 kernel forms of dgpu_set_miller_pipeline (as test_gpu_pairing.test_every_form_of_the_miller_kernels_gives_the_same_value) give
    one value on off-subgroup P and Q, the oracle's"""
    import crypto_amd as ca
    from crypto_amd import pairing
    from crypto_amd._native import lib
    ps, qs = miller_operands(n, 90 + n, True, n > 1)
    got = {}
    try:
        for mode in range(32):
            assert lib().dgpu_set_miller_pipeline(mode) == 0
            got[mode] = ca.multi_miller_loop(ps, qs)
            if 3 <= n <= 1100 and mode in (0, 3, 31):
                pc = pairing.G2Prepared.from_affine(qs)
                assert (pairing.multi_miller_loop(ps, [qs[:n // 3], pc[n // 3:]]) == got[mode]).all(), mode
    finally:
        lib().dgpu_set_miller_pipeline(31)
    for mode in range(1, 32):
        assert (got[mode] == got[0]).all(), mode
    if n <= 1100:
        assert (got[31] == O.multi_miller_loop(ps, qs, threads=16)).all()


# ============================================ the scaled Miller loop's device-side identity ============================================
def scaled_case(n, n_prep, seed, shared=False):
    """P_i: subgroup points, a fifth of them +-S.  Scalars: for the S rows a non-zero GLV split with k1 + k2 = 0 mod 3 (the scaled point is the
    identity only on the device) or != 0 mod 3 (it is +-S); random for the rest.  Returns the arguments and the pairs they mean:
    (P, sc, Q, skip, Pp, Qp, eff, eff_skip) with eff_i = ((k1 + k2) mod 3) P_i for the S rows, [m_i] P_i for the others"""
    a, _ = pts()
    rng = np.random.default_rng(seed)
    P = O.G1.gen_seq(O.rand_scalars(seed, 1)[0], O.rand_scalars(seed + 1, 1)[0], n + n_prep, threads=16)
    Q = O.G2.gen_seq(O.rand_scalars(seed + 2, 1)[0], O.rand_scalars(seed + 3, 1)[0], n + n_prep, threads=16)
    srow = np.zeros(n, bool)
    srow[rng.integers(0, 5, n) == 0] = True
    srow[0] = True
    for i in np.nonzero(srow)[0]:
        P[i] = a["S"] if rng.integers(0, 2) else a["-S"]
    if shared:
        sv = killing_scalars(rng, 1, True) * n
    else:
        sv = [O.limbs_to_int(x) for x in O.rand_scalars(seed + 4, n)]
        kill = srow & (rng.integers(0, 3, n) != 0)
        kill[0] = True
        if n >= 3:
            kill[1] = False; srow[1] = True; P[1] = a["S"]        # an S row that stays +-S
        for i in np.nonzero(srow)[0]:
            sv[i] = killing_scalars(rng, 1, bool(kill[i]))[0]
    sc = np.stack([O.int_to_limbs(s, 4) for s in sv])
    skip = np.zeros(n, np.uint8)
    if n >= 70:
        skip[rng.integers(0, 9, n) == 0] = 1
        skip[:2] = 0
    # what the pairs mean: the oracle's double-and-add for the subgroup rows, ((k1 + k2) mod 3) P for the S rows
    eff, einf = O.g1_scale_batch(P[:n], sc, threads=16)
    for i in np.nonzero(srow)[0]:
        k1, k2 = U.glv_split(sv[i])
        j = (k1 + k2) % 3
        if j == 0:
            eff[i] = 0; einf[i] = 1
        else:
            eff[i], inf = O.G1.to_affine(O.G1.mul(P[i], O.int_to_limbs(j, 4)))
            einf[i] = 0
            assert not inf
    return P[:n], sc, Q[:n], skip, P[n:], Q[n:], eff, einf, srow


@gpu
@pytest.mark.parametrize("n,n_prep", [(1, 0), (3, 0), (3, 2), (70, 0), (70, 2), (1024, 0), (1024, 2), (9000, 0), (9000, 1)])
def test_scaled_miller_loop_pair_killed_on_the_device(n, n_prep, dev):
    """pipelined form (n <= 8192: k_line_products3 for small launches, k_line_products for n = 1024) and two-call form (n = 9000): equal to the
    Miller loop over the pairs the scalings mean, with the killed pairs skipped, and to the oracle on them; dgpu_g1_scale_batch flags the killed rows"""
    import crypto_amd as ca
    from crypto_amd import pairing
    from crypto_amd import pairing_check as pc
    P, sc, Q, skip, Pp, Qp, eff, einf, srow = scaled_case(n, n_prep, 1000 + n + n_prep)
    # the scaling alone: killed rows are the identity (zero words, flag), the other S rows +-S exactly, the rest [m] P
    out, oinf = pc.g1_scale_each(P, sc)
    bad = np.nonzero((out != eff).any(axis=1) | (oinf != einf))[0]
    assert not len(bad), [(int(i), "S row" if srow[i] else "subgroup row", int(einf[i]), int(oinf[i])) for i in bad[:8]]
    assert not out[einf == 1].any()
    prep = pairing.G2Prepared.from_affine(Qp) if n_prep else None
    got = pairing.multi_miller_loop_scaled(P, sc, Q, skip, Pp if n_prep else None, prep)
    esk = skip | einf
    if n_prep:
        osk = np.concatenate([esk, np.zeros(n_prep, np.uint8)])
        dev_want = pairing.multi_miller_loop(np.concatenate([eff, Pp]), [Q, prep], osk)
        o_want = O.multi_miller_loop(np.concatenate([eff, Pp]), np.concatenate([Q, Qp]), osk, threads=16)
    else:
        dev_want = ca.multi_miller_loop(eff, Q, esk)
        o_want = O.multi_miller_loop(eff, Q, esk, threads=16)
    assert (got == dev_want).all()
    assert (got == o_want).all()
    if n == 1 and not n_prep:
        assert (got == O.fp12_one()).all()                 # the one pair is killed: the neutral value


@gpu
@pytest.mark.parametrize("n", [1, 3, 70, 9000])
def test_scaled_miller_loop_shared_killing_scalar(n, dev):
    """scalar_stride = 0: one scalar for every pair, killing every S row and scaling the others"""
    import crypto_amd as ca
    from crypto_amd import pairing
    P, sc, Q, skip, _, _, eff, einf, srow = scaled_case(n, 0, 2000 + n, shared=True)
    assert einf[srow].all() and not einf[~srow].any()
    got = pairing.multi_miller_loop_scaled(P, sc[0], Q, skip)
    assert (got == ca.multi_miller_loop(eff, Q, skip | einf)).all()
    assert (got == O.multi_miller_loop(eff, Q, skip | einf, threads=16)).all()


@gpu
@pytest.mark.parametrize("n,n_prep", [(3, 0), (70, 2), (1024, 0), (1024, 2)])
def test_scaled_miller_loop_pair_killed_in_every_product_kernel(n, n_prep, twin, dev):
    """the pipelined form with each product kernel: k_line_products3 (dgpu_set_miller_pipeline bit 4, the default while the launch is small)
    and k_line_products (bit 4 off; the default for launches that fill the chip) both treat the device-side identity as the neutral line"""
    from crypto_amd import pairing
    from crypto_amd._native import lib
    P, sc, Q, skip, Pp, Qp, eff, einf, srow = scaled_case(n, n_prep, 3000 + n + n_prep)
    prep = pairing.G2Prepared.from_affine(Qp) if n_prep else None
    osk = np.concatenate([skip | einf, np.zeros(n_prep, np.uint8)])
    want = O.multi_miller_loop(np.concatenate([eff, Pp]), np.concatenate([Q, Qp]), osk, threads=16)
    try:
        for mode in (31, 15):
            assert lib().dgpu_set_miller_pipeline(mode) == 0
            got = pairing.multi_miller_loop_scaled(P, sc, Q, skip, Pp if n_prep else None, prep)
            assert (got == want).all(), mode
    finally:
        lib().dgpu_set_miller_pipeline(31)
