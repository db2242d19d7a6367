"""GPU: LegoGroth16 key generation from a resident circuit (dgpu_qap_instance_map, dgpu_legogroth16_setup) against the Python mirror
(legogroth16.instance_map_with_evaluation / generate_parameters, which tests/test_gpu_legogroth16.py::test_generator_matches_oracle_setup ties to the
oracle): the instance map word for word on short, power-of-two and long-column circuits, the whole key word for word, the key proving and verifying,
the 2^20 domain, the refusals, and two host threads generating keys at once."""
import threading
import numpy as np
import pytest
import torch
import oracle_c as O
import lego_setup as LS
import crypto_amd as ca
from crypto_amd import legogroth16 as LG, qap, fixed_base as FB
from bigcase import big_circuit, ints_to_limbs

pytestmark = pytest.mark.gpu
R = LS.R


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)


def limbs(vals):
    return ints_to_limbs([v % R for v in vals])


def upload(cs, montgomery=False):
    mats = [qap.csr(cs[k]) for k in "ABC"]
    if montgomery:
        mats = [(rp, cl, O.fr_to_mont(vl) if len(vl) else vl) for rp, cl, vl in mats]
    return qap.DeviceR1cs(*mats, cs["n_inst"] + cs["n_wit"], cs["n_inst"], len(cs["A"]), montgomery=montgomery)


def check_instance_map(cs, t, montgomery=False):
    dr = upload(cs, montgomery)
    try:
        a, b, c, zt, V, D = LG.instance_map_with_evaluation(cs["A"], cs["B"], cs["C"], cs["n_inst"], cs["n_wit"], t)
        ga, gb, gc, gzt, gV, gD = dr.instance_map(t)
        assert (gD, gV) == (D, V)
        assert (ga == limbs(a)).all() and (gb == limbs(b)).all() and (gc == limbs(c)).all()
        assert (gzt == limbs([zt])[0]).all()
        # the &[Fr] form: t in and a, b, c, zt out as Montgomery limbs
        ma, mb, mc, mzt, _, _ = dr.instance_map(O.fr_to_mont(limbs([t]))[0], montgomery=True)
        assert (ma == O.fr_to_mont(limbs(a))).all() and (mc == O.fr_to_mont(limbs(c))).all() and (mzt == O.fr_to_mont(limbs([zt]))[0]).all()
    finally:
        dr.free()


def rnd_of(seed):
    rng = np.random.default_rng(seed)
    return lambda: int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1


@pytest.mark.parametrize("m", [1, 20, 200, (1 << 12) - 3])
@pytest.mark.parametrize("montgomery", [False, True])
def test_instance_map_matches_the_mirror(m, montgomery):
    check_instance_map(LS.circuit(m, x0=3), rnd_of(m)(), montgomery)


def test_instance_map_domain_exactly_a_power_of_two():
    cs = LS.circuit(29, x0=4)                 # 30 constraints + 2 inputs = 32
    assert len(cs["A"]) + cs["n_inst"] == 32
    check_instance_map(cs, rnd_of(32)())


def long_column_circuit(rows):
    """one witness variable (index 2) in every row of A and B, variable 0 in every row of C: three columns of `rows` entries each"""
    A, B, C = [], [], []
    for i in range(rows):
        A.append([(i + 1, 2), (1, 3 + i)]); B.append([((R - i) % R, 2)]); C.append([(i * i + 5, 0), (1, 3 + i)])
    return {"A": A, "B": B, "C": C, "n_inst": 2, "n_wit": rows + 1, "n_cons": rows}


@pytest.mark.parametrize("rows", [100, 1 << 16])
def test_instance_map_long_columns(rows):
    check_instance_map(long_column_circuit(rows), rnd_of(rows)())


def waste_and_generators(seed):
    rnd = rnd_of(seed)
    w = [rnd() for _ in range(6)]
    k1, k2 = rnd(), rnd()
    g1 = O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(k1, 4)))[0]
    g2 = O.G2.to_affine(O.G2.mul(O.G2.generator(), O.int_to_limbs(k2, 4)))[0]
    return w, g1, g2


def host_key(cs, cw, w, g1, g2):
    return LG.generate_parameters(cs["A"], cs["B"], cs["C"], cs["n_inst"], cs["n_wit"], cw, *w, g1, g2)[0]


def key_words(pk):
    vk = pk.vk
    return [vk.alpha_g1, vk.beta_g2, vk.gamma_g2, vk.delta_g2, vk.gamma_abc_g1, vk.eta_gamma_inv_g1, pk.beta_g1, pk.delta_g1, pk.eta_delta_inv_g1, pk.a0, pk.b1_0, pk.b2_0]


def free_key(pk):
    for q in (pk.a_query, pk.b_g1_query, pk.b_g2_query, pk.h_query, pk.l_query):
        q.free()


@pytest.mark.parametrize("m,cw", [(20, 2), (200, 0), ((1 << 14) - 5, 3)])
def test_full_key_matches_generate_parameters(m, cw):
    cs = LS.circuit(m, x0=9)
    w, g1, g2 = waste_and_generators(500 + m)
    ref = host_key(cs, cw, w, g1, g2)
    dr = upload(cs)
    pk, n_inst = LG.generate_parameters_r1cs(dr, cw, *w, g1, g2, queries_to_host=True)
    assert n_inst == cs["n_inst"] and pk.vk.commit_witness_count == cw
    for x, y in zip(key_words(pk), key_words(ref)):
        assert (np.asarray(x) == np.asarray(y)).all()
    # the five queries word for word (host copies of the same products the Python key's handles were made from)
    a, b, c, zt, V, D = LG.instance_map_with_evaluation(cs["A"], cs["B"], cs["C"], cs["n_inst"], cs["n_wit"], w[5])
    n = cs["n_inst"] + cw
    mix = [(w[1] * x + w[0] * y + z) % R for x, y, z in zip(a, b, c)]
    di = pow(w[3], R - 2, R)
    hq = [zt * di % R * pow(w[5], i, R) % R for i in range(D - 1)]
    scal = {"a_query": a, "b_g1_query": b, "b_g2_query": b, "h_query": hq, "l_query": [x * di % R for x in mix[n:]]}
    for name, (xy, inf) in pk.host_queries.items():
        tab = FB.WindowTable(ca.G2 if name == "b_g2_query" else ca.G1, g2 if name == "b_g2_query" else g1)
        want, want_inf = tab.multiply_many(scal[name]) if len(scal[name]) else (np.zeros_like(xy), np.zeros_like(inf))
        tab.free()
        assert (xy == want).all() and (inf == want_inf).all(), name
        # the resident handle holds the same points: a random-scalar MSM over both
        db, refq = getattr(pk, name), getattr(ref, name)
        assert db.n == refq.n == len(xy), name
        if db.n:
            rs = O.rand_scalars(31, db.n)
            curve = ca.G2 if name == "b_g2_query" else ca.G1
            assert (db.msm_bigint(rs) == ca.msm_bigint(curve, xy, rs, is_inf=inf)).all(), name
            assert (db.msm_bigint(rs) == refq.msm_bigint(rs)).all(), name
    free_key(pk); free_key(ref); dr.free()


@pytest.mark.parametrize("m,cw", [(20, 1), (300, 4)])
def test_generated_key_proves_and_verifies(m, cw):
    cs = LS.circuit(m, x0=13)
    w, g1, g2 = waste_and_generators(700 + m)
    dr = upload(cs)
    pk, n_inst = LG.generate_parameters_r1cs(dr, cw, *w, g1, g2)
    z = LS.scalars(cs["z"])
    pvk = LG.prepare_verifying_key(pk.vk)
    proof = LG.prove_abi(pk, 1234567, 7654321, 99999, z, n_inst, circuit=dr)
    assert LG.verify_proof(pvk, proof, z[1:n_inst])
    bad = z[1:n_inst].copy(); bad[0, 0] ^= 1
    assert not LG.verify_proof(pvk, proof, bad)                        # a flipped public input
    swapped = dict(proof); swapped["a"], swapped["c"] = proof["c"], proof["a"]
    assert not LG.verify_proof(pvk, swapped, z[1:n_inst])              # a swapped proof element
    free_key(pk); dr.free()


BADARG = -3          # DGPU_E_BADARG (include/dock_gpu.h)


def next_handle_id():
    """the id the library hands out next, observed by registering (and freeing) a one-scalar handle: ids are issued in order, so two of these with
    nothing registered in between differ by exactly one"""
    import ctypes as C
    L = ca._native.lib()
    one = np.zeros(4, np.uint64)
    h = C.c_uint64(0)
    assert L.dgpu_scalars_upload(one.ctypes.data_as(C.c_void_p), 1, 0, C.byref(h)) == 0
    assert L.dgpu_scalars_free(h.value) == 0
    return h.value


def test_refusals_leave_nothing_behind():
    L = ca._native.lib()
    cs = LS.circuit(50, x0=2)
    w, g1, g2 = waste_and_generators(9)
    dr = upload(cs)
    nw = cs["n_wit"]
    D = 64
    omega = pow(7, (R - 1) // D, R)
    bad = [
        ("cw > witnesses", dict(cw=nw + 1)),
        ("gamma = 0", dict(w=w[:2] + [0] + w[3:])),
        ("delta = 0", dict(w=w[:3] + [R] + w[4:])),        # (R = 0 mod r)
        ("t = 1", dict(w=w[:5] + [1])),
        ("t = omega^5", dict(w=w[:5] + [pow(omega, 5, R)])),
    ]
    free_key(LG.generate_parameters_r1cs(dr, 0, *w, g1, g2)[0])     # warm: the prover workspace exists before the counts are taken
    import ctypes as C
    assert L.dgpu_legogroth16_setup(0, 0, None, None, None, 0, None, None, None, None, 0, None, None, None) == BADARG
    h0 = next_handle_id()
    a0 = L.dgpu_device_alloc_count()
    for label, kw in bad:
        with pytest.raises((ca.DockGpuError, ValueError)) as e:
            LG.generate_parameters_r1cs(dr, kw.get("cw", 0), *kw.get("w", w), g1, g2)
        if isinstance(e.value, ca.DockGpuError):
            assert e.value.code == BADARG, label
    # the C call itself for the refusal the Python wrapper checks first, and the instance map's refusal of t in the domain
    h5, o1, o2, gabc = np.zeros(5, np.uint64), np.zeros(7 * 12, np.uint64), np.zeros(4 * 24, np.uint64), np.zeros(12 * 64, np.uint64)
    waste = np.concatenate([LG._sc(x) for x in w])
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert L.dgpu_legogroth16_setup(dr.handle, nw + 1, p(waste), p(np.ascontiguousarray(g1)), p(np.ascontiguousarray(g2)), 0, p(h5), p(o1), p(o2), p(gabc), 64, None, None, None) == BADARG
    for wv in ([w[0], w[1], 0, w[3], w[4], w[5]], [w[0], w[1], w[2], 0, w[4], w[5]], w[:5] + [1]):
        wz = np.concatenate([LG._sc(x) for x in wv])
        assert L.dgpu_legogroth16_setup(dr.handle, 0, p(wz), p(np.ascontiguousarray(g1)), p(np.ascontiguousarray(g2)), 0, p(h5), p(o1), p(o2), p(gabc), 64, None, None, None) == BADARG
    assert L.dgpu_legogroth16_setup(dr.handle, 0, p(waste), p(np.ascontiguousarray(g1)), p(np.ascontiguousarray(g2)), 0, p(h5), p(o1), p(o2), p(gabc), 1, None, None, None) == BADARG
    with pytest.raises(ca.DockGpuError):
        dr.instance_map(1)
    assert (h5 == 0).all()
    assert L.dgpu_device_alloc_count() == a0, "a refused call allocated"
    h1 = next_handle_id()
    assert h1 == h0 + 1, "a refused call registered a handle (ids %d -> %d)" % (h0, h1)
    a0 = L.dgpu_device_alloc_count()
    handle = dr.handle
    dr.free()
    assert L.dgpu_legogroth16_setup(handle, 0, p(waste), p(np.ascontiguousarray(g1)), p(np.ascontiguousarray(g2)), 0, p(h5), p(o1), p(o2), p(gabc), 64, None, None, None) == BADARG
    assert L.dgpu_qap_instance_map(handle, p(LG._sc(5)), 0, None, None, None, None, None) == BADARG
    assert L.dgpu_device_alloc_count() == a0


def test_two_threads_generate_keys_at_once():
    shapes = [LS.circuit(400, x0=21), LS.circuit(700, x0=22)]
    params = [waste_and_generators(40 + k) for k in range(2)]
    drs = [upload(cs) for cs in shapes]

    def gen(k):
        w, g1, g2 = params[k]
        pk, _ = LG.generate_parameters_r1cs(drs[k], 2, *w, g1, g2, queries_to_host=True)
        words = key_words(pk) + [x for q in pk.host_queries.values() for x in q]
        free_key(pk)
        return words
    serial = [gen(k) for k in range(2)]
    got = [None, None]

    def run(k):
        got[k] = gen(k)
    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(2):
        assert len(got[k]) == len(serial[k]) and all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(got[k], serial[k])), k
    for d in drs:
        d.free()


def test_full_size_2_20():
    """D = 2^20: the instance map word for word, A(t) B(t) - C(t) = h(t) Z(t) for the satisfying assignment with h from the witness map, and a proof
    made with the generated key verifies"""
    m, cw = (1 << 20) - 3, 2
    z, A, B, Cm, n_inst, nc = big_circuit(m, 7)
    zl = ints_to_limbs(z)
    w, g1, g2 = waste_and_generators(2021)
    t = w[5]
    dr = qap.DeviceR1cs(A, B, Cm, len(z), n_inst, nc)
    ga, gb, gc, gzt, V, D = dr.instance_map(t)
    assert D == 1 << 20 and V == len(z) - 1
    cs = LS.circuit(m, 7)
    a, b, c, zt, V2, D2 = LG.instance_map_with_evaluation(cs["A"], cs["B"], cs["C"], n_inst, len(z) - n_inst, t)
    del cs
    assert (V2, D2) == (V, D)
    assert (ga == limbs(a)).all() and (gb == limbs(b)).all() and (gc == limbs(c)).all() and (gzt == limbs([zt])[0]).all()
    # the QAP identity at t
    At = sum(x * y for x, y in zip(z, a)) % R
    Bt = sum(x * y for x, y in zip(z, b)) % R
    Ct = sum(x * y for x, y in zip(z, c)) % R
    h, _ = dr.witness_map(zl)
    ht = 0
    for coef in reversed([int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in h]):
        ht = (ht * t + coef) % R
    assert (At * Bt - Ct - ht * zt) % R == 0
    pk, _ = LG.generate_parameters_r1cs(dr, cw, *w, g1, g2)
    proof = LG.prove_abi(pk, 111, 222, 333, zl, n_inst, circuit=dr)
    assert LG.verify_proof(LG.prepare_verifying_key(pk.vk), proof, zl[1:n_inst])
    free_key(pk); dr.free()


def test_setup_takes_the_toxic_waste_as_fr_limbs():
    """montgomery = 1: the six scalars as ark-ff Fr limbs give the same key as their canonical form (montgomery = 0)"""
    import ctypes as C
    L = ca._native.lib()
    cs = LS.circuit(40, x0=6)
    w, g1, g2 = waste_and_generators(77)
    dr = upload(cs)
    n = cs["n_inst"] + 1
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    outs = []
    for mont in (0, 1):
        waste = limbs(w).reshape(-1)
        if mont:
            waste = O.fr_to_mont(limbs(w)).reshape(-1)
        h5, o1, o2, gabc = np.zeros(5, np.uint64), np.zeros(7 * 12, np.uint64), np.zeros(4 * 24, np.uint64), np.zeros(n * 12, np.uint64)
        D = C.c_size_t(0)
        assert L.dgpu_legogroth16_setup(dr.handle, 1, p(np.ascontiguousarray(waste)), p(np.ascontiguousarray(g1)), p(np.ascontiguousarray(g2)), mont,
                                        p(h5), p(o1), p(o2), p(gabc), n, None, None, C.byref(D)) == 0
        for hd in h5:
            assert L.dgpu_bases_free(int(hd)) == 0
        outs.append((o1, o2, gabc))
    for x, y in zip(*outs):
        assert (x == y).all()
    ref = host_key(cs, 1, w, g1, g2)
    assert (outs[0][0][:12] == ref.vk.alpha_g1).all() and (outs[0][1][24:48] == ref.vk.delta_g2).all()
    free_key(ref); dr.free()
