"""CPU: the integer model of the range-proof calls (tests/smc_model.py) against the reference's own properties, and crypto_amd.smc_range_proof's statement rules
against the model's: the sumset rules reproduce cls_range_proof/util.rs' sumsets_check for bases 2 .. 16, the randomness multiple and the u128 product b, honest
proofs of every statement the GPU tests use verify in the exponent, every single tamper gives its (status, detail), two Schnorr errors that cancel pass the batch
under rho = 1 and fail under rho = 2, and two pairing errors that cancel inside one proof pass the merged form under random = 1 and fail under 2."""
import numpy as np
import pytest
import smc_model as SM
from smc_model import CLS, CCS
from bbs_model import R
from crypto_amd import smc_range_proof as SRP

# (kind, base, min, max) of the GPU tests (tests/test_gpu_smc_range_proof.py)
STATEMENTS = [(CLS, 2, 0, 2 ** 64 - 1), (CLS, 3, 5, 13), (CLS, 3, 5, 12), (CLS, 4, 10, 11), (CLS, 16, 0, 65536), (CCS, 4, 10, 1000), (CCS, 2, 0, 2 ** 63)]


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def setup(seed=5):
    rng = np.random.default_rng(seed)
    return rng, SM.Key(*rand(rng, 4))


def a_proof(rng, key, st, value):
    b = rand(rng, 1 + st.sides * (1 + 3 * st.l) + 2)
    return SM.prove(key, st, value, b[-1], b[-2], lambda k: b[k])


@pytest.mark.parametrize("base", [2, 3, 4, 5, 8, 10, 11, 14, 16])
def test_sumsets_check(base):
    """util.rs sumsets_check: for ranges that are multiples of base - 1, 0, 1, range - 1, range and values between decompose into l digits < base whose
    weighted sum is the value; the library's rules give the same boundaries"""
    rng = np.random.default_rng(base)
    ranges = [int(rng.integers(1, 2 ** 63)) * 2 * (base - 1) for _ in range(12)] + [(2 ** 64 - 1) * (base - 1), base - 1, 3 * (base - 1)]
    for rg in ranges:
        l = SM.find_number_of_digits(rg, base)
        G = SM.find_sumset_boundaries(rg, base, l)
        assert base ** l >= rg + 1 and (l == 0 or base ** (l - 1) < rg + 1) and len(G) == l <= 64
        assert SRP.number_of_digits(rg, base) == l and SRP.sumset_boundaries(rg, base, l) == G
        for v in [0, 1, rg - 1, rg] + [int(rng.integers(0, 2 ** 62)) % (rg + 1) for _ in range(20)]:
            sigma = SM.decompose_for_sumset(v, G, base)
            assert len(sigma) == l and all(0 <= d < base for d in sigma) and sum(d * g for d, g in zip(sigma, G)) == v
            assert SRP.decompose_for_sumset(v, G, base) == sigma


def test_randomness_multiple_and_the_u128_product():
    assert SM.range_and_rm(3, 5, 12) == (14, 2) and SM.range_and_rm(3, 5, 11) == (6, 1)
    st = SM.Statement(CLS, 5, 13, 3)
    assert (st.rm, st.range, st.l) == (2, 14, 3) and st.consts == [(R - 2, 10, 2)]
    assert SM.Statement(CLS, 5, 12, 3).rm == 1
    st = SM.Statement(CLS, 10, 11, 4)
    assert (st.l, st.w, st.M, st.D) == (0, [], 1, 0)                       # max = min + 1: the one commitment equation and no pairing
    # min rm does not fit a u64: the reference multiplies in a u128
    lo = 2 ** 64 - 20
    st = SM.Statement(CLS, lo, 2 ** 64 - 1, 16)
    assert st.rm == 15 and st.consts[0][1] == lo * 15 and lo * 15 >= 2 ** 64
    assert SM.Statement(CLS, 0, 2 ** 64 - 1, 2).l == 64 and SM.Statement(CCS, 0, 2 ** 63, 2).l == 64
    for base in range(3, 65536, 977):                                     # rm > 1 only lengthens ranges of base >= 3: never past 64 digits
        assert SM.Statement(CLS, 0, 2 ** 64 - 1, base).l <= 41


@pytest.mark.parametrize("kind, base, lo, hi", STATEMENTS)
def test_the_library_derives_the_models_statement(kind, base, lo, hi):
    st = SM.Statement(kind, lo, hi, base)
    got = (SRP.cls_statement if kind == CLS else SRP.ccs_statement)(lo, hi, base, set_size=base)
    assert got == st.as_tuple()
    assert st.l <= 64 and all(0 <= v < R for t in st.consts for v in t)


def test_the_library_refuses_what_the_reference_refuses():
    for f in (SRP.cls_statement, SRP.ccs_statement):
        for lo, hi in ((5, 5), (6, 5)):
            with pytest.raises(ValueError, match="IncorrectBounds"):
                f(lo, hi, 4)
        with pytest.raises(ValueError, match="UnsupportedBase"):
            f(0, 100, 5, set_size=4)
        f(0, 100, 4, set_size=4)
        f(0, 100, 4, set_size=16)                                         # params that support a larger base are fine


@pytest.mark.parametrize("kind, base, lo, hi", STATEMENTS)
def test_honest_proofs_verify_and_every_tamper_gives_its_status(kind, base, lo, hi):
    rng, key = setup(base + hi % 1000)
    st = SM.Statement(kind, lo, hi, base)
    for value in sorted({lo, hi - 1, (lo + hi) // 2}):
        p = a_proof(rng, key, st, value)
        assert all(p.equations(key, st)) and not any(p.pairing_errors(key))
        assert p.status(key, st) == (0, 0) and p.status(key, st, random=7) == (0, 0)
        assert SM.batch_verdict(key, st, [p], 12345)
        for s in range(st.sides):
            assert SM.tamper(p, "D", s=s).status(key, st) == (1, s + 1)
        if not st.l:
            continue
        for d in sorted({0, st.l - 1, st.D - 1}):
            q = st.ref_position(d)
            assert SM.tamper(p, "A_identity", d).status(key, st) == (2, 4 * q + 1)
            assert SM.tamper(p, "z1", d).status(key, st) == (2, 4 * q + 2)
            t = SM.tamper(p, "shift", d)
            assert t.status(key, st) == (2, 4 * q + 3) and t.status(key, st, random=3) == (3, 0)
            both = SM.tamper(SM.tamper(p, "z1", d), "D", s=st.sides - 1)
            assert both.status(key, st) == (1, st.sides)                  # status 1 wins over a bad digit
            assert not SM.batch_verdict(key, st, [SM.tamper(p, "z1", d)], 12345) and not SM.batch_verdict(key, st, [t], 12345)
            assert not SM.batch_verdict(key, st, [SM.tamper(p, "A_identity", d)], 12345)


def test_another_keys_signature_fails_the_pairing_alone():
    rng, key = setup(9)
    st = SM.Statement(CCS, 10, 1000, 4)
    b = rand(rng, 1 + st.sides * (1 + 3 * st.l) + 2)
    p = SM.prove(key, st, 500, b[-1], b[-2], lambda k: b[k])
    f = SM.prove(key, st, 500, b[-1], b[-2], lambda k: b[k], other_key=True)
    assert all(f.equations(key, st)) and all(f.pairing_errors(key))
    assert SM.tamper(p, "forged", st.l, forged=f).status(key, st) == (2, 4 * 1 + 3)      # max[0] is second in the reference's order
    # two bad digits: max[0] (position 1) and min[1] (position 2) — the reference's first is reported
    two = SM.tamper(SM.tamper(p, "z1", st.l), "z1", 1)
    assert two.status(key, st) == (2, 4 * 1 + 2)
    two = SM.tamper(SM.tamper(p, "forged", st.l, forged=f), "z1", 1)
    assert two.status(key, st) == (2, 4 * 1 + 3)


def test_only_short_ccs_proofs_are_proof_shorter_than_expected():
    """arbitrary_range_cdh.rs:327-337: the reference's error is for CCS sides with fewer than l digits; longer arrays and CLS proofs are malformed calls"""
    z12 = lambda k: np.zeros((k, 12), np.uint64)
    z4 = lambda k: np.zeros((k, 4), np.uint64)
    ccs, cls = SRP.ccs_statement(10, 1000, 4), SRP.cls_statement(5, 13, 3)
    mk = lambda st, nd: SRP.Proofs(st, z12(2), z4(2), z12(2 * st[0]), z4(2 * st[0]), z12(3 * nd), z4(2 * nd))
    assert mk(ccs, 2 * 2 * ccs[1]).n == 2 and mk(cls, 2 * cls[1]).n == 2
    with pytest.raises(ValueError, match="^ProofShorterThanExpected"):
        mk(ccs, 2 * 2 * ccs[1] - 1)
    for st, nd in ((ccs, 2 * 2 * ccs[1] + 1), (cls, 2 * cls[1] - 1), (cls, 2 * cls[1] + 1)):
        with pytest.raises(ValueError, match="^the digit arrays"):
            mk(st, nd)


def test_challenge_contribution_writes_the_references_order():
    """range_proof_cdh.rs:258-272 / arbitrary_range_cdh.rs:291-309: per digit (all of min, then all of max) Abar, A', g1, T; then g, h, the commitment, D
    (D_min, D_max) — every point compressed by the library's encoder; the points are k G for distinct k, so a wrong order cannot give the same bytes"""
    import types
    import oracle_c as O
    from crypto_amd import serde, G1
    pts, inf = O.g1_scale_batch(np.tile(O.G1.generator(), (40, 1)), np.array([[k + 1, 0, 0, 0] for k in range(40)], np.uint64), threads=2)
    assert not inf.any()
    enc = lambda q: serde.serialize(G1, q.reshape(1, 12))
    params = types.SimpleNamespace(g1=pts[0], ck_g=pts[1], ck_h=pts[2])
    for stmt in (SRP.cls_statement(5, 13, 3), SRP.ccs_statement(10, 1000, 4), SRP.cls_statement(10, 11, 4)):
        S, l = stmt[0], stmt[1]
        C_, D, dig = pts[3], pts[4:4 + S], pts[6:6 + 3 * S * l].reshape(S * l, 3, 12)
        want = b"".join(enc(d[1]) + enc(d[0]) + enc(pts[0]) + enc(d[2]) for d in dig) + enc(pts[1]) + enc(pts[2]) + enc(C_) + b"".join(enc(q) for q in D)
        got = SRP.challenge_contribution(params, stmt, C_, D, dig)
        assert got == want and len(got) == 48 * (4 * S * l + 3 + S)


@pytest.mark.parametrize("kind, base, lo, hi", [(CLS, 3, 5, 13), (CCS, 4, 10, 1000)])
def test_cancelling_errors_pass_under_one_and_fail_under_two(kind, base, lo, hi):
    rng, key = setup(3)
    st = SM.Statement(kind, lo, hi, base)
    proofs = [a_proof(rng, key, st, lo + k % (hi - lo)) for k in range(5)]
    assert SM.batch_verdict(key, st, proofs, 1) and SM.batch_verdict(key, st, proofs, 2) and SM.batch_verdict(key, st, [], 2)
    # two Schnorr errors: T of one digit each in two proofs, + X and - X — every weight is one under rho = 1
    bad = [p.copy() for p in proofs]
    bad[1].digits[0].t = (bad[1].digits[0].t + 77) % R
    bad[3].digits[st.D - 1].t = (bad[3].digits[st.D - 1].t - 77) % R
    assert bad[1].status(key, st)[0] == 2 and bad[3].status(key, st)[0] == 2
    assert SM.batch_verdict(key, st, bad, 1) and not SM.batch_verdict(key, st, bad, 2)
    # two pairing errors inside one proof: Abar_a + delta g1, Abar_b - delta g1, the Schnorr checks consistent
    p = SM.tamper(SM.tamper(proofs[0], "shift", 0, delta=5), "shift", st.D - 1, delta=R - 5)
    assert p.status(key, st)[0] == 2 and p.status(key, st, random=1) == (0, 0) and p.status(key, st, random=2) == (3, 0)
    assert SM.batch_verdict(key, st, [p], 1) and not SM.batch_verdict(key, st, [p], 2)
