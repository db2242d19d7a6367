"""GPU: the batched GT chains (crypto_amd/csrc/gt_kernels.hip.h, k_gt.hip) through dgpu_final_exponentiation_batch and
dgpu_legogroth16_verify_each.
  - final_exponentiation_batch: word for word dgpu_final_exponentiation (host) of every element, at sizes around the lane-group, wave and
    chunk borders, zeros planted at the ends and borders flagged without touching their neighbours;
  - verify_each: one verdict per proof equal to the set of planted faults (wrong C, wrong public input, identity A / B / C, B_i <-> B_j) at the ends
    and around the chunk borders, Montgomery inputs alike, n single dgpu_legogroth16_verify calls alike, and a compensating pair that the batch
    check accepts at the batching scalar 1 rejected exactly at its two proofs; more public inputs than DGPU_MAX_LINCOMB; two threads at once."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd import legogroth16 as LG
from crypto_amd import pairing
from crypto_amd import fixed_base as FB
from crypto_amd._native import lib

pytestmark = pytest.mark.gpu
R, P = U.R, U.P
p_ = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)


def lim(vals):
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def ints(rng, k):
    return [int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1 for _ in range(k)]


def g1(k):
    return O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(k % R, 4)))[0]


def rand_f12(rng, n):
    """n random Fp12 elements as ABI words: every coefficient below p (its top word below p's)"""
    w = rng.integers(0, 2 ** 64, size=(n, 12, 6), dtype=np.uint64)
    w[:, :, 5] %= np.uint64(P >> 320)
    return w.reshape(n, 72)


def host_fe_all(fs):
    def one(f):
        out = np.zeros(72, np.uint64)
        rc = lib().dgpu_final_exponentiation(p_(np.ascontiguousarray(f)), p_(out))
        return rc, out
    with ThreadPoolExecutor(16) as ex:
        res = list(ex.map(one, fs))
    return np.stack([r[1] for r in res]), np.array([r[0] == -5 for r in res])


FE_SIZES = [1, 2, 5, 6, 7, 9, 10, 11, 63, 64, 65, 1000, 2047, 2048, 4095, 4096, 4097, 20479, 20480, 20481, 65536]


@pytest.mark.parametrize("n", FE_SIZES)
def test_final_exponentiation_batch_matches_host(n):
    rng = np.random.default_rng(100 + n)
    fs = rand_f12(rng, n)
    zeros = sorted({p for p in (0, 9, 10, 59, 60, 2047, 2048, 16383, 16384, n - 1) if p < n})
    fs[zeros] = 0
    got, gz = pairing.final_exponentiation_batch(fs)
    want, wz = host_fe_all(fs)
    assert (gz == wz).all() and set(np.nonzero(gz)[0]) == set(zeros)
    assert (got == want).all()
    assert not got[zeros].any()


_STMT = {}


def statement(n_pub, n_max=20000):
    """n_max valid proofs of one key with n_pub public inputs each, made on the device from known discrete logs"""
    if (n_pub, n_max) in _STMT:
        return _STMT[(n_pub, n_max)]
    rng = np.random.default_rng(9000 + n_pub)
    al, be, ga, de = ints(rng, 4)
    gab = ints(rng, n_pub + 1)
    av, bv, dv = ints(rng, n_max), ints(rng, n_max), ints(rng, n_max)
    xs = [ints(rng, n_pub) for _ in range(n_max)]
    dinv = pow(de, R - 2, R)
    sv = [(gab[0] + sum(x * g for x, g in zip(xr, gab[1:]))) % R for xr in xs]
    cv = [((a * b - al * be - (s + d) * ga) * dinv) % R for a, b, d, s in zip(av, bv, dv, sv)]
    with FB.WindowTable(ca.G2, O.G2.generator()) as t2, FB.WindowTable(ca.G1, O.G1.generator()) as t1:
        A, _ = t1.multiply_many(lim(av)); Cc, _ = t1.multiply_many(lim(cv)); D, _ = t1.multiply_many(lim(dv)); K, _ = t1.multiply_many(lim([al] + gab))
        B, _ = t2.multiply_many(lim(bv)); V, _ = t2.multiply_many(lim([be, ga, de]))
    vk = LG.VerifyingKey(K[0], V[0], V[1], V[2], K[1:], O.G1.generator(), 0)
    pubs = lim([x for xr in xs for x in xr]).reshape(n_max, n_pub, 4)
    st = dict(pvk=LG.prepare_verifying_key(vk), A=A, B=B, C=Cc, D=D, pubs=pubs, cv=cv)
    _STMT[(n_pub, n_max)] = st
    return st


def columns(st, n):
    return {k: np.ascontiguousarray(st[k][:n]).copy() for k in "ABCD"}, np.ascontiguousarray(st["pubs"][:n]).copy()


def each(st, cols, pubs, mont=False):
    return LG.verify_proofs_each_abi(st["pvk"], None, None, montgomery=mont, packed=(cols["A"], cols["B"], cols["C"], cols["D"], pubs))


def plant(st, cols, pubs, n, n_pub):
    """the faults at the ends and around the borders; returns the indices that must be rejected"""
    bad = set()
    pos = sorted({p for p in (0, 15, 16, 63, 64, 4095, 4096, n - 1) if p < n})
    kinds = ["C", "pub", "A0", "B0", "C0", "swapB"]
    for t, p in enumerate(pos):
        kind = kinds[(t + n) % len(kinds)]
        if kind == "pub" and not n_pub:
            kind = "C"
        if kind == "swapB" and n < 2:
            kind = "A0"
        if kind == "C":
            cols["C"][p] = g1(st["cv"][p] + 1)
        elif kind == "pub":
            pubs[p, 0] = lim([(O.limbs_to_int(pubs[p, 0]) + 1) % R])[0]
        elif kind in ("A0", "C0"):
            cols[kind[0]][p] = 0
        elif kind == "B0":
            cols["B"][p] = 0
        else:
            q = (p + 7) % n if (p + 7) % n != p else (p + 1) % n
            cols["B"][[p, q]] = cols["B"][[q, p]]
            bad.add(q)
        bad.add(p)
    return bad


EACH_CASES = [(n, k) for n in (1, 3, 64, 65, 1024, 4096, 4097, 20000) for k in (0, 1, 5)]


@pytest.mark.parametrize("n,n_pub", EACH_CASES)
def test_verify_each_verdicts_are_the_planted_faults(n, n_pub):
    st = statement(n_pub)
    cols, pubs = columns(st, n)
    assert each(st, cols, pubs).all()
    bad = plant(st, cols, pubs, n, n_pub)
    got = each(st, cols, pubs)
    assert set(np.nonzero(~got)[0]) == bad
    if n in (1024, 65):
        assert (each(st, cols, np.ascontiguousarray(O.fr_to_mont(pubs)), mont=True) == got).all()
    if n <= 300:
        proofs = [{k.lower(): cols[k][t] for k in "ABCD"} for t in range(n)]
        one = []
        for t in range(n):
            try:
                one.append(LG.verify_proof_abi(st["pvk"], proofs[t], pubs[t]))
            except ValueError:                                          # UnexpectedIdentity is a rejection
                one.append(False)
        assert (np.array(one) == got).all()


def test_compensating_pair_rejected_exactly_at_its_two_proofs():
    n, n_pub = 1024, 1
    st = statement(n_pub)
    cols, pubs = columns(st, n)
    e = 123456789
    i, j = 15, 64
    cols["C"][i] = g1(st["cv"][i] + e); cols["C"][j] = g1(st["cv"][j] - e)
    assert LG.verify_proofs_batch_abi(st["pvk"], None, None, 1, packed=(cols["A"], cols["B"], cols["C"], cols["D"], pubs))
    got = each(st, cols, pubs)
    assert set(np.nonzero(~got)[0]) == {i, j}


def test_more_public_inputs_than_the_one_call_verifier_takes():
    n, n_pub = 70, 20
    st = statement(n_pub, n_max=n)
    cols, pubs = columns(st, n)
    assert each(st, cols, pubs).all()
    bad = plant(st, cols, pubs, n, n_pub)
    assert set(np.nonzero(~each(st, cols, pubs))[0]) == bad


def test_two_threads():
    rng = np.random.default_rng(77)
    fs = rand_f12(rng, 3000)
    st = statement(1)
    cols, pubs = columns(st, 2000)
    bad = plant(st, cols, pubs, 2000, 1)
    serial_fe = pairing.final_exponentiation_batch(fs)[0]
    serial_ve = each(st, cols, pubs)
    with ThreadPoolExecutor(2) as ex:
        for _ in range(2):
            f1 = ex.submit(pairing.final_exponentiation_batch, fs)
            f2 = ex.submit(each, st, cols, pubs)
            assert (f1.result()[0] == serial_fe).all() and (f2.result() == serial_ve).all()
    assert set(np.nonzero(~serial_ve)[0]) == bad
