"""CPU: tests/saver_model.py (the big-integer model test_gpu_saver.py decides every expected byte with) against itself, against the oracle's Miller loop,
final exponentiation and GT power on a handful of rows, and compose / decompose against the vectors of the reference's own test (saver/src/utils.rs:113-201)."""
import numpy as np
import pytest
import oracle_c as O
import saver_model as M

R = M.R


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def key(K, b, seed=5):
    rng = np.random.default_rng(seed)
    d, h, rho = rand(rng, 3)
    return M.Key(rand(rng, K), d, h, rho, rand(rng, K), rand(rng, K + 1), rand(rng, K), b)


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def g1_times(scalars):
    out, inf = O.g1_scale_batch(np.tile(O.G1.generator(), (len(scalars), 1)), limbs([k % R for k in scalars]), threads=4)
    out[inf.astype(bool)] = 0
    return out


def g2_times(scalars):
    g = O.G2.generator()
    return np.stack([np.zeros(24, np.uint64) if k % R == 0 else O.G2.to_affine(O.G2.mul(g, O.int_to_limbs(k % R, 4)))[0] for k in scalars])


@pytest.mark.parametrize("value,b,tail", [(53, 4, [3, 5]), (53, 8, [53]), (53, 16, [53]), (325, 4, [1, 4, 5]), (325, 8, [1, 69]), (325, 16, [325]),
                                          (7986, 4, [1, 15, 3, 2]), (7986, 8, [31, 50]), (7986, 16, [7986]), (65831, 4, [0, 1, 0, 1, 2, 7]), (65831, 8, [1, 1, 39]),
                                          (65831, 16, [1, 295])])
def test_compose_and_decompose_on_the_references_vectors(value, b, tail):
    d = M.decompose(value, b)
    assert len(d) == 256 // b and d[-len(tail):] == tail and not any(d[:-len(tail)])
    assert M.compose(d, b) == value
    from crypto_amd.saver import compose
    assert compose(d, b) == value


def test_compose_reduces_and_refuses_other_bases():
    from crypto_amd.saver import compose
    for b in (4, 8, 16):
        top = [(1 << b) - 1] * (256 // b)
        assert M.compose(top, b) == compose(top, b) == (2 ** 256 - 1) % R
        assert M.compose(M.decompose(R - 1, b), b) == R - 1
    for b in (1, 5, 12, 17):
        with pytest.raises(ValueError, match="UnexpectedBase"):
            M.compose([0, 0], b)
        with pytest.raises(ValueError, match="UnexpectedBase"):
            compose([0, 0], b)


@pytest.mark.parametrize("K,b", [(1, 4), (3, 4), (2, 8), (2, 16)])
def test_a_ciphertext_decrypts_verifies_and_commits_in_the_exponent(K, b):
    k = key(K, b)
    rng = np.random.default_rng(K * 100 + b)
    for msgs in ([0] * K, [k.E] * K, [1] + [0] * (K - 1), [int(x) % (k.E + 1) for x in rng.integers(0, 1 << 16, K)]):
        row = k.encrypt(msgs, rand(rng, 1)[0])
        st, chunks, nu = k.decrypt(row)
        assert st == 0 and chunks == msgs
        assert k.decryption_verifies(row, chunks, nu) and k.commitment_verifies(row)
        assert not k.decryption_verifies(row, chunks, nu + 1)
        bad = list(chunks); bad[-1] = (bad[-1] + 1) % (k.E + 1)
        assert not k.decryption_verifies(row, bad, nu)
        # the GT form the device checks (e(c_j, V_2_j) e(-nu, V_1_j) = T_j[m_j]) is the reference's condition
        vals = k.pairing_values(row, second=R - nu)
        assert all(v == k.power(j, m) for j, (v, m) in enumerate(zip(vals, chunks)))
    # out of range: 2^b and r - 1 as "chunks"
    for m in (k.E + 1, R - 1):
        st, chunks, _ = k.decrypt(k.encrypt([m] + [0] * (K - 1), 7))
        assert st == 1 and chunks == [0] * K
    # a nu that satisfies the chunk column but not the V_0 check
    row = k.encrypt([3] * K, 11)
    if K == 1:
        nu = k.nu_for_chunk_columns_only(row, [2])
        assert nu != k.rho * row[0] % R and not k.decryption_verifies(row, [2], nu)
        assert (k.pairing_values(row, second=R - nu)[0] - k.power(0, 2)) % R == 0


def test_the_batch_equation_catches_what_cancels_unweighted():
    k = key(3, 4)
    rows = [k.encrypt([i % 16, 1, 2], 100 + i) for i in range(5)]
    w1, w2 = [1] * 5, [pow(2, i, R) for i in range(5)]
    assert k.batch_verifies(rows, w1) and k.batch_verifies(rows, w2) and k.batch_verifies([], [])
    rows[1][-1] = (rows[1][-1] + 9) % R
    rows[3][-1] = (rows[3][-1] - 9) % R
    assert not k.commitment_verifies(rows[1]) and not k.commitment_verifies(rows[3])
    assert k.batch_verifies(rows, w1) and not k.batch_verifies(rows, w2)


def test_the_model_is_the_oracles_pairing_on_a_handful_of_rows():
    k = key(2, 4, seed=9)
    e_gen = O.final_exponentiation(O.multi_miller_loop(O.G1.generator().reshape(1, 12), O.G2.generator().reshape(1, 24)))
    gt = lambda log: np.asarray(O.fp12_pow(e_gen, log % R), np.uint64)
    V1, V2 = g2_times(k.V_1()), g2_times(k.V_2())
    for msgs, r in (([5, 15], 1234567), ([0, 1], R - 2), ([16, 3], 99)):
        row = k.encrypt(msgs, r)
        pts = g1_times(row + [(R - k.rho * row[0]) % R])
        for j, log in enumerate(k.pairing_values(row)):
            p = O.final_exponentiation(O.multi_miller_loop(np.stack([pts[1 + j], pts[-1]]), np.stack([V2[j], V1[j]])))
            assert (np.asarray(p, np.uint64) == gt(log)).all()
            m = k.find(j, log)
            if m is not None:
                assert (gt(k.power(j, m)) == np.asarray(p, np.uint64)).all()
    # the table's entries are powers of the base
    base = O.final_exponentiation(O.multi_miller_loop(g1_times([k.a[0]]), V2[:1]))
    assert (np.asarray(O.fp12_pow(base, 7), np.uint64) == gt(k.power(0, 7))).all()
