"""GPU (-m gpu): the seven dgpu_saver_* calls (include/dock_gpu_saver.h, libdock_gpu_saver.so: crypto_amd/csrc/dock_saver.hip, saver_kernels.hip.h) through crypto_amd.saver.  Keys and ciphertexts come from
known discrete logs (tests/saver_model.py) through the oracle's G1 / G2 scalar multiplication, so every point is k G or k G2 for a k the model computes, every
expected chunk, status and verdict is decided in the exponent (tests/test_saver_model.py pins the model against the oracle's pairing), and the table's entries are
compared with the oracle's fp12_pow.  Every comparison is exact.  One scenario per (chunk_bit_size, K) is built once; every batch is a prefix of its rows."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import saver_model as M
import crypto_amd as ca
from crypto_amd import saver as S
from crypto_amd._native import saver_lib, twin, DockGpuError

pytestmark = pytest.mark.gpu
R = M.R
R2 = pow(2, 256, R)
BADARG = -3
SHAPES = [(4, 1), (4, 3), (8, 2), (16, 2)]
NS = [1, 2, 9, 65]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)
    yield


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def g1_times(scalars):
    """k G as affine ABI words (k = 0: zero words), on the oracle's host threads"""
    scalars = [k % R for k in scalars]
    out, inf = O.g1_scale_batch(np.tile(O.G1.generator(), (len(scalars), 1)), limbs(scalars), threads=16)
    out[inf.astype(bool)] = 0
    return out


def g2_times(scalars):
    g = O.G2.generator()
    return np.stack([np.zeros(24, np.uint64) if k % R == 0 else O.G2.to_affine(O.G2.mul(g, O.int_to_limbs(k % R, 4)))[0] for k in scalars])


_E_GEN = []


def gt_of(log):
    """e(G, G2)^log by the oracle"""
    if not _E_GEN:
        _E_GEN.append(O.final_exponentiation(O.multi_miller_loop(O.G1.generator().reshape(1, 12), O.G2.generator().reshape(1, 24))))
    return np.asarray(O.fp12_pow(_E_GEN[0], log % R), np.uint64)


class Scenario:
    """rows 0 .. 9: legal messages with the edge chunks; 10 ..: what must not decrypt (the model decides each); the rest random legal messages"""
    def __init__(self, b, K, rows=65, seed=7):
        rng = np.random.default_rng(seed * 1000 + b * 10 + K)
        d, h, rho = rand(rng, 3)
        self.b, self.K, self.rows = b, K, rows
        self.key = k = M.Key(rand(rng, K), d, h, rho, rand(rng, K), rand(rng, K + 1), rand(rng, K), b)
        E = k.E
        legal = lambda: [int(x) % (E + 1) for x in rng.integers(0, 1 << 16, K)]
        self.msgs = [legal() for _ in range(rows)]
        edge = [[0] * K, [E] * K, [0] + [E] * (K - 1), [E] + [0] * (K - 1), [1] + [0] * (K - 1), [0] * (K - 1) + [1], [1] * K, [E - 1 if E > 1 else 1] * K]
        for i, m in enumerate(edge[:rows - 1]):
            self.msgs[1 + i] = m
        self.bad = {}
        if rows > 20:
            self.msgs[10] = [E + 1] + legal()[1:]; self.bad[10] = "chunk of 2^b"
            self.msgs[11] = legal()[:-1] + [R - 1]; self.bad[11] = "r - 1 as a chunk"
        self.r = rand(rng, rows)
        self.logs = [k.encrypt(m, r) for m, r in zip(self.msgs, self.r)]
        if rows > 20:
            self.logs[12][1] = rand(rng, 1)[0]; self.bad[12] = "a replaced c_1"
            self.logs[13][0] = rand(rng, 1)[0]; self.bad[13] = "a replaced c_0"
            self.logs[14] = k.encrypt([3] * K, 5); self.logs[14][0] = 0; self.bad[14] = "an identity c_0 with a non-zero message"
            self.logs[15][K] = 0; self.bad[15] = "an identity c_K"
            self.logs[16] = k.encrypt([0] * K, 5); self.logs[16][0] = 0      # identity c_0, zero message: whatever the model says
        self.ct = g1_times([v for row in self.logs for v in row]).reshape(rows, K + 2, 12)
        self.g = g1_times(k.a)
        g2 = g2_times([k.H(), k.V_0()] + k.V_1() + k.V_2() + k.Z())
        self.H, self.V0, self.V1, self.V2, self.Z = g2[0], g2[1], g2[2:2 + K], g2[2 + K:2 + 2 * K], g2[2 + 2 * K:]
        self.expect = [k.decrypt(row) for row in self.logs]

    def dk(self):
        return S.DecryptionKey(self.g, self.H, self.V0, self.V1, self.V2, self.b)

    def ck(self):
        return S.CommitmentKey(self.Z, self.H)

    def check_decrypt(self, dk, n, sk=None, montgomery=False):
        sk = self.key.rho if sk is None else sk
        chunks, nu, status = S.decrypt_chunks_many(dk, self.ct[:n], sk * R2 % R if montgomery else sk, montgomery=montgomery)
        want = self.expect[:n] if sk == self.key.rho else [model_decrypt(self.key, row, sk) for row in self.logs[:n]]
        assert [int(s) for s in status] == [w[0] for w in want]
        assert chunks.tolist() == [w[1] for w in want]
        assert (nu == g1_times([sk * row[0] for row in self.logs[:n]])).all()
        return chunks, nu, status


def model_decrypt(k, row, sk):
    """the model's decrypt with ANOTHER secret key over the same public key"""
    found = [k.find(j, p) for j, p in enumerate(k.pairing_values(row, second=R - sk * row[0]))]
    return (1, [0] * k.K, sk * row[0] % R) if any(m is None for m in found) else (0, found, sk * row[0] % R)


_SC = {}


def scenario(b, K, rows=65):
    if (b, K) not in _SC:
        _SC[(b, K)] = Scenario(b, K, rows)
    return _SC[(b, K)]


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,K,entries", [(4, 3, list(range(1, 16))), (8, 2, [1, 2, 3, 127, 128, 129, 254, 255]), (16, 2, [1, 2, 32767, 32768, 32769, 65534, 65535]),
                                         (1, 1, [1])])
def test_table_entries_are_the_oracles_powers(b, K, entries):
    sc = scenario(b, K) if (b, K) in SHAPES else Scenario(b, K, rows=2)
    with sc.dk() as dk:
        for j in range(K):
            base = np.asarray(O.final_exponentiation(O.multi_miller_loop(sc.g[j:j + 1], sc.V2[j:j + 1])), np.uint64)
            assert (base == gt_of(sc.key.base(j))).all()
            for m in entries:
                got = dk.powers(j, m, 1)[0]
                assert (got == np.asarray(O.fp12_pow(base, m), np.uint64)).all(), (j, m)
        # a run of entries in one call, and the bounds of the call
        run = dk.powers(K - 1, 1, min(3, (1 << b) - 1))
        assert (run[0] == dk.powers(K - 1, 1, 1)[0]).all()
        for j, first, count in ((K, 1, 1), (0, 0, 1), (0, 1 << b, 1), (0, (1 << b) - 1, 2)):
            with pytest.raises(DockGpuError):
                dk.powers(j, first, count)


def test_handles_of_another_kind_and_freed_handles_are_refused():
    sc = scenario(4, 3)
    import ctypes
    L = saver_lib()                                                       # handles live in the library that made them: a bases handle of THIS library
    out, st, bh = np.zeros((1, 72), np.uint64), np.zeros(1, np.uint8), ctypes.c_uint64(0)
    p_ = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    g = np.ascontiguousarray(sc.g)
    assert L.dgpu_bases_upload_g1(p_(g), None, len(g), ctypes.byref(bh)) == 0 and bh.value
    assert L.dgpu_saver_dk_powers(bh.value, 0, 1, 1, p_(out)) == BADARG
    assert L.dgpu_saver_dk_free(bh.value) == BADARG
    assert L.dgpu_saver_verify_decryption_each(bh.value, p_(sc.ct), 1, p_(np.zeros(3, np.uint16)), p_(np.zeros(12, np.uint64)), p_(st)) == BADARG
    assert L.dgpu_bases_free(bh.value) == 0
    dk = sc.dk()
    h = dk.handle
    assert L.dgpu_bases_free(h) == BADARG                                 # ... and a key is no bases handle
    dk.free()
    assert L.dgpu_saver_dk_free(h) == BADARG
    assert L.dgpu_saver_dk_powers(h, 0, 1, 1, p_(out)) == BADARG


# ---- decryption --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,K", SHAPES)
def test_decrypt_against_the_model(b, K):
    sc = scenario(b, K)
    assert {10, 11, 12, 13, 14} <= {i for i, e in enumerate(sc.expect) if e[0] == 1}, "the rows that must not decrypt do not, in the model"
    assert all(sc.expect[i][0] == 0 and sc.expect[i][1] == sc.msgs[i] for i in range(10))
    with sc.dk() as dk:
        for n in NS:
            sc.check_decrypt(dk, n)
        sc.check_decrypt(dk, 9, montgomery=True)
        _, _, status = sc.check_decrypt(dk, 20, sk=(sc.key.rho + 1) % R)   # a wrong secret key
        assert status[:10].all()


def test_decrypt_the_real_shape_composes_messages():
    sc = Scenario(4, 64, rows=3)
    msgs = [0, R - 1, 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R]
    logs = [sc.key.encrypt(M.decompose(m, 4), r) for m, r in zip(msgs, sc.r)]
    ct = g1_times([v for row in logs for v in row]).reshape(3, 66, 12)
    with sc.dk() as dk:
        got, nu, status = S.decrypt_many(dk, ct, sc.key.rho)
        assert got == msgs and not status.any()
        assert (nu == g1_times([sc.key.rho * row[0] for row in logs])).all()
        ok = S.verify_decryption_each(dk, ct, [M.decompose(m, 4) for m in msgs], nu)
        assert ok.tolist() == [1, 1, 1]
    with Scenario(1, 1, rows=2).dk() as dk1, pytest.raises(ValueError, match="UnexpectedBase"):
        S.decrypt_many(dk1, np.zeros((1, 3, 12), np.uint64), 5)


def test_forced_chunks_fingerprint_runs_and_threads():
    """on the development twin: 16 pairing rows per chunk (five ciphertexts at K = 3, the last chunk ragged) and fingerprints cut to 3 bits (fifteen entries share
    eight values: runs exist by pigeonhole) and to none (the whole column is one run) give the chunks the full fingerprint gives; two threads on one handle too"""
    sc = scenario(4, 3)
    with sc.dk() as dk:
        base = S.decrypt_chunks_many(dk, sc.ct, sc.key.rho)
    with twin(saver=True) as T:
        try:
            assert T.dgpu_set_many_chunk_rows(16) == 0
            for bits in (3, -1, 0):
                assert T.dgpu_dev_set_saver_fp_bits(bits) == 0
                with sc.dk() as dk:
                    for n in NS:
                        sc.check_decrypt(dk, n)
                    got = sc.check_decrypt(dk, sc.rows)
                    assert all((a == b).all() for a, b in zip(got, base))
                    ok = S.verify_decryption_each(dk, sc.ct, got[0], got[1])
                    assert ok.tolist() == [1 if sc.key.decryption_verifies(row, e[1], e[2]) else 0 for row, e in zip(sc.logs, sc.expect)]
            assert T.dgpu_set_many_chunk_rows(0) == 0
            with sc.dk() as dk, ThreadPoolExecutor(2) as ex:
                res = list(ex.map(lambda _: S.decrypt_chunks_many(dk, sc.ct, sc.key.rho), range(4)))
            for r in res:
                assert all((a == b).all() for a, b in zip(r, base))
        finally:
            T.dgpu_set_many_chunk_rows(0)
            T.dgpu_dev_set_saver_fp_bits(0)


# ---- verify_decryption ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,K", SHAPES)
def test_verify_decryption_against_the_model(b, K):
    sc = scenario(b, K)
    k, E = sc.key, sc.key.E
    good = [i for i, e in enumerate(sc.expect) if e[0] == 0]
    cases = []                                                            # (row, chunks, nu log)
    for i in good[:12]:
        cases.append((i, list(sc.expect[i][1]), sc.expect[i][2]))
    i_zero, i_top, i_one = 1, 2, 7                                        # messages of all 0, all E, all 1
    for i, j, delta in ((0, 0, 1), (0, K - 1, -1), (i_top, K - 1, -1), (i_one, 0, 1), (i_one, K - 1, -1)):
        ch = list(sc.expect[i][1]); ch[j] = (ch[j] + delta) % (E + 1)
        cases.append((i, ch, sc.expect[i][2]))
    ch = list(sc.expect[i_top][1]); ch[0] = 0; cases.append((i_top, ch, sc.expect[i_top][2]))          # m = 0 where p is not one
    ch = list(sc.expect[i_zero][1]); ch[K - 1] = 1; cases.append((i_zero, ch, sc.expect[i_zero][2]))   # m != 0 where p is one
    if b < 16:
        ch = list(sc.expect[i_one][1]); ch[0] = E + 1; cases.append((i_one, ch, sc.expect[i_one][2]))  # m = 2^b
    cases.append((0, list(sc.expect[0][1]), (sc.expect[0][2] + 1) % R))                                # a wrong nu
    cases.append((0, list(sc.expect[0][1]), 0))                                                        # the identity as nu
    if K == 1:                                                            # a nu that satisfies the chunk column for another chunk, not the V_0 check
        other = [(sc.expect[0][1][0] + 1) % (E + 1)]
        cases.append((0, other, k.nu_for_chunk_columns_only(sc.logs[0], other)))
    for i in (12, 13, 16):                                                # tampered rows with the decryptor's claim for the untouched ciphertext
        cases.append((i, [c % (E + 1) for c in sc.msgs[i]], k.rho * sc.logs[i][0] % R))
    cases.append((13, [c % (E + 1) for c in sc.msgs[13]], k.rho * sc.r[13] * k.d % R))                 # ... and nu of the c_0 that was replaced
    want = [1 if k.decryption_verifies(sc.logs[i], ch, nu) else 0 for i, ch, nu in cases]
    assert want[:len(good[:12])] == [1] * len(good[:12]) and not any(want[len(good[:12]):len(good[:12]) + 7])
    ct = np.stack([sc.ct[i] for i, _, _ in cases])
    nus = g1_times([nu for _, _, nu in cases])
    with sc.dk() as dk:
        ok = S.verify_decryption_each(dk, ct, [ch for _, ch, _ in cases], nus)
        assert ok.tolist() == want
        # the decryptor's own output for the whole batch: accepted exactly where it decrypted
        chunks, nu, status = S.decrypt_chunks_many(dk, sc.ct, k.rho)
        assert S.verify_decryption_each(dk, sc.ct, chunks, nu).tolist() == [1 if k.decryption_verifies(row, e[1], e[2]) else 0 for row, e in zip(sc.logs, sc.expect)]
        assert S.verify_decryption_each(dk, sc.ct[:1], chunks[:1], nu[:1]).tolist() == [1]


# ---- commitments -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,K,n", [(4, 1, 9), (4, 3, 65), (4, 64, 3)])
def test_commitments_each_and_batch(b, K, n):
    sc = scenario(b, K) if (b, K) in SHAPES else Scenario(b, K, rows=3)
    k = sc.key
    logs = [k.encrypt(m, r) for m, r in zip(sc.msgs[:n], sc.r[:n])]       # (any scalar vector commits: rows 10, 11 too)
    ck = sc.ck()
    valid = g1_times([v for row in logs for v in row]).reshape(n, K + 2, 12)
    assert all(k.commitment_verifies(row) for row in logs)
    assert S.verify_commitment_each(ck, valid).tolist() == [1] * n
    for m in sorted({1, 2, n}):
        assert S.verify_commitment_each(ck, valid[:m]).tolist() == [1] * m
    rho = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
    w = [pow(rho, i, R) for i in range(n)]
    assert k.batch_verifies(logs, w) and S.verify_commitments_batch(ck, valid, w)
    assert S.verify_commitments_batch(ck, valid, limbs([v * R2 % R for v in w]), montgomery=True)
    assert S.verify_commitments_batch(ck, np.zeros((0, K + 2, 12), np.uint64), [])
    # psi, one c_j, c_0 tampered in single rows
    bad = [list(row) for row in logs]
    hit = {0: K + 1, n // 2: 1, n - 1: 0} if n >= 3 else {0: K + 1}
    for i, col in hit.items():
        bad[i][col] = (bad[i][col] + 1 + i) % R
    pts = g1_times([v for row in bad for v in row]).reshape(n, K + 2, 12)
    want = [1 if k.commitment_verifies(row) else 0 for row in bad]
    assert want == [0 if i in hit else 1 for i in range(n)]
    assert S.verify_commitment_each(ck, pts).tolist() == want
    assert not k.batch_verifies(bad, w) and not S.verify_commitments_batch(ck, pts, w)
    one_bad = [list(row) for row in logs]; one_bad[n - 1][K + 1] = (one_bad[n - 1][K + 1] + 1) % R
    assert not S.verify_commitments_batch(ck, g1_times([v for row in one_bad for v in row]).reshape(n, K + 2, 12), w)
    if n >= 3:
        # two errors that cancel unweighted pass at rho = 1 and fail at rho = 2
        canc = [list(row) for row in logs]
        canc[0][K + 1] = (canc[0][K + 1] + 9) % R; canc[2][K + 1] = (canc[2][K + 1] - 9) % R
        cp = g1_times([v for row in canc for v in row]).reshape(n, K + 2, 12)
        w1, w2 = [1] * n, [pow(2, i, R) for i in range(n)]
        assert k.batch_verifies(canc, w1) and not k.batch_verifies(canc, w2)
        assert S.verify_commitments_batch(ck, cp, w1) and not S.verify_commitments_batch(ck, cp, w2)
        assert S.verify_commitment_each(ck, cp).tolist() == [0, 1, 0] + [1] * (n - 3)


def test_commitments_in_forced_chunks():
    sc = scenario(4, 3)
    logs = [sc.key.encrypt(m, r) for m, r in zip(sc.msgs, sc.r)]
    logs[7][2] = (logs[7][2] + 1) % R
    logs[64][0] = (logs[64][0] + 1) % R
    pts = g1_times([v for row in logs for v in row]).reshape(sc.rows, 5, 12)
    want = [0 if i in (7, 64) else 1 for i in range(sc.rows)]
    w = [pow(3, i, R) for i in range(sc.rows)]
    with twin(saver=True) as T:
        try:
            assert T.dgpu_set_many_chunk_rows(16) == 0                    # three rows of five pairs per chunk; the batch in MSMs of 16 rows
            ck = sc.ck()
            assert S.verify_commitment_each(ck, pts).tolist() == want
            assert not S.verify_commitments_batch(ck, pts, w)
            good = [i for i in range(sc.rows) if want[i]]
            assert S.verify_commitments_batch(ck, pts[good], [w[i] for i in good])
        finally:
            T.dgpu_set_many_chunk_rows(0)
