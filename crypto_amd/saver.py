"""Mirror of the reference's saver crate (verifiable encryption over LegoGroth16; saver/src/encryption.rs, keygen.rs, utils.rs) in bulk on the C ABI: what the
authority that opens ciphertexts, the auditor of its decryptions and the verifier of a presentation run per ciphertext.  Encryption stays with the holder.

    PreparedDecryptionKey + pairing_powers(chunk_bit_size, g_i)                         -> DecryptionKey(g_i, H, V_0, V_1, V_2, chunk_bit_size)
    Ciphertext::decrypt_to_chunks_given_pairing_powers(.., sk, ..), n times             -> decrypt_chunks_many(dk, ct, sk)      returns (chunks, nu, status)
    Ciphertext::decrypt_given_pairing_powers (chunks composed into the message)         -> decrypt_many(dk, ct, sk)             returns (messages, nu, status)
    Ciphertext::verify_decryption(chunks, c_0, c, nu, dk, g_i, gens), n times           -> verify_decryption_each(dk, ct, chunks, nu)   returns ok
    Ciphertext::verify_ciphertext_commitment(c_0, c, commitment, ek, gens), n times     -> verify_commitment_each(key, ct)      returns ok
    Ciphertext::verify_commitments_in_batch(ciphertexts, r_powers, ek, gens)            -> verify_commitments_batch(key, ct, r_powers)  returns True / False

A ciphertext row is [c_0, c_1 .. c_K, psi] as a (K + 2, 12) uint64 array of affine Montgomery limbs (`Ciphertext { X_r, enc_chunks, commitment }`); G2 points
are (24,).  Zero words are the identity.  status: 0 decrypted, 1 the reference's CouldNotFindDiscreteLog (that row's chunks are zeros).

These calls are served by libdock_gpu_saver.so (include/dock_gpu_saver.h), a library of its own beside the product with its own contexts and handle table: this
module brings it up on the product's device(s) when it is first used (crypto_amd._native.saver_lib), and a DecryptionKey lives in it."""
import ctypes as C
import numpy as np
from ._native import saver_lib as lib, DockGpuError
from .msm import _ensure
from .fixed_base import _scalars_to_limbs, _p
from .pairing import PREPARED_WORDS

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def compose(chunks, chunk_bit_size):
    """utils.rs:48-73: the scalar of big-endian chunks, mod r; chunk_bit_size 4, 8 or 16 only (UnexpectedBase otherwise)"""
    b = int(chunk_bit_size)
    if b not in (4, 8, 16):
        raise ValueError("UnexpectedBase(%d)" % b)
    chunks = [int(c) for c in chunks]
    if b == 4:
        if len(chunks) % 2:
            raise ValueError("InvalidDecomposition")
        by = [((chunks[i] << 4) + chunks[i + 1]) & 255 for i in range(0, len(chunks), 2)]
    elif b == 8:
        by = [c & 255 for c in chunks]
    else:
        by = [x for c in chunks for x in ((c >> 8) & 255, c & 255)]
    return int.from_bytes(bytes(by), "big") % R


class DecryptionKey:
    """A decryption key resident on the device: the prepared coefficients of H, V_0, V_1, V_2, the table of the powers e(g_j, V_2_j)^m, m < 2^chunk_bit_size,
    and its search index (dgpu_saver_dk_create).  free() (or leaving a `with` block) releases it."""

    def __init__(self, g_i, H, V_0, V_1, V_2, chunk_bit_size):
        _ensure()
        g = np.ascontiguousarray(g_i, dtype=np.uint64).reshape(-1, 12)
        v1 = np.ascontiguousarray(V_1, dtype=np.uint64).reshape(-1, 24)
        v2 = np.ascontiguousarray(V_2, dtype=np.uint64).reshape(-1, 24)
        if not (len(g) == len(v1) == len(v2)):
            raise ValueError("%d generators, %d points of V_1, %d of V_2" % (len(g), len(v1), len(v2)))
        self.K, self.chunk_bit_size = len(g), int(chunk_bit_size)
        h = C.c_uint64(0)
        rc = lib().dgpu_saver_dk_create(_p(g), _p(np.ascontiguousarray(H, dtype=np.uint64).reshape(24)), _p(np.ascontiguousarray(V_0, dtype=np.uint64).reshape(24)),
                                        _p(v1), _p(v2), self.chunk_bit_size, self.K, C.byref(h))
        if rc:
            raise DockGpuError(rc, "dgpu_saver_dk_create")
        self.handle = h.value

    def powers(self, j, first=1, count=None):
        """pairing_powers[j][first - 1 : first - 1 + count] as a (count, 72) array: e(g_j, V_2_j)^m for m = first .."""
        if count is None:
            count = (1 << self.chunk_bit_size) - first
        out = np.zeros((count, 72), np.uint64)
        rc = lib().dgpu_saver_dk_powers(self.handle, j, first, count, _p(out) if count else None)
        if rc:
            raise DockGpuError(rc, "dgpu_saver_dk_powers")
        return out

    def free(self):
        if self.handle:
            lib().dgpu_saver_dk_free(self.handle)
            self.handle = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class CommitmentKey:
    """What the verifier of a presentation holds: the prepared coefficients of [Z_0 .. Z_K, H] (PreparedEncryptionKey::Z, PreparedEncryptionGens::H)"""

    def __init__(self, Z, H):
        z = np.ascontiguousarray(Z, dtype=np.uint64).reshape(-1, 24)
        self.K = len(z) - 1
        pts = np.ascontiguousarray(np.concatenate([z, np.asarray(H, dtype=np.uint64).reshape(1, 24)]))
        self.all_pc, inf = np.zeros((len(pts), PREPARED_WORDS), np.uint64), np.zeros(len(pts), np.uint8)
        _ensure()
        rc = lib().dgpu_g2_prepare(_p(pts), None, len(pts), _p(self.all_pc), _p(inf))
        if rc:
            raise DockGpuError(rc, "dgpu_g2_prepare")


def _rows(ct, K):
    a = np.ascontiguousarray(ct, dtype=np.uint64).reshape(-1, K + 2, 12)
    return a, len(a)


def decrypt_chunks_many(dk, ct, sk, montgomery=False):
    """(chunks, nu, status): chunks (n, K) uint16, nu (n, 12) = sk c_0, status (n,) uint8"""
    _ensure()
    a, n = _rows(ct, dk.K)
    chunks, nu, status = np.zeros((n, dk.K), np.uint16), np.zeros((n, 12), np.uint64), np.zeros(n, np.uint8)
    rc = lib().dgpu_saver_decrypt_many(dk.handle, _p(a) if n else None, n, _p(_scalars_to_limbs([sk] if isinstance(sk, int) else sk).reshape(4)), 1 if montgomery else 0,
                                       _p(chunks) if n else None, _p(nu) if n else None, _p(status) if n else None)
    if rc:
        raise DockGpuError(rc, "dgpu_saver_decrypt_many")
    return chunks, nu, status


def decrypt_many(dk, ct, sk, montgomery=False):
    """(messages, nu, status): messages[i] = compose(chunks[i]) as a Python integer, None where status[i] != 0"""
    if dk.chunk_bit_size not in (4, 8, 16):
        raise ValueError("UnexpectedBase(%d)" % dk.chunk_bit_size)
    chunks, nu, status = decrypt_chunks_many(dk, ct, sk, montgomery)
    return [None if st else compose(row, dk.chunk_bit_size) for row, st in zip(chunks, status)], nu, status


def verify_decryption_each(dk, ct, chunks, nu):
    """ok, an (n,) uint8 array: ok[i] = 1 iff verify_decryption accepts (chunks[i], nu[i]) for ciphertext i (else InvalidDecryption)"""
    _ensure()
    a, n = _rows(ct, dk.K)
    m = np.ascontiguousarray(chunks, dtype=np.uint16).reshape(-1, dk.K)
    v = np.ascontiguousarray(nu, dtype=np.uint64).reshape(-1, 12)
    if not (len(m) == len(v) == n):
        raise ValueError("%d ciphertexts, %d rows of chunks, %d values of nu" % (n, len(m), len(v)))
    ok = np.zeros(n, np.uint8)
    rc = lib().dgpu_saver_verify_decryption_each(dk.handle, _p(a) if n else None, n, _p(m) if n else None, _p(v) if n else None, _p(ok) if n else None)
    if rc:
        raise DockGpuError(rc, "dgpu_saver_verify_decryption_each")
    return ok


def verify_commitment_each(key, ct):
    """ok, an (n,) uint8 array: ok[i] = 1 iff e(c_0, Z_0) prod_j e(c_j, Z_j) e(-psi, H) = 1 (else InvalidCommitment)"""
    _ensure()
    a, n = _rows(ct, key.K)
    ok = np.zeros(n, np.uint8)
    rc = lib().dgpu_saver_verify_commitment_each(_p(key.all_pc), key.K, _p(a) if n else None, n, _p(ok) if n else None)
    if rc:
        raise DockGpuError(rc, "dgpu_saver_verify_commitment_each")
    return ok


def verify_commitments_batch(key, ct, r_powers, montgomery=False):
    """True iff the one multi-pairing over the K + 2 column sums weighted by r_powers is one (an empty batch verifies)"""
    _ensure()
    a, n = _rows(ct, key.K)
    w = _scalars_to_limbs(r_powers) if n else np.zeros((0, 4), np.uint64)
    if len(w) != n:
        raise ValueError("%d ciphertexts, %d weights" % (n, len(w)))
    ok = C.c_int32(0)
    rc = lib().dgpu_saver_verify_commitments_batch(_p(key.all_pc), key.K, _p(a) if n else None, n, _p(w) if n else None, 1 if montgomery else 0, C.byref(ok))
    if rc:
        raise DockGpuError(rc, "dgpu_saver_verify_commitments_batch")
    return bool(ok.value)
