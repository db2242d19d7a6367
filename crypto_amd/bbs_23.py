"""Mirror of the 2023 BBS scheme in G1 (bbs_plus/src/signature_23.rs: Signature23G1, SignatureParams23G1; proof_23_cdl.rs and proof_23_ietf.rs: the two
PoKOfSignature23G1Proof) in bulk on the C ABI.  The scheme has no s and no h_0.

    SignatureParams23G1 { g1, g2, h } + PublicKeyG2(w)            -> Params23(g1, h, g2, w)                 uploads [g1, h ..], prepares w and g2
    Signature23G1::new(rng, messages, sk, params), n times        -> sign_many(params, sk, messages, e)     returns (A, bad)
    sig.verify(messages, pk, params), n times                     -> verify_each(params, A, e, messages)    returns ok, one byte per signature
    the same through RandomizedPairingChecker                     -> verify_batch(params, A, e, messages, random)     returns True / False
    proof_23_cdl's proof.verify(revealed, challenge, pk, params)  -> pok_verify_each(params, points, resp_fixed, values, revealed, challenge)     status per proof
    the same with one verdict for all                             -> pok_verify_batch(.., random)           returns True / False
    proof_23_ietf's proof.verify(..)                              -> pok_ietf_verify_each / pok_ietf_verify_batch
    the two compute_challenge_contribution                        -> challenge_contribution / challenge_contribution_ietf     return bytes

`e` stands in for the `rand` draw of Signature23G1::new, so signing is deterministic.  Scalars, messages, points and `montgomery` are as in crypto_amd.bbs_plus.
"""
import ctypes as C
import numpy as np
from ._native import lib, DockGpuError
from .msm import G1, _ensure, DeviceBases
from .fixed_base import _scalars_to_limbs, _p
from .pairing import G2Prepared
from .bbs_plus import _messages, _sigs, STATUS  # noqa: F401  (STATUS: the status bytes keep the reference's names; the IETF calls never return 2)


class Params23:
    """The signature parameters and the public key of one issuer on the device: a plain G1 bases handle holding [g1, h_1 .. h_L] and the prepared coefficients
    of w and g2.  free() (or leaving a `with` block) releases the handle."""

    def __init__(self, g1, h, g2, w):
        _ensure()
        h = np.ascontiguousarray(h, dtype=np.uint64).reshape(-1, 12)
        self.L = len(h)
        if self.L == 0:
            raise ValueError("NoMessageToSign")                                  # signature_23.rs:47-49
        self.bases = DeviceBases(G1, np.concatenate([np.asarray(g1, dtype=np.uint64).reshape(1, 12), h]))
        pc = G2Prepared.from_affine(np.stack([np.asarray(w, dtype=np.uint64).reshape(24), np.asarray(g2, dtype=np.uint64).reshape(24)]))
        self.pk_pc, self.g2_pc = np.ascontiguousarray(pc.coeffs[0]), np.ascontiguousarray(pc.coeffs[1])

    @property
    def handle(self):
        return self.bases.handle

    def free(self):
        if self.bases is not None:
            self.bases.free()
            self.bases = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


def _rows(params, e, messages):
    m, stride, n = _messages(messages, params.L)
    e = _scalars_to_limbs(e) if n else np.zeros((0, 4), np.uint64)
    if len(e) != n:
        raise ValueError("%d rows of messages, %d values of e" % (n, len(e)))
    return m, stride, n, e


def _one(x):
    return _scalars_to_limbs([x] if isinstance(x, int) else x).reshape(4)


def sign_many(params, sk, messages, e, montgomery=False):
    """(A, bad): A_i = (sk + e_i)^-1 (g1 + sum_j m_ij h_j) as an (n, 12) array; bad[i] = 1 (and zero words) where no signature exists: sk + e_i = 0, where
    the reference draws e again, or an identity b_i"""
    _ensure()
    m, stride, n, e = _rows(params, e, messages)
    out, bad = np.zeros((n, 12), np.uint64), np.zeros(n, np.uint8)
    rc = lib().dgpu_bbs23_sign_many_g1(params.handle, params.L, _p(_one(sk)), _p(m) if n else None, stride, _p(e) if n else None, n, 1 if montgomery else 0,
                                       _p(out) if n else None, _p(bad) if n else None)
    if rc:
        raise DockGpuError(rc, "dgpu_bbs23_sign_many_g1")
    return out, bad


def verify_each(params, sig_a, e, messages, montgomery=False):
    """ok, an (n,) uint8 array: ok[i] = 1 iff A_i is not the identity and e(A_i, w) e(e_i A_i - b_i, g2) = 1 (signature_23.rs:136-160)"""
    _ensure()
    m, stride, n, e = _rows(params, e, messages)
    a = _sigs(sig_a, n)
    ok = np.zeros(n, np.uint8)
    rc = lib().dgpu_bbs23_verify_each_g1(params.handle, params.L, _p(params.pk_pc), _p(params.g2_pc), _p(a) if n else None, _p(e) if n else None, _p(m) if n else None,
                                         stride, n, 1 if montgomery else 0, _p(ok) if n else None)
    if rc:
        raise DockGpuError(rc, "dgpu_bbs23_verify_each_g1")
    return ok


def verify_batch(params, sig_a, e, messages, random, montgomery=False):
    """True iff every signature verifies, by one pairing check over the random linear combination with the weights random^i (non-zero modulo r)"""
    _ensure()
    m, stride, n, e = _rows(params, e, messages)
    a = _sigs(sig_a, n)
    ok = C.c_int32(0)
    rc = lib().dgpu_bbs23_verify_batch_g1(params.handle, params.L, _p(params.pk_pc), _p(params.g2_pc), _p(a) if n else None, _p(e) if n else None, _p(m) if n else None,
                                          stride, n, 1 if montgomery else 0, _p(_one(random)), C.byref(ok))
    if rc:
        raise DockGpuError(rc, "dgpu_bbs23_verify_batch_g1")
    return bool(ok.value)


# ---- proofs of knowledge of a signature: proof_23_cdl.rs (5 points, 3 fixed responses) and proof_23_ietf.rs (3 points, 2 fixed responses) -------------------
def _proofs(params, npts, nresp, points, resp_fixed, values, revealed, challenge):
    v, stride, n = _messages(values, params.L)
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, npts, 12)
    flat = resp_fixed if isinstance(resp_fixed, np.ndarray) and resp_fixed.dtype == np.uint64 else [z for r in resp_fixed for z in r]
    fixed = _scalars_to_limbs(flat).reshape(-1, nresp, 4) if n else np.zeros((0, nresp, 4), np.uint64)
    rev = np.ascontiguousarray(np.asarray(revealed) != 0, dtype=np.uint8).reshape(-1, params.L) if n else np.zeros((0, params.L), np.uint8)
    c = _scalars_to_limbs(challenge) if n else np.zeros((0, 4), np.uint64)
    if not (len(pts) == len(fixed) == len(rev) == len(c) == n):
        raise ValueError("%d rows of values, %d proofs' points, %d of fixed responses, %d masks, %d challenges" % (n, len(pts), len(fixed), len(rev), len(c)))
    return v, stride, n, pts, fixed, rev, c


def _each(name, npts, nresp, params, points, resp_fixed, values, revealed, challenge, montgomery):
    _ensure()
    v, stride, n, pts, fixed, rev, c = _proofs(params, npts, nresp, points, resp_fixed, values, revealed, challenge)
    status = np.zeros(n, np.uint8)
    rc = getattr(lib(), name)(params.handle, params.L, _p(params.pk_pc), _p(params.g2_pc), _p(pts) if n else None, _p(fixed) if n else None, _p(v) if n else None, stride,
                              _p(rev) if n else None, _p(c) if n else None, n, 1 if montgomery else 0, _p(status) if n else None)
    if rc:
        raise DockGpuError(rc, name)
    return status


def _batch(name, npts, nresp, params, points, resp_fixed, values, revealed, challenge, random, montgomery):
    _ensure()
    v, stride, n, pts, fixed, rev, c = _proofs(params, npts, nresp, points, resp_fixed, values, revealed, challenge)
    ok = C.c_int32(0)
    rc = getattr(lib(), name)(params.handle, params.L, _p(params.pk_pc), _p(params.g2_pc), _p(pts) if n else None, _p(fixed) if n else None, _p(v) if n else None, stride,
                              _p(rev) if n else None, _p(c) if n else None, n, 1 if montgomery else 0, _p(_one(random)), C.byref(ok))
    if rc:
        raise DockGpuError(rc, name)
    return bool(ok.value)


def pok_verify_each(params, points, resp_fixed, values, revealed, challenge, montgomery=False):
    """status, an (n,) uint8 array: 0 where proof_23_cdl's PoKOfSignature23G1Proof::verify accepts proof i, else the first of its errors in the order it returns
    them (STATUS): 1 ZeroSignature (Abar is the identity), 2 the first Schnorr check z1 Abar + z2 d - c Bbar = T1, 3 the second, sum_hidden z_j h_j + z3 d +
    c (g1 + sum_revealed m_j h_j) = T2, 4 the pairing e(Abar, w) e(-Bbar, g2) = 1.

    points: (n, 5, 12), Abar, Bbar, d, T1 (sc_resp_1.t), T2.  resp_fixed: (n, 3) scalars z1, z2 (sc_resp_1.response1 / .response2), z3 (the last response of
    sc_resp_2, over d).  values: n rows of L scalars; entry j is the revealed message where revealed[i][j] is non-zero, else the response of the hidden message
    j.  A proof with partial responses needs no path of its own: write the missing responses into the row.  The points are taken as validated members of the
    subgroup, as the reference takes them (crypto_amd.serde.validate)."""
    return _each("dgpu_bbs23_pok_verify_each_g1", 5, 3, params, points, resp_fixed, values, revealed, challenge, montgomery)


def pok_verify_batch(params, points, resp_fixed, values, revealed, challenge, random, montgomery=False):
    """True iff every CDL proof verifies, by ONE G1 equation and one pairing check over the random linear combination with the weights random^(2i) on the first
    Schnorr check of proof i, random^(2i+1) on the second and random^i on the pairing (random non-zero modulo r; an empty batch verifies)."""
    return _batch("dgpu_bbs23_pok_verify_batch_g1", 5, 3, params, points, resp_fixed, values, revealed, challenge, random, montgomery)


def pok_ietf_verify_each(params, points, resp_fixed, values, revealed, challenge, montgomery=False):
    """status as above for proof_23_ietf's PoKOfSignature23G1Proof::verify: 1 ZeroSignature, 3 its one Schnorr check sum_hidden z_j h_j + z_a Abar + z_b Bbar +
    c (g1 + sum_revealed m_j h_j) = T, 4 the pairing; never 2.  points: (n, 3, 12), Abar, Bbar, T.  resp_fixed: (n, 2) scalars z_a, z_b, the last two
    responses of sc_resp (over Abar and Bbar)."""
    return _each("dgpu_bbs23_pok_ietf_verify_each_g1", 3, 2, params, points, resp_fixed, values, revealed, challenge, montgomery)


def pok_ietf_verify_batch(params, points, resp_fixed, values, revealed, challenge, random, montgomery=False):
    """True iff every IETF proof verifies, by ONE G1 equation and one pairing check with the weights random^i on both"""
    return _batch("dgpu_bbs23_pok_ietf_verify_batch_g1", 3, 2, params, points, resp_fixed, values, revealed, challenge, random, montgomery)


def _contribution(head_of, npts, param_points, proof_points, revealed_row, values_row):
    from . import serde
    P = np.ascontiguousarray(param_points, dtype=np.uint64).reshape(-1, 12)
    Q = np.ascontiguousarray(proof_points, dtype=np.uint64).reshape(npts, 12)
    L = len(P) - 1
    if len(revealed_row) != L or len(values_row) != L:
        raise ValueError("a row of %d mask bytes and %d values for %d generators" % (len(revealed_row), len(values_row), L))
    out = [serde.serialize(G1, np.stack(head_of(P, Q)))]
    hs = serde.serialize(G1, P[1:])
    for j in range(L):
        out.append(hs[48 * j:48 * j + 48])
        if revealed_row[j]:
            out.append(int(values_row[j]).to_bytes(32, "little"))
    return b"".join(out)


def challenge_contribution(param_points, proof_points, revealed_row, values_row):
    """The bytes proof_23_cdl's compute_challenge_contribution writes for one proof (proof_23_cdl.rs:272-296): Abar, Bbar, d, g1, T1, T2 compressed, then every
    h_j compressed, followed by m_j as 32 little-endian bytes where j is revealed.  param_points: (L + 1, 12) = [g1, h ..]; proof_points: (5, 12);
    values_row: L canonical integers (only the revealed entries are read).  Hashing the bytes to a challenge stays with the caller."""
    return _contribution(lambda P, Q: [Q[0], Q[1], Q[2], P[0], Q[3], Q[4]], 5, param_points, proof_points, revealed_row, values_row)


def challenge_contribution_ietf(param_points, proof_points, revealed_row, values_row):
    """The same for proof_23_ietf (proof_23_ietf.rs:218-238): Abar, Bbar, g1, T compressed, then the h_j and the revealed messages as above.  proof_points: (3, 12)"""
    return _contribution(lambda P, Q: [Q[0], Q[1], P[0], Q[2]], 3, param_points, proof_points, revealed_row, values_row)
