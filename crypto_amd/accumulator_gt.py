"""The accumulator proofs with a GT commitment verified in bulk (include/dock_gpu_acc_gt.h, crypto_amd/csrc/dock_acc_gt.hip): MembershipProof::verify and
NonMembershipProof::verify of the reference's vb_accumulator/src/proofs.rs — the proofs behind the statements VBAccumulatorMembership / VBAccumulatorNonMembership
and, through kb_universal_accumulator/proofs.rs, KBUniversalAccumulatorMembership / KBUniversalAccumulatorNonMembership — for many proofs against ONE accumulator
value and one key.  The calls are served by libdock_gpu_acc_gt.so, a library of its own beside the product, brought up on the product's device(s) when it is first
used (crypto_amd._native.acc_gt_lib).  The key is crypto_amd.accumulator.VerifierKey, as for the CDH proofs.

A proof is its points — membership (7, 12): E_C, T_sigma, T_rho, R_sigma, R_rho, R_delta_sigma, R_delta_rho; non-membership (11, 12): those, then E_d, E_d_inv,
R_A, R_B — its GT element R_E (72 words, as crypto_amd.pairing holds GT elements), its responses — (5,): s_sigma, s_rho, s_delta_sigma, s_delta_rho, s_y;
non-membership (8,): those, then s_u, s_v, s_w; for a partial proof the caller writes resp_for_element into s_y — and its challenge, computed by the caller.
Points are taken as validated subgroup members and R_E as members of GT (crypto_amd.serde.validate, crypto_amd.pairing's GT membership test)."""
import ctypes as C
import numpy as np
from ._native import acc_gt_lib as lib, DockGpuError
from .msm import _ensure
from .fixed_base import _scalars_to_limbs, _p
from .accumulator import VerifierKey, _point  # noqa: F401  (VerifierKey: the key these calls take)

# the first failing check in the order the reference returns its errors (VBAccumulatorError)
MEMBERSHIP_STATUS = {0: "verified", 1: "SigmaResponseInvalid", 2: "RhoResponseInvalid", 3: "DeltaSigmaResponseInvalid", 4: "DeltaRhoResponseInvalid",
                     5: "PairingResponseInvalid"}
NON_MEMBERSHIP_STATUS = {0: "verified", 1: "E_d_ResponseInvalid", 2: "E_d_inv_ResponseInvalid", 3: "SigmaResponseInvalid", 4: "RhoResponseInvalid",
                         5: "DeltaSigmaResponseInvalid", 6: "DeltaRhoResponseInvalid", 7: "PairingResponseInvalid"}


def _proofs(points, npts, r_e, responses, nresp, challenge):
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, npts, 12)
    n = len(pts)
    gt = np.ascontiguousarray(r_e, dtype=np.uint64).reshape(-1, 72)
    flat = responses if isinstance(responses, np.ndarray) and responses.dtype == np.uint64 else [z for r in responses for z in r]
    resp = _scalars_to_limbs(flat).reshape(-1, nresp, 4) if n else np.zeros((0, nresp, 4), np.uint64)
    c = _scalars_to_limbs(challenge) if n else np.zeros((0, 4), np.uint64)
    if not (len(resp) == len(c) == len(gt) == n):
        raise ValueError("%d proofs' points, %d GT elements, %d rows of responses, %d challenges" % (n, len(gt), len(resp), len(c)))
    return n, (pts, gt, resp, c)


def _prk(prk, k):
    return np.ascontiguousarray(prk, dtype=np.uint64).reshape(k, 12)


def _each(name, head, n, arrays, montgomery):
    status = np.zeros(n, np.uint8)
    rc = getattr(lib(), name)(*head, *[_p(a) if n else None for a in arrays], n, 1 if montgomery else 0, _p(status) if n else None)
    if rc:
        raise DockGpuError(rc, name)
    return status


def _batch(name, head, n, arrays, random, montgomery):
    rho = _scalars_to_limbs([random] if isinstance(random, int) else random).reshape(4)
    ok = C.c_int32(0)
    rc = getattr(lib(), name)(*head, *[_p(a) if n else None for a in arrays], n, 1 if montgomery else 0, _p(rho), C.byref(ok))
    if rc:
        raise DockGpuError(rc, name)
    return bool(ok.value)


def membership_proofs_verify_each(key, accumulator, prk, points, r_e, responses, challenge, montgomery=False):
    """status, an (n,) uint8 array: 0 where MembershipProof::verify accepts proof i against the accumulator value V, else the first failing check in the
    reference's order (MEMBERSHIP_STATUS): 1 .. 4 the Schnorr checks of sigma, rho, delta_sigma, delta_rho, 5 e(p, P~) e(q, pk) = R_E.

    prk: (3, 12), the proving key's X, Y, Z.  points: (n, 7, 12); r_e: (n, 72); responses: (n, 5)."""
    _ensure()
    n, arrays = _proofs(points, 7, r_e, responses, 5, challenge)
    X = _prk(prk, 3)
    return _each("dgpu_accumulator_gt_membership_proofs_verify_each_g1", (_p(_point(accumulator)), _p(X), _p(key.pk_pc), _p(key.ptilde_pc)), n, arrays, montgomery)


def membership_proofs_verify_batch(key, accumulator, prk, points, r_e, responses, challenge, random, montgomery=False):
    """True iff every proof verifies, by ONE G1 equation over all Schnorr checks (check j of proof i weighs random^(4 i + j)) and one pairing check against the
    GT product of the R_E_i^(random^i) (random non-zero modulo r; an empty batch verifies)"""
    _ensure()
    n, arrays = _proofs(points, 7, r_e, responses, 5, challenge)
    X = _prk(prk, 3)
    return _batch("dgpu_accumulator_gt_membership_proofs_verify_batch_g1", (_p(_point(accumulator)), _p(X), _p(key.pk_pc), _p(key.ptilde_pc)), n, arrays, random, montgomery)


def non_membership_proofs_verify_each(key, accumulator, P, prk, points, r_e, responses, challenge, montgomery=False):
    """status, an (n,) uint8 array: 0 where NonMembershipProof::verify accepts proof i, else the first failing check in the reference's order
    (NON_MEMBERSHIP_STATUS): 1 the check of E_d, 2 that of E_d_inv, 3 .. 6 the four Schnorr checks of the membership part, 7 the pairing.

    P: params.P.  prk: (4, 12), the proving key's X, Y, Z, K.  points: (n, 11, 12); r_e: (n, 72); responses: (n, 8)."""
    _ensure()
    n, arrays = _proofs(points, 11, r_e, responses, 8, challenge)
    X = _prk(prk, 4)
    head = (_p(_point(accumulator)), _p(_point(P)), _p(X), _p(key.pk_pc), _p(key.ptilde_pc))
    return _each("dgpu_accumulator_gt_non_membership_proofs_verify_each_g1", head, n, arrays, montgomery)


def non_membership_proofs_verify_batch(key, accumulator, P, prk, points, r_e, responses, challenge, random, montgomery=False):
    """True iff every proof verifies, by ONE G1 equation over all Schnorr checks (check j of proof i weighs random^(6 i + j)) and one pairing check against the
    GT product of the R_E_i^(random^i) (random non-zero modulo r; an empty batch verifies)"""
    _ensure()
    n, arrays = _proofs(points, 11, r_e, responses, 8, challenge)
    X = _prk(prk, 4)
    head = (_p(_point(accumulator)), _p(_point(P)), _p(X), _p(key.pk_pc), _p(key.ptilde_pc))
    return _batch("dgpu_accumulator_gt_non_membership_proofs_verify_batch_g1", head, n, arrays, random, montgomery)
