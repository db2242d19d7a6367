"""Mirror of the accumulator manager's batch witness update (vb_accumulator/src/witness.rs:165-285) on the C ABI.

    Witness::compute_update_using_secret_key_after_batch_updates(additions, removals, elements, old_witnesses, old_accumulator, sk)
        -> update_witnesses(additions, removals, alpha, elements, witnesses, accumulator)     returns (d_factors, new_witnesses)
    ..._after_batch_additions / ..._after_batch_removals       -> the same call with `removals` / `additions` empty
    the factors alone (d_A / d_D and v_AD / d_D per element)   -> update_factors(additions, removals, alpha, elements)

    Omega::new(additions, removals, old_accumulator, sk)       -> omega(additions, removals, alpha, accumulator)               returns (points, identity_mask)
    Omega::new_for_kb_positive_accumulator(removals, V, sk)    -> omega([], members, alpha, -V)
    Witness::compute_update_using_public_info_after_batch_updates(additions, removals, omega, element, old_witness), for m holders at once (witness.rs:292-314)
        -> update_witnesses_public(additions, removals, omega, elements, witnesses)       returns (d_factors, new_witnesses, ok)

    UniversalAccumulator::compute_d_for_batch_given_members(non_members, members) (universal.rs:479-495)
        -> d_for_batch(members, non_members, d_in=None)                                    returns (d, nonzero); members may be resident (DeviceScalars)
    ...::compute_non_membership_witnesses_for_batch_given_d(d, non_members, sk, params_gen) (universal.rs:499-535)
        -> non_membership_witnesses(d, non_members, f_V, alpha, params_gen)               returns ((points, identity_mask), ok)
    ...::get_non_membership_witnesses_for_batch(non_members, sk, state, params_gen) (universal.rs:540-583)
        -> get_non_membership_witnesses_for_batch(members, non_members, f_V, alpha, params_gen)      returns (d, (points, identity_mask))
    PositiveAccumulator::compute_membership_witnesses_for_batch(members, sk) (positive.rs:369-381)
        -> membership_witnesses(members, alpha, accumulator)                                returns (points, identity_mask)

    MembershipProof::verify(V, challenge, pk, params), n times (vb_accumulator/src/proofs_cdh.rs:138-149)
        -> membership_proofs_verify_each(key, accumulator, points, responses, challenge)      returns status, one byte per proof
    the same with one verdict for all                          -> membership_proofs_verify_batch(.., random)       returns True / False
    NonMembershipProof::verify(V, challenge, pk, params, Q), n times (proofs_cdh.rs:365-387, :481-523)
        -> non_membership_proofs_verify_each(key, accumulator, P, Q, points, responses, challenge)
    the same with one verdict for all                          -> non_membership_proofs_verify_batch(.., random)
    proof.challenge_contribution(V, writer) / (V, params, Q, writer)
        -> membership_challenge_contribution(accumulator, proof_points) / non_membership_challenge_contribution(accumulator, P, Q, proof_points)     return bytes

Field elements are (n, 4) uint64 limb arrays or Python ints, canonical unless `montgomery=True` (then ark-ff Montgomery limbs in and out).  Witnesses
and the accumulator are G1 affine Montgomery limbs, (m, 12) and (12,) uint64; an identity is all-zero words.  New witnesses come back normalised
(G::Group::normalize_batch, witness.rs:284) as an (m, 12) array plus a uint8 identity mask: a holder whose element was removed gets d_factor = 0 and
the identity.
"""
import ctypes as C
import numpy as np
from ._native import lib, DockGpuError
from .msm import _ensure
from .fixed_base import _scalars_to_limbs, _p


def _limbs(values):
    s = _scalars_to_limbs(values) if len(values) else np.zeros((0, 4), np.uint64)
    return s, (_p(s) if len(s) else None)


def update_factors(additions, removals, alpha, elements, montgomery=False):
    """(f, g): f_i = d_A(y_i) / d_D(y_i) (the reference's d_factor), g_i = v_AD(y_i) / d_D(y_i), each an (m, 4) uint64 array"""
    _ensure()
    a, pa = _limbs(additions)
    r, pr = _limbs(removals)
    y, py = _limbs(elements)
    al = _scalars_to_limbs([alpha] if isinstance(alpha, int) else alpha).reshape(4)
    m = len(y)
    f, g = np.zeros((m, 4), np.uint64), np.zeros((m, 4), np.uint64)
    rc = lib().dgpu_accumulator_update_factors(pa, len(a), pr, len(r), _p(al), py, m, 1 if montgomery else 0, _p(f), _p(g))
    if rc:
        raise DockGpuError(rc, "dgpu_accumulator_update_factors")
    return f, g


def update_witnesses(additions, removals, alpha, elements, witnesses, accumulator, montgomery=False):
    """(d_factors, (new_witnesses, identity_mask)): C_i' = f_i C_i + g_i V for every holder"""
    _ensure()
    a, pa = _limbs(additions)
    r, pr = _limbs(removals)
    y, py = _limbs(elements)
    al = _scalars_to_limbs([alpha] if isinstance(alpha, int) else alpha).reshape(4)
    m = len(y)
    w = np.ascontiguousarray(witnesses, dtype=np.uint64).reshape(-1, 12)
    if len(w) != m:
        raise ValueError("NeedSameNoOfElementsAndWitnesses: %d elements, %d witnesses" % (m, len(w)))      # witness.rs:246-248
    v = np.ascontiguousarray(accumulator, dtype=np.uint64).reshape(12)
    d = np.zeros((m, 4), np.uint64)
    out = np.zeros((m, 12), np.uint64)
    inf = np.zeros(m, np.uint8)
    rc = lib().dgpu_accumulator_update_witnesses_g1(pa, len(a), pr, len(r), _p(al), py, _p(w) if m else None, m, _p(v), 1 if montgomery else 0, _p(d), _p(out), _p(inf))
    if rc:
        raise DockGpuError(rc, "dgpu_accumulator_update_witnesses_g1")
    return d, (out, inf)


def omega(additions, removals, alpha, accumulator, montgomery=False):
    """(points, identity_mask): omega_j = c_j V for the coefficients c_j of v_AD, trimmed like ark-poly trims the polynomial (trailing zero coefficients
    dropped: two empty lists, or the zero polynomial, give no entries); a zero coefficient below the last one is an identity entry"""
    _ensure()
    a, pa = _limbs(additions)
    r, pr = _limbs(removals)
    al = _scalars_to_limbs([alpha] if isinstance(alpha, int) else alpha).reshape(4)
    v = np.ascontiguousarray(accumulator, dtype=np.uint64).reshape(12)
    n = max(len(a), len(r))
    out = np.zeros((n, 12), np.uint64)
    inf = np.zeros(n, np.uint8)
    length = C.c_size_t(0)
    rc = lib().dgpu_accumulator_omega_g1(pa, len(a), pr, len(r), _p(al), _p(v), 1 if montgomery else 0, _p(out) if n else None, _p(inf) if n else None, C.byref(length))
    if rc:
        raise DockGpuError(rc, "dgpu_accumulator_omega_g1")
    return out[:length.value], inf[:length.value]


def update_witnesses_public(additions, removals, omega, elements, witnesses, montgomery=False):
    """(d_factors, (new_witnesses, identity_mask), ok) without the secret key: C_i' = f_i C_i + <s_i y_i^j, omega_j>.  `omega` is (points, identity_mask) as
    omega() returns it, or the points alone (an entry of zero words is an identity).  ok[i] = 0 marks a holder whose element was removed (the reference's
    CannotBeZero): d_factor 0 and the identity for that holder, everyone else unaffected"""
    _ensure()
    a, pa = _limbs(additions)
    r, pr = _limbs(removals)
    y, py = _limbs(elements)
    opts, oinf = omega if isinstance(omega, tuple) else (omega, None)
    o = np.ascontiguousarray(opts, dtype=np.uint64).reshape(-1, 12)
    oi = None if oinf is None else np.ascontiguousarray(oinf, dtype=np.uint8)
    if oi is not None and len(oi) != len(o):
        raise ValueError("omega: %d points, %d identity flags" % (len(o), len(oi)))
    m = len(y)
    w = np.ascontiguousarray(witnesses, dtype=np.uint64).reshape(-1, 12)
    if len(w) != m:
        raise ValueError("NeedSameNoOfElementsAndWitnesses: %d elements, %d witnesses" % (m, len(w)))
    d = np.zeros((m, 4), np.uint64)
    out = np.zeros((m, 12), np.uint64)
    inf = np.zeros(m, np.uint8)
    ok = np.zeros(m, np.uint8)
    rc = lib().dgpu_accumulator_update_witnesses_public_g1(pa, len(a), pr, len(r), _p(o) if len(o) else None, _p(oi) if oi is not None and len(oi) else None, len(o),
                                                           py, _p(w) if m else None, m, 1 if montgomery else 0, _p(d), _p(out), _p(inf), _p(ok))
    if rc:
        raise DockGpuError(rc, "dgpu_accumulator_update_witnesses_public_g1")
    return d, (out, inf), ok


def _alpha(alpha):
    return _scalars_to_limbs([alpha] if isinstance(alpha, int) else alpha).reshape(4)


def d_for_batch(members, non_members, d_in=None, montgomery=False, offset=0, n=None):
    """(d, nonzero): d_i = d_in_i prod_j (member_j - y_i) over all members, d_in = None meaning one; nonzero[i] = 0 marks a y_i that is a member.  `members`
    is an array / list, or a resident scalar vector (crypto_amd.DeviceScalars, or its handle with `n` given) of which the entries [offset, offset + n) are
    read where they lie; `montgomery` then speaks for non_members, d_in and d only.  Feeding the d of one partition of the members as the d_in of the next
    is the reference's partitioning (universal.rs:476-478)"""
    _ensure()
    y, py = _limbs(non_members)
    m = len(y)
    di = None
    if d_in is not None:
        di = _scalars_to_limbs(d_in)
        if len(di) != m:
            raise ValueError("d_in: %d entries for %d non-members" % (len(di), m))
    d = np.zeros((m, 4), np.uint64)
    nz = np.zeros(m, np.uint8)
    mont = 1 if montgomery else 0
    if hasattr(members, "handle") or isinstance(members, int):
        handle = members if isinstance(members, int) else members.handle
        if n is None:
            if isinstance(members, int):
                raise ValueError("a bare handle needs n")
            n = members.n - offset
        rc = lib().dgpu_accumulator_d_for_batch_resident(handle, offset, n, py, m, mont, _p(di), _p(d), _p(nz))
        name = "dgpu_accumulator_d_for_batch_resident"
    else:
        a, pa = _limbs(members)
        a = a[offset:offset + n] if n is not None else a[offset:]
        rc = lib().dgpu_accumulator_d_for_batch(_p(np.ascontiguousarray(a)) if len(a) else None, len(a), py, m, mont, _p(di), _p(d), _p(nz))
        name = "dgpu_accumulator_d_for_batch"
    if rc:
        raise DockGpuError(rc, name)
    return d, nz


def non_membership_witnesses(d, non_members, f_V, alpha, params_gen, montgomery=False):
    """((points, identity_mask), ok): C_i = ((f_V - d_i) / (y_i + alpha)) params_gen.  ok[i] = 0 marks a zero d_i (the reference's CannotBeZero): the identity for
    that entry, everyone else unaffected"""
    _ensure()
    y, py = _limbs(non_members)
    dd, pd = _limbs(d)
    m = len(y)
    if len(dd) != m:
        raise ValueError("%d non-members, %d values of d" % (m, len(dd)))
    fv = _alpha(f_V)
    al = _alpha(alpha)
    g = np.ascontiguousarray(params_gen, dtype=np.uint64).reshape(12)
    out, inf, ok = np.zeros((m, 12), np.uint64), np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    rc = lib().dgpu_accumulator_non_membership_witnesses_g1(pd, py, m, _p(fv), _p(al), _p(g), 1 if montgomery else 0, _p(out), _p(inf), _p(ok))
    if rc:
        raise DockGpuError(rc, "dgpu_accumulator_non_membership_witnesses_g1")
    return (out, inf), ok


def membership_witnesses(members, alpha, accumulator, montgomery=False):
    """(points, identity_mask): C_i = (1 / (y_i + alpha)) V"""
    _ensure()
    y, py = _limbs(members)
    m = len(y)
    al = _alpha(alpha)
    v = np.ascontiguousarray(accumulator, dtype=np.uint64).reshape(12)
    out, inf = np.zeros((m, 12), np.uint64), np.zeros(m, np.uint8)
    rc = lib().dgpu_accumulator_membership_witnesses_g1(py, m, _p(al), _p(v), 1 if montgomery else 0, _p(out), _p(inf))
    if rc:
        raise DockGpuError(rc, "dgpu_accumulator_membership_witnesses_g1")
    return out, inf


def get_non_membership_witnesses_for_batch(members, non_members, f_V, alpha, params_gen, montgomery=False):
    """(d, (points, identity_mask)): the two calls in a row, as the reference does (universal.rs:540-583).  Raises ValueError("CannotBeZero") when a
    non-member is a member (the reference answers ElementPresent from its state, or CannotBeZero from the product)"""
    d, nz = d_for_batch(members, non_members, montgomery=montgomery)
    if not nz.all():
        raise ValueError("CannotBeZero")
    wits, ok = non_membership_witnesses(d, non_members, f_V, alpha, params_gen, montgomery=montgomery)
    if not ok.all():
        raise ValueError("CannotBeZero")
    return d, wits


# ---- the CDH proofs of membership and non-membership in bulk (vb_accumulator/src/proofs_cdh.rs) ------------------------------------------------------------
MEMBERSHIP_STATUS = {0: "verified", 1: "InvalidProof: A' is the identity", 2: "InvalidProof: the Schnorr check", 3: "InvalidProof: the pairing"}
NON_MEMBERSHIP_STATUS = {0: "verified", 1: "CannotBeZero: C' is the identity", 2: "CannotBeZero: J is the identity", 3: "IncorrectRandomizedWitness: J over Q",
                         4: "SchnorrError(InvalidResponse)", 5: "IncorrectRandomizedWitness: the pairing"}


class VerifierKey:
    """The verifier's half of an accumulator key, prepared once: the coefficients of pk = alpha P~ and of P~ (SetupParams.P_tilde), as bbs_plus.Params holds
    those of w and g2."""

    def __init__(self, pk, p_tilde):
        from .pairing import G2Prepared
        _ensure()
        pc = G2Prepared.from_affine(np.stack([np.asarray(pk, dtype=np.uint64).reshape(24), np.asarray(p_tilde, dtype=np.uint64).reshape(24)]))
        self.pk_pc, self.ptilde_pc = np.ascontiguousarray(pc.coeffs[0]), np.ascontiguousarray(pc.coeffs[1])


def _point(p):
    return np.ascontiguousarray(p, dtype=np.uint64).reshape(12)


def _acc_proofs(points, npts, responses, nresp, challenge):
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, npts, 12)
    n = len(pts)
    flat = responses if isinstance(responses, np.ndarray) and responses.dtype == np.uint64 else [z for r in responses for z in r]
    resp = _scalars_to_limbs(flat).reshape(-1, nresp, 4) if n else np.zeros((0, nresp, 4), np.uint64)
    c = _scalars_to_limbs(challenge) if n else np.zeros((0, 4), np.uint64)
    if not (len(resp) == len(c) == n):
        raise ValueError("%d proofs' points, %d rows of responses, %d challenges" % (n, len(resp), len(c)))
    return n, pts, resp, c


def _each(name, head, n, pts, resp, c, montgomery):
    status = np.zeros(n, np.uint8)
    rc = getattr(lib(), name)(*head, _p(pts) if n else None, _p(resp) if n else None, _p(c) if n else None, n, 1 if montgomery else 0, _p(status) if n else None)
    if rc:
        raise DockGpuError(rc, name)
    return status


def _batch(name, head, n, pts, resp, c, random, montgomery):
    rho = _scalars_to_limbs([random] if isinstance(random, int) else random).reshape(4)
    ok = C.c_int32(0)
    rc = getattr(lib(), name)(*head, _p(pts) if n else None, _p(resp) if n else None, _p(c) if n else None, n, 1 if montgomery else 0, _p(rho), C.byref(ok))
    if rc:
        raise DockGpuError(rc, name)
    return bool(ok.value)


def membership_proofs_verify_each(key, accumulator, points, responses, challenge, montgomery=False):
    """status, an (n,) uint8 array: 0 where MembershipProof::verify accepts proof i against the accumulator value V, else the first failing check in the
    reference's order (MEMBERSHIP_STATUS): 1 A' is the identity, 2 z1 V - z2 A' - c Abar = T, 3 e(A', pk) e(-Abar, P~) = 1.

    points: (n, 3, 12), A', Abar, T (sc.t).  responses: (n, 2) scalars z1 (response1, over V) and z2 (response2, over -A'; for a partial proof the caller
    writes resp_for_element there).  The points are taken as validated members of the subgroup, as the reference takes them (crypto_amd.serde.validate)."""
    _ensure()
    n, pts, resp, c = _acc_proofs(points, 3, responses, 2, challenge)
    return _each("dgpu_accumulator_membership_proofs_verify_each_g1", (_p(_point(accumulator)), _p(key.pk_pc), _p(key.ptilde_pc)), n, pts, resp, c, montgomery)


def membership_proofs_verify_batch(key, accumulator, points, responses, challenge, random, montgomery=False):
    """True iff every proof verifies, by ONE G1 equation and one pairing check over the random linear combination with the weights random^i (random non-zero
    modulo r; an empty batch verifies; an identity A' anywhere refuses)"""
    _ensure()
    n, pts, resp, c = _acc_proofs(points, 3, responses, 2, challenge)
    return _batch("dgpu_accumulator_membership_proofs_verify_batch_g1", (_p(_point(accumulator)), _p(key.pk_pc), _p(key.ptilde_pc)), n, pts, resp, c, random, montgomery)


def non_membership_proofs_verify_each(key, accumulator, P, Q, points, responses, challenge, montgomery=False):
    """status, an (n,) uint8 array: 0 where NonMembershipProof::verify accepts proof i, else the first failing check in the reference's order
    (NON_MEMBERSHIP_STATUS): 1 C' is the identity, 2 J is, 3 s_d Q - c J = T2, 4 s_r V - s_y C' - s_d P - c Cbar = T1, 5 e(C', pk) e(-Cbar, P~) = 1.

    P: params.P; Q: the second generator.  points: (n, 5, 12), C', Cbar, J, T1 (t_1), T2 (sc_2.t).  responses: (n, 3) scalars s_r, s_y (responses 0 and 1 of
    sc_resp_1; for a partial proof the caller writes resp_for_element into s_y) and s_d (sc_2.response)."""
    _ensure()
    n, pts, resp, c = _acc_proofs(points, 5, responses, 3, challenge)
    head = (_p(_point(accumulator)), _p(_point(P)), _p(_point(Q)), _p(key.pk_pc), _p(key.ptilde_pc))
    return _each("dgpu_accumulator_non_membership_proofs_verify_each_g1", head, n, pts, resp, c, montgomery)


def non_membership_proofs_verify_batch(key, accumulator, P, Q, points, responses, challenge, random, montgomery=False):
    """True iff every proof verifies, by ONE G1 equation and one pairing check: the weights random^(2i) on check 4 of proof i, random^(2i+1) on check 3,
    random^i on the pairing (random non-zero modulo r; an empty batch verifies; an identity C' or J anywhere refuses)"""
    _ensure()
    n, pts, resp, c = _acc_proofs(points, 5, responses, 3, challenge)
    head = (_p(_point(accumulator)), _p(_point(P)), _p(_point(Q)), _p(key.pk_pc), _p(key.ptilde_pc))
    return _batch("dgpu_accumulator_non_membership_proofs_verify_batch_g1", head, n, pts, resp, c, random, montgomery)


def membership_challenge_contribution(accumulator, proof_points):
    """The bytes PoKOfSignatureG1Protocol::compute_challenge_contribution writes for one membership proof (short_group_sig/src/weak_bb_sig_pok_cdh.rs:129-141):
    Abar, A', V, T compressed.  proof_points: (3, 12) = A', Abar, T.  Hashing the bytes to a challenge stays with the caller."""
    from . import serde
    from .msm import G1
    Q = np.ascontiguousarray(proof_points, dtype=np.uint64).reshape(3, 12)
    return serde.serialize(G1, np.stack([Q[1], Q[0], _point(accumulator), Q[2]]))


def non_membership_challenge_contribution(accumulator, P, Q, proof_points):
    """The bytes NonMembershipProofProtocol::compute_challenge_contribution writes for one proof (proofs_cdh.rs:326-346): Cbar, C', J, V, P, Q, T1, T2
    compressed.  proof_points: (5, 12) = C', Cbar, J, T1, T2."""
    from . import serde
    from .msm import G1
    W = np.ascontiguousarray(proof_points, dtype=np.uint64).reshape(5, 12)
    return serde.serialize(G1, np.stack([W[1], W[0], W[2], _point(accumulator), _point(P), _point(Q), W[3], W[4]]))
