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
