"""Mirror of the reference's smc_range_proof crate on the verifier's side, in bulk on the C ABI: BoundCheckSmc's two proofs over weak-BB signatures,
CLSRangeProof (cls_range_proof/range_proof_cdh.rs) and CCSArbitraryRangeProof (ccs_range_proof/arbitrary_range_cdh.rs), for n proofs of ONE statement.

    get_range_and_randomness_multiple, find_number_of_digits, find_sumset_boundaries (cls_range_proof/util.rs)    -> cls_statement(min, max, base, set_size)
    find_l_for_arbitrary_range, check_commitment_for_arbitrary_range's constants (ccs_range_proof/util.rs)        -> ccs_statement(min, max, base, set_size)
    CLSRangeProof::verify / CCSArbitraryRangeProof::verify, n times                                               -> verify_each(params, key, stmt, proofs)
    the same under one random linear combination                                                                  -> verify_batch(params, key, stmt, proofs, random)
    CLSRangeProof::challenge_contribution / CCSArbitraryRangeProof::challenge_contribution                        -> challenge_contribution(..)

A statement is (sides, l, weights, side_consts): sides 1 (CLS) or 2 (CCS: min, then max), l digits a side, the weights w_j of the digits' responses and per
side (a, b, e) with  a c C + (b c + sum_j w_j z2_j) g + e zr h = D.  Points are (12,) uint64 arrays of affine Montgomery limbs, zero words the identity; the
digits of a proof are side-major: all of min, then all of max.

These calls are served by libdock_gpu_smc.so (include/dock_gpu_smc.h), a library of its own beside the product with its own contexts: this module brings it up
on the product's device(s) when it is first used (crypto_amd._native.smc_lib)."""
import ctypes as C
import numpy as np
from ._native import smc_lib as lib, DockGpuError
from .msm import _ensure
from .fixed_base import _scalars_to_limbs, _p

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MAX_L = 64
STATUS = {0: "verified", 1: "InvalidRangeProof: the commitment equation of side detail - 1",
          2: "ShortGroupSig(InvalidProof): digit detail // 4 of the reference's order, check detail % 4 (1 A' is the identity, 2 the Schnorr check, 3 the pairing)",
          3: "the merged pairing check of the proof (verify_each with random)"}


def _check(min, max, base, set_size):
    """what both verifiers refuse before anything else: validate_base (UnsupportedBase) and min >= max (IncorrectBounds)"""
    min, max, base = int(min), int(max), int(base)
    if not (0 <= min < 1 << 64 and 0 <= max < 1 << 64 and 2 <= base < 1 << 16):
        raise ValueError("min, max are u64 and base a u16 of at least 2")
    if set_size is not None and int(set_size) < base:
        raise ValueError("UnsupportedBase(%d, %d)" % (base, set_size))
    if min >= max:
        raise ValueError("IncorrectBounds: min=%d should be < max=%d" % (min, max))
    return min, max, base


def range_and_randomness_multiple(base, min, max):
    """cls_range_proof/util.rs:15-27: (range, randomness_multiple) with range a multiple of base - 1"""
    rng, rm = max - min, 1
    if rng % (base - 1):
        rng, rm = rng * (base - 1), base - 1
    return rng, rm


def number_of_digits(rng, base):
    """util.rs:67-73: the least l with base^l >= rng + 1"""
    l = 0
    while base ** l < rng + 1:
        l += 1
    return l


def base_digits(value, base):
    out = []
    while value:
        out.append(value % base)
        value //= base
    return out


def sumset_boundaries(rng, base, num):
    """util.rs:77-93: the G_i of Theorem 2"""
    if base == 2:
        return [(rng + (1 << i)) >> (i + 1) for i in range(num)]
    h = base_digits(rng, base)
    h += [0] * (num - len(h))
    return [rng // base ** (i + 1) + (1 + h[i] + sum(h[:i]) % (base - 1)) // base for i in range(num)]


def decompose_for_sumset(value, G, base):
    """util.rs:96-113: the digits of value over the boundaries G, greedily from the first"""
    out = []
    for g in G:
        u = next((u for u in range(base - 1, 0, -1) if value >= g * u), 0)
        out.append(u)
        value -= g * u
    if value:
        raise ValueError("value outside the sumset")
    return out


def cls_statement(min, max, base, set_size=None):
    """(1, l, w, [(a, b, e)]) of CLSRangeProof::verify for min <= value < max: check_commitment (util.rs:29-64) works on (min, max - 1) —
    w = find_sumset_boundaries(range, base, l), a = -rm, b = min rm (a u128 product), e = rm"""
    min, max, base = _check(min, max, base, set_size)
    rng, rm = range_and_randomness_multiple(base, min, max - 1)
    l = number_of_digits(rng, base)
    return 1, l, [g % R for g in sumset_boundaries(rng, base, l)], [((R - rm) % R, min * rm % R, rm)]


def arbitrary_range_l(max, min, base):
    """ccs_range_proof/util.rs:70-78: the least l with max - min < base^l"""
    l = 0
    while base ** l <= max - min:
        l += 1
    return l


def ccs_statement(min, max, base, set_size=None):
    """(2, l, w, [(a, b, e) of min, of max]) of CCSArbitraryRangeProof::verify: w_j = base^j, a = -1, e = 1, b_min = min, b_max = -(base^l - max)
    (util.rs:6-49).  base^l is taken as an integer: where it reaches 2^64 (base 2 from max - min = 2^63 on) the reference's u64 power overflows on both
    the prover's and the verifier's side, and this is the statement its equations mean"""
    min, max, base = _check(min, max, base, set_size)
    l = arbitrary_range_l(max, min, base)
    return 2, l, [pow(base, j, R) for j in range(l)], [(R - 1, min % R, 1), (R - 1, (max - base ** l) % R, 1)]


class Params:
    """The verifier's half of SetMembershipCheckParamsWithPairing and the MemberCommitmentKey, prepared once: g1 of the weak-BB parameters, the coefficients of
    the public key and of g2, and the commitment key (g, h)"""

    def __init__(self, g1, g2, pk, ck_g, ck_h):
        from .pairing import G2Prepared
        _ensure()
        pc = G2Prepared.from_affine(np.stack([np.asarray(pk, dtype=np.uint64).reshape(24), np.asarray(g2, dtype=np.uint64).reshape(24)]))
        self.pk_pc, self.g2_pc = np.ascontiguousarray(pc.coeffs[0]), np.ascontiguousarray(pc.coeffs[1])
        self.g1, self.ck_g, self.ck_h = (np.ascontiguousarray(q, dtype=np.uint64).reshape(12).copy() for q in (g1, ck_g, ck_h))


class Proofs:
    """n proofs of one statement as arrays: commitments (n, 12), challenge n scalars, side_points (n, S, 12) the D, side_responses (n, S) the resp_r,
    digit_points (n, S, l, 3, 12) = A', Abar, T per digit and digit_responses (n, S, l, 2) = z1 (response1, over g1), z2 (response2, the digit's response).
    CCS proofs whose sides hold fewer than l digits are the reference's ProofShorterThanExpected; any other mismatch of the digit arrays with the
    statement's shape is a plain ValueError."""

    def __init__(self, stmt, commitments, challenge, side_points, side_responses, digit_points, digit_responses):
        S, l = stmt[0], stmt[1]
        self.commitments = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 12)
        n = self.n = len(self.commitments)
        sc = lambda v, k: (_scalars_to_limbs(v).reshape(-1, 4) if k else np.zeros((0, 4), np.uint64))
        self.challenge = sc(challenge, n)
        self.side_points = np.ascontiguousarray(side_points, dtype=np.uint64).reshape(-1, 12)
        self.side_responses = sc(side_responses, n)
        self.digit_points = np.ascontiguousarray(digit_points, dtype=np.uint64).reshape(-1, 12)
        self.digit_responses = sc(digit_responses, n * S * l)
        if len(self.digit_points) != 3 * n * S * l or len(self.digit_responses) != 2 * n * S * l:
            what = "%d digit points and %d responses for %d proofs of %d x %d digits" % (len(self.digit_points), len(self.digit_responses), n, S, l)
            # the reference's own error is for CCS sides that hold fewer than l digits (arbitrary_range_cdh.rs:327-337); anything else is a malformed call
            short = S == 2 and len(self.digit_points) <= 3 * n * S * l and len(self.digit_responses) <= 2 * n * S * l
            raise ValueError(("ProofShorterThanExpected: " if short else "the digit arrays do not have the statement's shape: ") + what)
        if not (len(self.challenge) == n and len(self.side_points) == n * S and len(self.side_responses) == n * S):
            raise ValueError("%d proofs: %d challenges, %d side points, %d side responses" % (n, len(self.challenge), len(self.side_points), len(self.side_responses)))


def _head(params, stmt, pr, montgomery):
    S, l, w, consts = stmt
    if S not in (1, 2) or len(consts) != S or len(w) != l or l > MAX_L:
        raise ValueError("a statement is (sides in {1, 2}, l <= 64, l weights, sides x (a, b, e))")
    form = (lambda v: [x * pow(2, 256, R) % R for x in v]) if montgomery else (lambda v: list(v))
    wl = _scalars_to_limbs(form(w)).reshape(-1, 4) if l else None
    cl = _scalars_to_limbs(form([x for t in consts for x in t])).reshape(-1, 4)
    opt = lambda a: _p(a) if a is not None and len(a) else None
    return [_p(params.g1), _p(params.ck_g), _p(params.ck_h), _p(params.pk_pc), _p(params.g2_pc), S, l, opt(wl), _p(cl), opt(pr.commitments), opt(pr.digit_points),
            opt(pr.digit_responses), opt(pr.side_points), opt(pr.side_responses), opt(pr.challenge), pr.n, 1 if montgomery else 0], (wl, cl)


def verify_each(params, stmt, proofs, random=None, montgomery=False):
    """(status, detail): two (n,) arrays, uint8 and int32 — 0, 0 where the reference's verify accepts proof i; 1, s + 1 where the commitment equation of side s
    fails (InvalidRangeProof); 2, 4 q + k where the digit at position q of the reference's order fails check k (STATUS).  The statement's constants are
    converted to the proofs' form.  random: n scalars in the proofs' form, non-zero modulo r — the merged form, verify_given_randomized_pairing_checker with
    one checker per proof: the proof's pairings become ONE two-pair check under the weights random_i^d, whose failure is 3, 0."""
    _ensure()
    head, keep = _head(params, stmt, proofs, montgomery)
    n = proofs.n
    status, detail = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    rnd = None if random is None else _scalars_to_limbs(random).reshape(-1, 4)
    rc = lib().dgpu_smc_range_proofs_verify_each_g1(*head, None if rnd is None else _p(rnd), _p(status) if n else None, _p(detail) if n else None)
    if rc:
        raise DockGpuError(rc, "dgpu_smc_range_proofs_verify_each_g1")
    return status, detail


def verify_batch(params, stmt, proofs, random, montgomery=False):
    """True iff every proof verifies, by ONE G1 equation and one two-pair pairing check over the random linear combination with the weights random^(i M + m)
    on equation m of proof i and random^(i S l + d) on the pairing of its digit d (random in the proofs' form, non-zero modulo r; an empty batch verifies; an
    identity A' anywhere refuses)"""
    _ensure()
    head, keep = _head(params, stmt, proofs, montgomery)
    rho = _scalars_to_limbs([random] if isinstance(random, int) else random).reshape(4)
    ok = C.c_int32(0)
    rc = lib().dgpu_smc_range_proofs_verify_batch_g1(*head, _p(rho), C.byref(ok))
    if rc:
        raise DockGpuError(rc, "dgpu_smc_range_proofs_verify_batch_g1")
    return bool(ok.value)


def challenge_contribution(params, stmt, commitment, side_points, digit_points):
    """The bytes CLSRangeProof::challenge_contribution (range_proof_cdh.rs:258-272) and CCSArbitraryRangeProof::challenge_contribution
    (arbitrary_range_cdh.rs:291-309) write for ONE proof: per digit, all of min then all of max, the weak-BB proof's Abar, A', g1, T
    (weak_bb_sig_pok_cdh.rs:129-141); then the commitment key g, h, the commitment and D (D_min, D_max), all compressed.  side_points: (S, 12);
    digit_points: (S l, 3, 12) = A', Abar, T.  Hashing the bytes to a challenge stays with the caller."""
    from . import serde
    from .msm import G1
    S, l = stmt[0], stmt[1]
    dp = np.ascontiguousarray(digit_points, dtype=np.uint64).reshape(S * l, 3, 12)
    sp = np.ascontiguousarray(side_points, dtype=np.uint64).reshape(S, 12)
    pts = [q for d in dp for q in (d[1], d[0], params.g1, d[2])] + [params.ck_g, params.ck_h, np.ascontiguousarray(commitment, dtype=np.uint64).reshape(12)] + list(sp)
    return serde.serialize(G1, np.stack(pts))
