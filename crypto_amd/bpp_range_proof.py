"""Mirror of the reference's bulletproofs_plus_plus crate on the verifier's side, in bulk on the C ABI: BoundCheckBpp's proof, ProofArbitraryRange over
Proof::verify (range_proof.rs:773-873) and the weighted-norm linear argument (weighted_norm_linear_argument.rs:213-238, :380-453), for n proofs of ONE shape
(base, num_bits, m values a proof) over ONE setup.

    SetupParams::get_no_of_G (setup.rs:114-116)                                        -> num_g(base, num_bits, m)
    SetupParams { G, G_vec, H_vec } resident on the device                             -> setup_handle(G, G_vec, H_vec)
    Round1Commitments::challenge, Round2Commitments::challenges, Round3Commitments::challenge (range_proof.rs:86-131) and the argument's gammas
    (weighted_norm_linear_argument.rs:413-418)                                         -> challenges(transcript, base, num_bits, proof)
    Proof::verify, n times                                                             -> verify_each(setup, base, num_bits, proofs, challenges)
    the same under one random linear combination                                       -> verify_batch(setup, base, num_bits, proofs, challenges, random)
    get_commitments_to_values_given_transformed_commitments_and_g (range_proof_arbitrary_range.rs:148-172)    -> commitments_to_values(V, bounds, g)

A proof is a dict (or any object with these attributes) of V (m, 12), D, M, R, S (12,), X (K, 12), Rr (K, 12) — the argument's X and R — and the scalars l0, n0;
points are uint64 arrays of affine Montgomery limbs, zero words the identity.  The challenges are INPUTS of the calls, as in proof_system, where the transcript
is shared with the other statements of a presentation: challenges() derives them for a proof that stands alone.

These calls are served by libdock_gpu_bpp.so (include/dock_gpu_bpp.h), a library of its own beside the product with its own contexts: this module brings it up
on the product's device(s) when it is first used (crypto_amd._native.bpp_lib)."""
import ctypes as C
import numpy as np
from ._native import bpp_lib as lib, DockGpuError
from .msm import _ensure, G1
from .fixed_base import _scalars_to_limbs, _p

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_H = 8
STATUS = {0: "verified", 1: "WeightedNormLinearArgumentVerificationFailed", 2: "one of t, r, e + k (k < base) is zero: the reference unwrap()s an inverse there"}


def _shape(base, num_bits, m):
    base, num_bits, m = int(base), int(num_bits), int(m)
    pow2 = lambda v: v > 0 and v & (v - 1) == 0
    if base not in (2, 4, 8, 16):
        raise ValueError("base is one of 2, 4, 8, 16")
    bb = base.bit_length() - 1
    if not pow2(num_bits) or not bb <= num_bits <= 64:
        raise ValueError("num_bits is a power of two in [%d, 64]" % bb)
    if not pow2(m) or m > 8:
        raise ValueError("1, 2, 4 or 8 values a proof")
    NG = max(num_bits // bb, base) * m
    if not pow2(NG):
        raise ValueError("ExpectedPowerOfTwo: %d generators" % NG)
    return NG, max(3, NG.bit_length() - 1)


def num_g(base, num_bits, m):
    """SetupParams::get_no_of_G: max(num_bits / log2 base, base) m"""
    return _shape(base, num_bits, m)[0]


def rounds(base, num_bits, m):
    """the rounds K of the weighted-norm linear argument: X and R hold K points each"""
    return _shape(base, num_bits, m)[1]


class Setup:
    """SetupParams on the device: a plain G1 bases handle holding [G, H_0 .. H_7, G_0 ..] in the library that serves the calls.  free() (or leaving a `with`
    block) releases it."""

    def __init__(self, G, G_vec, H_vec):
        _ensure()
        g_vec = np.ascontiguousarray(G_vec, dtype=np.uint64).reshape(-1, 12)
        h_vec = np.ascontiguousarray(H_vec, dtype=np.uint64).reshape(-1, 12)
        if len(h_vec) != N_H:
            raise ValueError("H_vec holds %d points" % N_H)
        self.points = np.ascontiguousarray(np.concatenate([np.asarray(G, dtype=np.uint64).reshape(1, 12), h_vec, g_vec]))
        self.n_g = len(g_vec)
        self._L = lib()
        h = C.c_uint64(0)
        rc = self._L.dgpu_bases_upload_g1(_p(self.points), None, len(self.points), C.byref(h))
        if rc:
            raise DockGpuError(rc, "dgpu_bases_upload_g1")
        self.handle = h.value

    def free(self):
        if self.handle:
            self._L.dgpu_bases_free(self.handle)
            self.handle = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


def setup_handle(G, G_vec, H_vec):
    return Setup(G, G_vec, H_vec)


def _get(proof, name):
    return proof[name] if isinstance(proof, dict) else getattr(proof, name)


def _ser(point):
    from . import serde
    p = np.ascontiguousarray(point, dtype=np.uint64).reshape(1, 12)
    return serde.serialize(G1, p, np.array([0 if p.any() else 1], np.uint8))


def challenges(transcript, base, num_bits, proof):
    """[e, x, y, r, lambda, delta, t, gamma_0 .. gamma_(K-1)] as integers, in the order the calls take them, from a MerlinTranscript or NativeMerlinTranscript
    (crypto_amd.aggregation.transcript) in the state the reference's verifier would find it in: base and num_bits as u16 LE, every V, D, M -> e; R -> x, y, r,
    lambda, delta; S -> t; per round X_j, R_j -> gamma_j.  Points go in as their compressed serialization."""
    V = np.ascontiguousarray(_get(proof, "V"), dtype=np.uint64).reshape(-1, 12)
    X = np.ascontiguousarray(_get(proof, "X"), dtype=np.uint64).reshape(-1, 12)
    Rr = np.ascontiguousarray(_get(proof, "Rr"), dtype=np.uint64).reshape(-1, 12)
    if len(X) != len(Rr):
        raise ValueError("UnexpectedLengthOfVectors: length of X=%d not equal to length of R=%d" % (len(X), len(Rr)))
    t = transcript
    t.append_message(b"base", int(base).to_bytes(2, "little"))
    t.append_message(b"num_bits", int(num_bits).to_bytes(2, "little"))
    for v in V:
        t.append(b"V", _ser(v))
    t.append(b"D", _ser(_get(proof, "D")))
    t.append(b"M", _ser(_get(proof, "M")))
    out = [t.challenge_scalar(b"e")]
    t.append(b"R", _ser(_get(proof, "R")))
    out += [t.challenge_scalar(l) for l in (b"x", b"y", b"r", b"lambda", b"delta")]
    t.append(b"S", _ser(_get(proof, "S")))
    out.append(t.challenge_scalar(b"t"))
    for x, r in zip(X, Rr):
        t.append(b"X", _ser(x))
        t.append(b"R", _ser(r))
        out.append(t.challenge_scalar(b"gamma"))
    return out


class Proofs:
    """n proofs of one shape as arrays: values (n, m, 12), round_points (n, 4, 12) = D, M, R, S, wnla_points (n, 2 K, 12) = X_0 .., R_0 .., l_n (n, 2) = l0, n0 and
    challenges (n, 7 + K) — scalars as Python integers or as (.., 4) uint64 limbs, in the form the call is told (montgomery)."""

    def __init__(self, base, num_bits, m, values, round_points, wnla_points, l_n, challenges):
        self.base, self.num_bits, self.m = int(base), int(num_bits), int(m)
        self.NG, self.K = _shape(base, num_bits, m)
        self.values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 12)
        n = self.n = len(self.values) // self.m
        def sc(v, k):                  # (n, 4) uint64 limbs as they are, else Python integers
            if isinstance(v, np.ndarray) and v.dtype == np.uint64:
                return np.ascontiguousarray(v).reshape(-1, 4)
            return _scalars_to_limbs([int(x) for x in np.asarray(v, dtype=object).reshape(-1)]).reshape(-1, 4) if k else np.zeros((0, 4), np.uint64)
        self.round_points = np.ascontiguousarray(round_points, dtype=np.uint64).reshape(-1, 12)
        self.wnla_points = np.ascontiguousarray(wnla_points, dtype=np.uint64).reshape(-1, 12)
        self.l_n = sc(l_n, n)
        self.challenges = sc(challenges, n)
        if not (len(self.values) == n * self.m and len(self.round_points) == 4 * n and len(self.wnla_points) == 2 * self.K * n and len(self.l_n) == 2 * n and
                len(self.challenges) == (7 + self.K) * n):
            raise ValueError("%d proofs of %d values and %d rounds: %d values, %d round points, %d argument points, %d of l and n, %d challenges"
                             % (n, self.m, self.K, len(self.values), len(self.round_points), len(self.wnla_points), len(self.l_n), len(self.challenges)))

    @classmethod
    def pack(cls, base, num_bits, proofs, challenges):
        """from a list of proofs (dicts or objects, see the module's head) and their challenges (n lists of 7 + K integers)"""
        m = len(np.asarray(_get(proofs[0], "V")).reshape(-1, 12)) if len(proofs) else 1
        cat = lambda rows: np.concatenate([np.asarray(r, dtype=np.uint64).reshape(-1, 12) for r in rows]) if len(rows) else np.zeros((0, 12), np.uint64)
        return cls(base, num_bits, m, cat([_get(p, "V") for p in proofs]), cat([_get(p, k) for p in proofs for k in ("D", "M", "R", "S")]),
                   cat([_get(p, k) for p in proofs for k in ("X", "Rr")]), [int(_get(p, k)) for p in proofs for k in ("l0", "n0")], [int(c) for row in challenges for c in row])


def _as_proofs(base, num_bits, proofs, challenges):
    return proofs if isinstance(proofs, Proofs) else Proofs.pack(base, num_bits, proofs, challenges)


def _head(setup, pr, montgomery):
    opt = lambda a: _p(a) if len(a) else None
    return [setup.handle, pr.base, pr.num_bits, pr.m, opt(pr.values), opt(pr.round_points), opt(pr.wnla_points), opt(pr.l_n), opt(pr.challenges), pr.n, 1 if montgomery else 0]


def verify_each(setup, base, num_bits, proofs, challenges=None, montgomery=False):
    """(n,) uint8 statuses (STATUS): 0 where the reference's verify accepts proof i under its challenges, 1 where the equation fails, 2 where an inverse does not
    exist.  proofs: a Proofs, or a list of proofs with `challenges` their n lists"""
    _ensure()
    pr = _as_proofs(base, num_bits, proofs, challenges)
    status = np.zeros(pr.n, np.uint8)
    rc = setup._L.dgpu_bpp_range_proofs_verify_each_g1(*_head(setup, pr, montgomery), _p(status) if pr.n else None)
    if rc:
        raise DockGpuError(rc, "dgpu_bpp_range_proofs_verify_each_g1")
    return status


def verify_batch(setup, base, num_bits, proofs, challenges=None, random=1, montgomery=False):
    """True iff every proof verifies, by ONE equation: proof i weighed by random^i (random in the proofs' form, non-zero modulo r — uniform, from the verifier's own
    randomness: an invalid batch passes with probability at most (n - 1) / r; random = 1 lets errors that cancel between proofs through).  An empty batch verifies"""
    _ensure()
    pr = _as_proofs(base, num_bits, proofs, challenges)
    rho = _scalars_to_limbs([random] if isinstance(random, int) else random).reshape(4)
    ok = C.c_int32(0)
    rc = setup._L.dgpu_bpp_range_proofs_verify_batch_g1(*_head(setup, pr, montgomery), _p(rho), C.byref(ok))
    if rc:
        raise DockGpuError(rc, "dgpu_bpp_range_proofs_verify_batch_g1")
    return bool(ok.value)


# ---- host arithmetic of commitments_to_values: affine G1 over Python integers (y^2 = x^3 + 4); None is the identity ----
_P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
_RQ, _RQI = pow(2, 384, _P), pow(pow(2, 384, _P), _P - 2, _P)


def _from_words(w):
    w = np.ascontiguousarray(w, dtype=np.uint64).reshape(12)
    if not w.any():
        return None
    f = lambda h: sum(int(v) << (64 * k) for k, v in enumerate(h)) * _RQI % _P
    return f(w[:6]), f(w[6:])


def _to_words(pt):
    if pt is None:
        return np.zeros(12, np.uint64)
    return np.array([(c * _RQ % _P) >> (64 * k) & 0xFFFFFFFFFFFFFFFF for c in pt for k in range(6)], dtype=np.uint64)


def _add(a, b):
    if a is None or b is None:
        return b if a is None else a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if (y1 + y2) % _P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, _P - 2, _P) % _P
    else:
        lam = (y2 - y1) * pow(x2 - x1, _P - 2, _P) % _P
    x3 = (lam * lam - x1 - x2) % _P
    return x3, (lam * (x1 - x3) - y1) % _P


def _mul(a, k):
    out = None
    for bit in bin(k)[2:] if k else "":
        out = _add(out, out)
        if bit == "1":
            out = _add(out, a)
    return out


def _neg(a):
    return None if a is None else (a[0], -a[1] % _P)


def commitments_to_values(V, bounds, g):
    """get_commitments_to_values_given_transformed_commitments_and_g: V holds per bound (min, max) a commitment to value - min and one to max - 1 - value;
    returns per bound the two commitments to the value itself, V[2 i] + min g and (max - 1) g - V[2 i + 1], as a (len(bounds), 2, 12) array.  Host arithmetic
    over Python integers, as the reference does it on the host: a presentation holds a handful of bounds"""
    V = np.ascontiguousarray(V, dtype=np.uint64).reshape(-1, 12)
    if len(V) != 2 * len(bounds):
        raise ValueError("IncorrectNumberOfCommitments(%d, %d)" % (len(bounds), len(V) // 2))
    gp = _from_words(g)
    out = np.zeros((len(bounds), 2, 12), np.uint64)
    for i, (lo, hi) in enumerate(bounds):
        lo, hi = int(lo), int(hi)
        if hi <= lo:
            raise ValueError("IncorrectBounds: max=%d should be > min=%d" % (hi, lo))
        out[i, 0] = _to_words(_add(_from_words(V[2 * i]), _mul(gp, lo)))
        out[i, 1] = _to_words(_add(_mul(gp, hi - 1), _neg(_from_words(V[2 * i + 1]))))
    return out
