"""CPU: the host-side contract of the two dgpu_bpp_* calls (include/dock_gpu_bpp.h, served by libdock_gpu_bpp.so and its development build, NOT by the product,
the SAVER or the SMC libraries) — what can be decided without a device: the header, crypto_amd/_native.py and the libraries' exports agree, the other six images
export none of the names, n = 0 is DGPU_OK with every pointer NULL and the empty batch verifies, every DGPU_E_BADARG case of the header that does not need a
handle answers so before the device is looked at (NULL pointers with n > 0, a base outside {2, 4, 8, 16}, num_bits that is no power of two in [log2 base, 64], m
that is no power of two in [1, 8], an NG that is no power of two, n = 2^31, a zero rho in either form), and a well-formed call is stopped by the missing device
only.  (A handle of the wrong length is DGPU_E_BADARG too, but a handle exists only where a device does: tests/test_gpu_bpp_range_proof.py.)  Also CPU: the Python
mirror's shape rules, its transcript order over both Merlin implementations, and commitments_to_values against the oracle."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import bpp_model as BM
from crypto_amd import _native
from crypto_amd._native import lib, dev_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
blib = lambda: _native.bpp_lib(bring_up=False)                   # libdock_gpu_bpp.so, not brought up on a device
bdev = lambda: _native._load(_native._BPP_DEV_SO)                # its development build

OK, NODEVICE, BADARG = 0, -1, -3
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
vp, sz, i32, u32, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_uint64
HEAD = [u64, u32, u32, u32] + [vp] * 5 + [sz, i32]
SIGNATURES = {"dgpu_bpp_range_proofs_verify_each_g1": HEAD + [vp], "dgpu_bpp_range_proofs_verify_batch_g1": HEAD + [vp, C.POINTER(i32)]}
NAMES = ["setup", "base", "num_bits", "m", "values", "round", "wnla", "l_n", "chal", "n", "mont"]
OTHERS = ("libdock_gpu.so", "libdock_gpu_dev.so", "libdock_gpu_saver.so", "libdock_gpu_saver_dev.so", "libdock_gpu_smc.so", "libdock_gpu_smc_dev.so")


def p_(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(v):
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], np.uint64)


def exported(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "crypto_amd", so)], text=True)
    return sorted(l.split()[-1] for l in out.splitlines() if " T dgpu_" in l)


def test_symbols_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "dock_gpu_bpp.h")).read()
    assert sorted(set(re.findall(r"\b(dgpu_bpp_[a-z0-9_]+)\s*\(", hdr))) == sorted(SIGNATURES) == sorted(_native.BPP_SYMBOLS)
    others = [lib(), dev_lib(), _native.saver_lib(bring_up=False), _native._load(_native._SAVER_DEV_SO), _native.smc_lib(bring_up=False), _native._load(_native._SMC_DEV_SO)]
    for name, args in SIGNATURES.items():
        assert name not in _native.SYMBOLS + _native.DEV_SYMBOLS + _native.SAVER_SYMBOLS + _native.SMC_SYMBOLS
        for other in others:
            assert not hasattr(other, name)
        for L in (blib(), bdev()):
            fn = getattr(L, name)
            assert fn.restype is C.c_int32 and fn.argtypes == args, name
    assert exported("libdock_gpu_bpp.so") == sorted(_native.SYMBOLS + _native.BPP_SYMBOLS)
    assert exported("libdock_gpu_bpp_dev.so") == sorted(_native.SYMBOLS + _native.BPP_SYMBOLS + _native.DEV_SYMBOLS)
    for so in OTHERS:
        assert not [s for s in exported(so) if "bpp" in s], so
    assert hasattr(bdev(), "dgpu_set_many_chunk_rows") and not hasattr(blib(), "dgpu_set_many_chunk_rows")      # the knob that cuts the chunks: the development build alone


class Args:
    def __init__(self, base=2, num_bits=8, m=1, n=2):
        s = BM.Shape(base, num_bits, m)
        one = lambda *shape: np.ones(shape, np.uint64)
        self.v = dict(setup=1, base=base, num_bits=num_bits, m=m, values=one(n * m, 12), round=one(n * 4, 12), wnla=one(n * 2 * s.K, 12), l_n=one(n * 2, 4),
                      chal=one(n * (7 + s.K), 4), n=n, mont=0)
        self.rho = limbs(5)
        self.status, self.ok = np.full(n, 9, np.uint8), C.c_int32(-7)

    def head(self, **kw):
        v = dict(self.v, **kw)
        return [p_(v[k]) if isinstance(v[k], np.ndarray) else v[k] for k in NAMES]

    def each(self, L, status=True, **kw):
        return L.dgpu_bpp_range_proofs_verify_each_g1(*self.head(**kw), p_(self.status) if status else None)

    def batch(self, L, rho=True, ok=True, **kw):
        return L.dgpu_bpp_range_proofs_verify_batch_g1(*self.head(**kw), (p_(self.rho) if rho is True else rho), C.byref(self.ok) if ok else None)


@pytest.mark.parametrize("L", [blib, bdev], ids=["bpp", "bpp-dev"])
def test_n_zero_needs_nothing(L):
    L = L()
    ok = C.c_int32(-7)
    nulls = [0, 0, 0, 0] + [None] * 5 + [0, 0]
    assert L.dgpu_bpp_range_proofs_verify_each_g1(*nulls, None) == OK
    assert L.dgpu_bpp_range_proofs_verify_batch_g1(*nulls, None, C.byref(ok)) == OK and ok.value == 1      # an empty batch verifies
    assert L.dgpu_bpp_range_proofs_verify_batch_g1(*nulls, None, None) == OK
    nulls[1], nulls[2], nulls[3] = 7, 1000, 99                                                              # ... before the shape is looked at
    assert L.dgpu_bpp_range_proofs_verify_each_g1(*nulls, None) == OK


@pytest.mark.parametrize("L", [blib, bdev], ids=["bpp", "bpp-dev"])
def test_bad_arguments_are_refused_before_the_device(L):
    L, a = L(), Args()
    for k in NAMES:
        if isinstance(a.v[k], np.ndarray):
            assert a.each(L, **{k: None}) == BADARG and a.batch(L, **{k: None}) == BADARG, k
    assert a.each(L, status=False) == BADARG and a.batch(L, rho=None) == BADARG and a.batch(L, ok=False) == BADARG
    for base in (0, 1, 3, 5, 6, 32, 64, 2 ** 16 + 2):
        assert a.each(L, base=base) == BADARG and a.batch(L, base=base) == BADARG, base
    for base, num_bits in ((2, 0), (2, 3), (2, 12), (2, 128), (4, 1), (16, 2), (16, 24), (8, 2), (8, 32), (8, 64)):      # (8, 32), (8, 64): 10 and 21 digits, NG no power of two
        assert a.each(L, base=base, num_bits=num_bits) == BADARG and a.batch(L, base=base, num_bits=num_bits) == BADARG, (base, num_bits)
    for m in (0, 3, 5, 6, 7, 16):
        assert a.each(L, m=m) == BADARG and a.batch(L, m=m) == BADARG, m
    assert a.each(L, n=2 ** 31) == BADARG and a.batch(L, n=2 ** 31) == BADARG
    for zero, mont in ((0, 0), (R, 0), (0, 1)):                              # rho = 0 mod r: canonical zero, r itself, and in the Montgomery form zero
        a.rho = limbs(zero)
        assert a.batch(L, mont=mont) == BADARG
    assert (a.status == 9).all() and a.ok.value == -7


@pytest.mark.parametrize("L", [blib, bdev], ids=["bpp", "bpp-dev"])
def test_a_well_formed_call_stops_at_the_missing_device(L):
    L = L()
    if L.dgpu_context_count() != 0:                                         # (the suite's CPU half never initialises a device; with one these calls would run)
        pytest.skip("this library is up on a device in this process: DGPU_E_NODEVICE cannot be observed")
    for shape in BM.SHAPES + [(8, 4, 1), (8, 16, 8), (2, 64, 8), (16, 4, 1)]:
        a = Args(*shape)
        assert a.each(L) == NODEVICE and a.batch(L) == NODEVICE and a.each(L, mont=1) == NODEVICE and a.batch(L, mont=1) == NODEVICE, shape
        assert a.each(L, setup=0) == NODEVICE                                # (the handle is looked up where it lives: behind the device)
    assert (a.status == 9).all() and a.ok.value == -7


# ---- the Python mirror, as far as the host goes -------------------------------------------------------------------------------------------------------
def test_shape_rules_of_the_mirror():
    from crypto_amd import bpp_range_proof as BRP
    for shape in BM.SHAPES:
        s = BM.Shape(*shape)
        assert BRP.num_g(*shape) == s.NG and BRP.rounds(*shape) == s.K
    assert BRP.num_g(2, 64, 2) == 128 and BRP.rounds(2, 64, 2) == 7          # proof_system's shape
    for bad in ((3, 8, 1), (32, 8, 1), (2, 12, 1), (2, 128, 1), (16, 2, 1), (2, 8, 3), (2, 8, 16), (8, 32, 1)):
        with pytest.raises(ValueError):
            BRP.num_g(*bad)


def test_challenges_over_both_transcripts_and_in_the_reference_order():
    """challenges() over the C transcript equals it over the Python one, and equals the order of range_proof.rs:86-131 and
    weighted_norm_linear_argument.rs:413-418 written out by hand here"""
    import oracle_c as O
    from crypto_amd import bpp_range_proof as BRP, serde
    from crypto_amd.msm import G1
    from crypto_amd.aggregation.transcript import MerlinTranscript, NativeMerlinTranscript, build_helper
    build_helper()
    K, m = 4, 2
    pts = O.G1.gen_seq(O.int_to_limbs(5, 4), O.int_to_limbs(7, 4), m + 4 + 2 * K, threads=2)
    proof = dict(V=pts[:m], D=pts[m], M=pts[m + 1], R=pts[m + 2], S=pts[m + 3], X=pts[m + 4:m + 4 + K], Rr=pts[m + 4 + K:], l0=1, n0=2)
    proof["X"] = proof["X"].copy()
    proof["X"][1] = 0                                                        # an identity among the points serializes as arkworks' infinity
    a = BRP.challenges(MerlinTranscript(b"BPP/tests"), 2, 8, proof)
    b = BRP.challenges(NativeMerlinTranscript(b"BPP/tests"), 2, 8, proof)
    assert a == b and len(a) == 7 + K and len(set(a)) == len(a)
    t = MerlinTranscript(b"BPP/tests")
    ser = lambda p: serde.serialize(G1, p.reshape(1, 12), np.array([0 if p.any() else 1], np.uint8))
    t.append_message(b"base", (2).to_bytes(2, "little")); t.append_message(b"num_bits", (8).to_bytes(2, "little"))
    for v in proof["V"]:
        t.append(b"V", ser(v))
    t.append(b"D", ser(proof["D"])); t.append(b"M", ser(proof["M"]))
    want = [t.challenge_scalar(b"e")]
    t.append(b"R", ser(proof["R"]))
    want += [t.challenge_scalar(l) for l in (b"x", b"y", b"r", b"lambda", b"delta")]
    t.append(b"S", ser(proof["S"]))
    want.append(t.challenge_scalar(b"t"))
    for j in range(K):
        t.append(b"X", ser(proof["X"][j])); t.append(b"R", ser(proof["Rr"][j]))
        want.append(t.challenge_scalar(b"gamma"))
    assert a == want
    assert BRP.challenges(MerlinTranscript(b"BPP/tests"), 2, 16, proof) != a and BRP.challenges(MerlinTranscript(b"other"), 2, 8, proof) != a


def test_commitments_to_values_against_the_oracle():
    import oracle_c as O
    from crypto_amd import bpp_range_proof as BRP
    G = O.G1
    g = G.generator()
    mul = lambda p, k: G.to_affine(G.mul(p, O.int_to_limbs(k % R, 4)))[0]
    bounds = [(0, 1), (5, 2 ** 64 - 1), (100, 101)]
    V = np.stack([mul(g, 11 + 3 * k) for k in range(6)])
    got = BRP.commitments_to_values(V, bounds, g)
    for i, (lo, hi) in enumerate(bounds):
        assert (got[i, 0] == mul(g, 11 + 6 * i + lo)).all(), i                       # V[2 i] + min g
        assert (got[i, 1] == mul(g, hi - 1 - (14 + 6 * i))).all(), i                 # (max - 1) g - V[2 i + 1]
    V[0] = 0                                                                         # the identity as a commitment; min = 0: the identity comes back
    assert not BRP.commitments_to_values(V, bounds, g)[0, 0].any()
    with pytest.raises(ValueError):
        BRP.commitments_to_values(V, [(3, 3), (0, 1), (0, 1)], g)
    with pytest.raises(ValueError):
        BRP.commitments_to_values(V, bounds[:2], g)
