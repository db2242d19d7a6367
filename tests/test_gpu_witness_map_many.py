"""GPU (-m gpu): dgpu_witness_map_r1cs_many — the witness maps of one resident circuit over many assignments in one call (crypto_amd/csrc/
wm_block_kernels.hip.h: a statement's a, b, c stay in one block's LDS from the sparse rows to the h scalars; domains above 2^10 run row by row inside the
call).  Bar: bytes.  Every row equals the single call dgpu_witness_map_r1cs on that row and the CPU oracle, at every domain where the path or the
rows per block change, across chunk and block boundaries, with every flag and output form."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import wm_many_circuits as W
import crypto_amd as ca
from crypto_amd import qap
from crypto_amd._native import lib, twin

pytestmark = pytest.mark.gpu
BADARG = -3
M_MAX = 65


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    ca.init(0)
    lib().dgpu_set_min_gpu_n(0)
    yield
    lib().dgpu_set_min_gpu_n(0)


def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_CASES = {}


def case(logn):
    """per domain, built once: the circuit (one past a power of two for even exponents, filling the domain for odd ones), 65 rows (satisfying, not
    satisfying, zero), the oracle's h for them"""
    if logn not in _CASES:
        circ = W.fill_exact(900 + logn, logn) if logn & 1 else W.one_past(900 + logn, logn)
        assert circ.logn == logn
        rows = W.rows_for(circ, M_MAX, 950 + logn, kinds=("sat", "rand", "rand", "zero", "rand"))
        _CASES[logn] = (circ, rows, W.oracle_h(circ, rows))
    return _CASES[logn]


def upload(circ):
    return qap.DeviceR1cs(*circ.mats, circ.num_vars, circ.num_inputs, circ.num_constraints)


def many(dev, circ, z, m, montgomery=0, stride=None, host=True, resident=False):
    out = np.zeros((m, circ.D, 4), dtype=np.uint64) if host else None
    h, n = C.c_uint64(0), C.c_size_t(0)
    rc = lib().dgpu_witness_map_r1cs_many(dev.handle, p_(z), stride or circ.num_vars, circ.num_vars, m, montgomery, p_(out), C.byref(h) if resident else None, C.byref(n))
    assert rc == 0, rc
    assert n.value == circ.D
    return (out, h.value) if resident else out


def singles(dev, circ, z, m, montgomery=0):
    out = np.zeros((m, circ.D, 4), dtype=np.uint64)
    for j in range(m):
        zj = np.ascontiguousarray(z[j])
        assert lib().dgpu_witness_map_r1cs(dev.handle, p_(zj), circ.num_vars, montgomery, p_(out[j]), None, None) == 0
    return out


@pytest.mark.parametrize("logn", [1, 2, 3, 7, 8, 9, 10, 11])
def test_rows_equal_the_single_call_and_the_oracle(logn):
    """D = 2, 4, 8, 128 | 256 (rows per block changes), 512, 1024 (the last fused size), 2048 (the row-by-row path); m = 1, 2, 3, 65"""
    circ, rows, want = case(logn)
    dev = upload(circ)
    ref = singles(dev, circ, rows, M_MAX)
    assert (ref == want).all()
    for m in (1, 2, 3, M_MAX):
        got = many(dev, circ, rows, m)
        assert (got == want[:m]).all() and (got == ref[:m]).all(), "D = %d, m = %d" % (circ.D, m)
    dev.free()


def test_chunk_boundaries_and_every_rows_per_block():
    """chunks of 4 rows with m = 9 (two boundaries, a tail of one), at every rows-per-block setting a domain of 8 and of 256 elements admits"""
    with twin() as T:
        try:
            for logn, settings in ((3, range(1, 129)), (8, range(1, 5))):
                circ, rows, want = case(logn)
                dev = upload(circ)
                for rpb in settings:
                    assert T.dgpu_set_wm_many(4, rpb) == 0
                    assert (many(dev, circ, rows, 9) == want[:9]).all(), "D = %d, %d rows per block" % (circ.D, rpb)
                assert T.dgpu_set_wm_many(4, 512) == 0           # more than the block holds: clamped
                assert (many(dev, circ, rows, 9) == want[:9]).all()
                dev.free()
        finally:
            T.dgpu_set_wm_many(0, 0)


@pytest.mark.parametrize("logn", [5, 9, 11])
def test_row_stride_and_both_montgomery_flags(logn):
    """rows further apart than num_vars, the gap filled with words that set bit 255: neither read nor refused; inputs as Fr limbs; h as Fr limbs"""
    circ, rows, want = case(logn)
    m, nv = 5, circ.num_vars
    wide = np.full((m, nv + 3, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    wide[:, :nv] = rows[:m]
    dev = upload(circ)
    assert (many(dev, circ, wide, m, stride=nv + 3) == want[:m]).all()
    assert (many(dev, circ, rows, m, montgomery=2) == O.fr_to_mont(want[:m])).all()
    assert (many(dev, circ, rows, m, montgomery=2) == singles(dev, circ, rows, m, montgomery=2)).all()
    dev.free()
    mont_mats = [(rp, cl, O.fr_to_mont(vl)) for rp, cl, vl in circ.mats]
    devm = qap.DeviceR1cs(*mont_mats, nv, circ.num_inputs, circ.num_constraints, montgomery=True)
    wide[:, :nv] = O.fr_to_mont(rows[:m])
    assert (many(devm, circ, wide, m, montgomery=1, stride=nv + 3) == want[:m]).all()
    assert (many(devm, circ, wide, m, montgomery=3, stride=nv + 3) == O.fr_to_mont(want[:m])).all()
    # the Python surface takes the strided view as it is
    h, _ = qap.witness_map_many(devm, wide[:, :nv], montgomery=True)
    assert (h == want[:m]).all()
    devm.free()


@pytest.mark.parametrize("logn", [9, 11])
def test_resident_vector_alone_and_with_the_host_copy(logn):
    """out_handle only: one vector of m * D canonical scalars, row j at scalar offset j * D (a row copied out with dgpu_scalars_copy_range multiplies like
    the oracle's row); out_h and out_handle together, also with h as Fr limbs on the host (the resident vector stays canonical)"""
    circ, rows, want = case(logn)
    m, D = 3, circ.D
    dev = upload(circ)
    bases = U.seq_bases(O.G1, D, 41, threads=16)[0]
    db = ca.DeviceBases(ca.G1, bases)
    L = lib()

    def check_resident(handle):
        ln = C.c_size_t(0)
        assert L.dgpu_handle_len(handle, C.byref(ln)) == 0 and ln.value == m * D
        for j in (0, m - 1):
            hj = C.c_uint64(0)
            assert L.dgpu_scalars_copy_range(handle, j * D, (j + 1) * D, 0, C.byref(hj)) == 0
            out = np.zeros(18, np.uint64)
            assert L.dgpu_msm_g1_resident(db.handle, 0, hj.value, 0, D, p_(out)) == 0
            assert (out == db.msm_bigint(want[j])).all(), "row %d of the resident vector" % j
            assert L.dgpu_scalars_free(hj.value) == 0
        assert L.dgpu_scalars_free(handle) == 0

    _, h = many(dev, circ, rows, m, host=False, resident=True)
    check_resident(h)
    got, h = many(dev, circ, rows, m, resident=True)
    assert (got == want[:m]).all()
    check_resident(h)
    got, h = many(dev, circ, rows, m, montgomery=2, resident=True)
    assert (got == O.fr_to_mont(want[:m])).all()
    check_resident(h)
    db.free(); dev.free()


def test_refusals_on_a_real_circuit():
    circ, rows, _ = case(5)
    dev = upload(circ)
    out = np.zeros((2, circ.D, 4), np.uint64)
    L = lib()
    assert L.dgpu_witness_map_r1cs_many(dev.handle, p_(rows), circ.num_vars + 1, circ.num_vars + 1, 2, 0, p_(out), None, None) == BADARG    # not the circuit's num_vars
    assert L.dgpu_witness_map_r1cs_many(dev.handle, p_(rows), circ.num_vars - 1, circ.num_vars, 2, 0, p_(out), None, None) == BADARG
    assert L.dgpu_witness_map_r1cs_many(dev.handle, p_(rows), circ.num_vars, circ.num_vars, 2, 0, None, None, None) == BADARG
    db = ca.DeviceBases(ca.G1, U.seq_bases(O.G1, 4, 43, threads=1)[0])
    assert L.dgpu_witness_map_r1cs_many(db.handle, p_(rows), circ.num_vars, circ.num_vars, 2, 0, p_(out), None, None) == BADARG           # a handle of another kind
    assert L.dgpu_witness_map_r1cs_many(dev.handle, None, 0, 0, 0, 0, None, None, None) == 0
    assert not out.any()
    db.free(); dev.free()


def test_two_calls_in_flight_on_two_circuits():
    (c1, r1, w1), (c2, r2, w2) = case(7), case(10)
    d1, d2 = upload(c1), upload(c2)
    with ThreadPoolExecutor(2) as ex:
        for _ in range(3):
            f1 = ex.submit(many, d1, c1, r1, M_MAX)
            f2 = ex.submit(many, d2, c2, r2, M_MAX)
            assert (f1.result() == w1).all() and (f2.result() == w2).all()
    d1.free(); d2.free()


def test_a_second_call_of_the_same_shape_allocates_nothing():
    circ, rows, want = case(9)
    dev = upload(circ)
    L = lib()
    L.dgpu_device_alloc_count.restype = C.c_uint64
    for _ in range(8):                                         # every slot of the context has seen the shape (slots are handed out in turn)
        many(dev, circ, rows, M_MAX)
    before = L.dgpu_device_alloc_count()
    for _ in range(8):
        assert (many(dev, circ, rows, M_MAX) == want).all()
    assert L.dgpu_device_alloc_count() == before
    dev.free()


def test_mimc_row_of_the_many_call_proves():
    """tests/mimc_circuit.py end to end: row 0 of witness_map_many -> the h-query MSM on the resident key (dgpu_msm_g1_handle) -> the existing prover; the
    proof verifies and is the proof of the single call's h"""
    import lego_setup as LS
    import mimc_circuit as MC
    from crypto_amd import legogroth16 as LG
    rng = np.random.default_rng(5)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % (W.R - 1) + 1
    constants = [rnd() for _ in range(MC.MIMC_ROUNDS)]
    g1 = lambda k: O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(k % W.R, 4)))[0]
    g2 = lambda k: O.G2.to_affine(O.G2.mul(O.G2.generator(), O.int_to_limbs(k % W.R, 4)))[0]
    shape = MC.circuit(1, 2, constants)
    pk, n_inst = LG.generate_parameters(shape["A"], shape["B"], shape["C"], shape["n_inst"], shape["n_wit"], 2, *[rnd() for _ in range(6)], g1(rnd()), g2(rnd()))
    pvk = LG.prepare_verifying_key(pk.vk)
    circ = qap.DeviceR1cs(*[qap.csr(shape[k]) for k in "ABC"], len(shape["z"]), shape["n_inst"], shape["n_cons"])
    stmts = [MC.circuit(rnd(), rnd(), constants) for _ in range(2)]
    zs = np.stack([LS.scalars(cs["z"]) for cs in stmts])
    h_many, _ = qap.witness_map_many(circ, zs)
    assert h_many.shape[1] == 1024
    for j, cs in enumerate(stmts):
        assert (h_many[j] == LS.scalars(LS.witness_map(cs))).all()
    z, h = zs[0], h_many[0]
    assert (pk.h_query.msm_bigint(h) == pk.h_query.msm_bigint(circ.witness_map(z)[0])).all()
    r, s, v = rnd(), rnd(), rnd()
    proof = LG.create_proof(pk, r, s, v, h, z[:n_inst], z[n_inst:])
    assert LG.verify_proof(pvk, proof, LS.scalars([cs["z"][1] for cs in stmts[:1]]))
    assert not LG.verify_proof(pvk, proof, LS.scalars([(stmts[0]["z"][1] + 1) % W.R]))
    circ.free()
