"""GPU (-m gpu): every route run_passes (crypto_amd/csrc/k_ntt.hip) can send a witness-map transform down, forced at small sizes through the development
knob dgpu_dev_set_ntt (include/dock_gpu_dev.h) and compared bit for bit with the CPU oracle's orc_witness_map (never one GPU route with another):
  * the staged route of domains above 2^26 — k_ntt_fused (both directions, the coset factors applied on load, L = 0 and L > 0 tiles) with the separate
    k_pointwise / k_coset_scale epilogue — at 2^11 .. 2^21: the group sizes and column distances of 2^27 / 2^28 ([6,7], [7,7], [6,7,7], [7,7,7]), the merge of a
    short group ([4,4,7], [4,5,7], [5,5,7]), the smallest tiles, and dense rows (the lazy-limb bounds of its per-stage fr_sub<FR_BIG> + fr_norm);
  * one k_ntt_stage launch per stage with the separate epilogue above the 2^9 where it runs by itself;
  * piped k_ntt_r4 schedules with three strided passes, what 2^23 .. 2^26 run ([5,5,5,8] .. [6,5,5,10]), as 5,5,5,1 / 5,5,5,3 / 5,5,5,5 / 6,5,5,1;
  * the other input / output forms (Montgomery in, Montgomery out, resident h into the MSM, a resident circuit) through a forced route.
Every case reads dgpu_dev_get_ntt_last back: a knob that is silently ignored would pass any parity test.  What no test here runs: arrays beyond 4 GB (the
size_t addressing of k_ntt_fused, k_pointwise, k_coset_scale) and the outermost L = 21 group of 2^27 / 2^28.
Inputs: as tests/test_gpu_witness_map.py test_every_pass_schedule_of_the_ntt (3 instance variables, m = D - 3 rows of two random terms; such an assignment
does not satisfy its constraints, so h[-1] is whatever the oracle says); the satisfied circuits of the I/O cases also have h[-1] = 0."""
import ctypes as C
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import lego_setup as LS
import crypto_amd as ca
from crypto_amd import qap
from test_gpu_witness_map import oracle_map

pytestmark = pytest.mark.gpu
OK, BADARG = 0, -3
PIPED, PER_STAGE, STAGED = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)
    yield
    _SPARSE.clear(); _DENSE.clear(); _CIRCUIT.clear()


@pytest.fixture
def ntt(twin):
    """the twin with the knob put back to automatic whatever the test did"""
    try:
        yield twin
    finally:
        assert twin.dgpu_dev_set_ntt(0, None, 0) == OK


def set_ntt(T, path, split=()):
    a = np.array(list(split), dtype=np.int32)
    return T.dgpu_dev_set_ntt(path, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a))


def last(T):
    """(route, stage groups in launch order) of the last transform the process launched: the inverse (DIF) transform that ends a witness map"""
    route, groups = C.c_int32(-1), np.zeros(32, dtype=np.int32)
    n = T.dgpu_dev_get_ntt_last(C.byref(route), groups.ctypes.data_as(C.c_void_p), 32)
    assert 0 <= n <= 32
    return route.value, [int(x) for x in groups[:n]]


_SPARSE, _DENSE, _CIRCUIT = {}, {}, {}          # inputs and the oracle's h, computed once per shape and never modified


def sparse_case(logd):
    if logd not in _SPARSE:
        n_inst = 3
        m = (1 << logd) - n_inst
        nv = 700
        rng = np.random.default_rng(100 + logd)
        rp = (np.arange(m + 1, dtype=np.uint64) * np.uint64(2))
        mats = [(rp, rng.integers(0, nv, 2 * m, dtype=np.uint32), O.rand_scalars(300 + 3 * logd + i, 2 * m)) for i in range(3)]
        z = O.rand_scalars(55 + logd, nv)
        cs = {"n_cons": m, "n_inst": n_inst, "z": [O.limbs_to_int(x) for x in z]}
        ref = oracle_map(cs, mats)
        ref.setflags(write=False)
        _SPARSE[logd] = (mats, z, n_inst, m, ref)
    return _SPARSE[logd]


def dense_case(logd, k, skew):
    """the shapes of test_gpu_witness_map.py test_dense_rows_do_not_outgrow_the_lazy_representation"""
    key = (logd, k, skew)
    if key not in _DENSE:
        n_inst = 2
        m = (1 << logd) - n_inst
        nv = 5000
        rng = np.random.default_rng(logd)
        per_row = np.full(m, k, dtype=np.uint64)
        if skew:
            per_row[0::2] = 0
        rp = np.concatenate([[0], np.cumsum(per_row)]).astype(np.uint64)
        nnz = int(rp[-1])
        mats = []
        for i in range(3):
            cols = rng.integers(0, nv, nnz, dtype=np.uint32)
            vals = O.rand_scalars(900 + 3 * logd + i, nnz)
            mats.append((rp, cols, vals))
        z = O.rand_scalars(77 + logd, nv)
        cs = {"n_cons": m, "n_inst": n_inst, "z": [O.limbs_to_int(x) for x in z]}
        ref = oracle_map(cs, mats)
        ref.setflags(write=False)
        _DENSE[key] = (mats, z, n_inst, m, ref)
    return _DENSE[key]


def circuit_case(logd):
    """a satisfied circuit that fills the domain (lego_setup.circuit: m + 1 constraints, 2 instance variables)"""
    if logd not in _CIRCUIT:
        cs = LS.circuit((1 << logd) - 3, x0=3)
        mats = [qap.csr(cs[k]) for k in "ABC"]
        ref = oracle_map(cs, mats)
        ref.setflags(write=False)
        assert len(ref) == 1 << logd
        _CIRCUIT[logd] = (cs, mats, LS.scalars(cs["z"]), ref)
    return _CIRCUIT[logd]


# plan_staged (crypto_amd/csrc/ntt_plan.hpp) in DIF order, as tests/test_ntt_plan_host.py pins it
STAGED_GROUPS = {11: [4, 7], 12: [5, 7], 13: [6, 7], 14: [7, 7], 15: [4, 4, 7], 16: [4, 5, 7], 17: [5, 5, 7], 20: [6, 7, 7], 21: [7, 7, 7]}


@pytest.mark.parametrize("logd", sorted(STAGED_GROUPS))
def test_staged_route_vs_oracle(ntt, logd):
    """path 2: k_ntt_fused over 2048-element tiles + k_pointwise + k_coset_scale, the route of 2^27 and 2^28"""
    mats, z, n_inst, m, ref = sparse_case(logd)
    assert set_ntt(ntt, STAGED) == OK
    h, _ = qap.witness_map(*mats, z, n_inst, m)
    assert last(ntt) == (STAGED, STAGED_GROUPS[logd])
    assert h.shape == ref.shape and (h == ref).all()


@pytest.mark.parametrize("logd,k,skew", [(16, 160, False), (17, 400, True)])
def test_staged_route_with_dense_rows(ntt, logd, k, skew):
    """D x k >= 2^23 products per partial sum through the staged kernel's DIF branch (fr_add + fr_norm, fr_sub<FR_BIG> + fr_norm per stage); skew: the odd
    rows alone carry terms, so the last inverse stages subtract a large partial sum from (nearly) nothing"""
    mats, z, n_inst, m, ref = dense_case(logd, k, skew)
    assert set_ntt(ntt, STAGED) == OK
    h, _ = qap.witness_map(*mats, z, n_inst, m)
    assert last(ntt) == (STAGED, STAGED_GROUPS[logd])
    assert (h == ref).all()


@pytest.mark.parametrize("logd", [10, 11, 14])
def test_per_stage_route_vs_oracle(ntt, logd):
    """path 1: log2 D launches of k_ntt_stage per transform with the separate k_coset_scale / k_pointwise, above the 2^9 where it runs by itself"""
    mats, z, n_inst, m, ref = sparse_case(logd)
    assert set_ntt(ntt, PER_STAGE) == OK
    h, _ = qap.witness_map(*mats, z, n_inst, m)
    assert last(ntt) == (PER_STAGE, [1] * logd)
    assert h.shape == ref.shape and (h == ref).all()


@pytest.mark.parametrize("split", [(5, 5, 5, 1), (5, 5, 5, 3), (5, 5, 5, 5), (6, 5, 5, 1)], ids=lambda s: "-".join(map(str, s)))
def test_piped_route_with_three_strided_passes(ntt, split):
    """what 2^23 .. 2^26 run ([5,5,5,8], [5,5,5,9], [5,5,5,10], [6,5,5,10] in DIF order; the largest automatic schedule the suite reaches has two strided
    passes): the same strided passes in front of a shorter flat one.  Flat passes under 6 stages only the knob produces; k_ntt_r4 handles them (S = 1 stores
    straight to HBM), so the setter accepts them."""
    logd = sum(split)
    mats, z, n_inst, m, ref = sparse_case(logd)
    assert set_ntt(ntt, 0, split) == OK
    h, _ = qap.witness_map(*mats, z, n_inst, m)
    assert last(ntt) == (PIPED, list(split))
    assert h.shape == ref.shape and (h == ref).all()


@pytest.mark.parametrize("path,logd", [(STAGED, 14), (PER_STAGE, 11)])
def test_io_forms_through_a_forced_route(ntt, path, logd):
    """as test_gpu_witness_map.py test_witness_map_vs_oracle: Montgomery inputs, h as Montgomery words (k_fr_canonical_to_mont after the unfused epilogue's
    out_words), a resident h that feeds the MSM, a resident circuit"""
    cs, mats, z, ref = circuit_case(logd)
    want = (STAGED, STAGED_GROUPS[logd]) if path == STAGED else (PER_STAGE, [1] * logd)
    assert set_ntt(ntt, path) == OK
    h, _ = qap.witness_map(*mats, z, cs["n_inst"], cs["n_cons"])
    assert last(ntt) == want
    assert h.shape == ref.shape and (h == ref).all()
    assert not h[-1].any()                     # a satisfied circuit: deg h <= D - 2
    dr = qap.DeviceR1cs(*mats, len(cs["z"]), cs["n_inst"], cs["n_cons"])
    h2, _ = dr.witness_map(z)
    assert (h2 == ref).all()
    matsm = [(rp, cl, O.fr_to_mont(vl)) for rp, cl, vl in mats]
    hm, _ = qap.witness_map(*matsm, O.fr_to_mont(z), cs["n_inst"], cs["n_cons"], montgomery=True)
    assert (hm == ref).all()
    hmm, dh = qap.witness_map(*matsm, O.fr_to_mont(z), cs["n_inst"], cs["n_cons"], montgomery=True, h_montgomery=True, resident=True)
    assert (hmm == O.fr_to_mont(ref)).all()
    h3, _ = dr.witness_map(z, h_montgomery=True)
    assert (h3 == hmm).all()
    assert last(ntt) == want
    bases, _, _ = U.seq_bases(O.G1, len(ref), 17, threads=16)
    assert (ca.DeviceBases(ca.G1, bases).msm_resident(dh) == ca.msm_bigint(ca.G1, bases, ref)).all()      # the resident copy stays canonical
    dh.free(); dr.free()


def test_knob_hygiene(ntt):
    """a refused setting changes nothing (neither the path nor the split in force), and after the reset the automatic schedule runs again"""
    mats, z, n_inst, m, ref = sparse_case(13)
    i32 = lambda v: np.array(v, dtype=np.int32)
    bad = [(1, i32([5, 0, 8])), (1, i32([2, 11])), (1, i32([1] * 13)), (-1, None), (-1, i32([5, 8])), (3, None)]
    for path, split in ((0, (5, 5, 3)), (STAGED, ())):
        assert set_ntt(ntt, path, split) == OK
        for bpath, bsplit in bad:
            assert ntt.dgpu_dev_set_ntt(bpath, None if bsplit is None else bsplit.ctypes.data_as(C.c_void_p), 0 if bsplit is None else len(bsplit)) == BADARG, (bpath, bsplit)
        h, _ = qap.witness_map(*mats, z, n_inst, m)
        assert last(ntt) == ((PIPED, [5, 5, 3]) if path == 0 else (STAGED, [6, 7]))
        assert (h == ref).all()
    # a split for another size is not this domain's business; path 2 leaves a domain below one tile (2^11) on the automatic route
    assert set_ntt(ntt, 0, (5, 5, 5, 1)) == OK
    h, _ = qap.witness_map(*mats, z, n_inst, m)
    assert last(ntt) == (PIPED, [5, 8]) and (h == ref).all()
    mats10, z10, n10, m10, ref10 = sparse_case(10)
    assert set_ntt(ntt, STAGED) == OK
    h, _ = qap.witness_map(*mats10, z10, n10, m10)
    assert last(ntt) == (PIPED, [10]) and (h == ref10).all()
    assert set_ntt(ntt, 0) == OK
    h, _ = qap.witness_map(*mats, z, n_inst, m)
    assert last(ntt) == (PIPED, [5, 8])
    assert (h == ref).all()
