"""CPU: the block witness map's DEVICE body (crypto_amd/csrc/wm_block_kernels.hip.h wm_block, what k_wm_block launches for
dgpu_witness_map_r1cs_many) compiled for the host with the FP29_CHECK operand asserts (tests/native/wm_block_host_shim.cpp) and compared word for
word with the oracle's witness map, for every domain from 2 to 2^10 (odd exponents start with a lone radix-2 stage).  A green run shows the fused
chain — sparse rows, three transforms back to back, the pointwise step — computes h and that no product of it leaves its operand contract: an
assert that fires inside the shim aborts the run."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import oracle_c as O                      # noqa: E402
import wm_many_circuits as W              # noqa: E402

SRC = os.path.join(HERE, "native", "wm_block_host_shim.cpp")
SO = os.path.join(HERE, "native", "libwm_block_host_shim.so")
CSRC = os.path.join(ROOT, "crypto_amd", "csrc")
R = W.R
p_ = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("fr29.hip.h", "ntt_lanes.hip.h", "wm_block_kernels.hip.h", "wm_block_args.hip.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DFP29_CHECK", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.shim_wm_many.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p] + [C.c_void_p] * 9 + [C.c_size_t] * 3 + [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.shim_wm_many.restype = C.c_int
    return L


def domain_consts(logn):
    """w, w^-1, g, g^-1, 1 / D, 1, 1 / Z(g) of the domain of 2^logn elements (ark-poly Radix2EvaluationDomain over Fr, coset generator 7)"""
    D = 1 << logn
    w = pow(7, (R - 1) >> logn, R)
    inv = lambda v: pow(v, R - 2, R)
    return W.to_words([w, inv(w), 7, inv(7), inv(D), 1, inv((pow(7, D, R) - 1) % R)])


def run(L, circ, rows, rows_per_block, nlanes, row_stride=None, mont=False, out_mont=False):
    m = len(rows)
    stride = row_stride or circ.num_vars
    z = np.full((m, stride, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)       # what lies between two rows is never read
    z[:, :circ.num_vars] = O.fr_to_mont(rows) if mont else rows
    mats = [(rp, cl, O.fr_to_mont(vl) if mont and len(vl) else vl) for rp, cl, vl in circ.mats]
    keep = [np.ascontiguousarray(a) for mtx in mats for a in mtx]
    consts = domain_consts(circ.logn)
    out = np.zeros((m, circ.D, 4), dtype=np.uint64)
    blocks = L.shim_wm_many(circ.logn, rows_per_block, nlanes, m, p_(consts), *[p_(a) for a in keep], circ.num_constraints, circ.num_inputs, circ.num_vars,
                            p_(z), stride, int(mont), int(out_mont), p_(out))
    assert blocks == (m + rows_per_block - 1) // rows_per_block
    return out


def default_rpb(logn):
    return 1 if logn >= 8 else 256 >> logn


@pytest.mark.parametrize("logn", range(1, 11))
def test_every_domain_matches_the_oracle_and_trips_no_bound(shim, logn):
    """a circuit that fills the domain exactly and one that is one past a power of two; rows that satisfy it, rows that do not, z = 0 (h = 0)"""
    for circ in (W.fill_exact(100 + logn, logn), W.one_past(200 + logn, logn)):
        assert circ.logn == logn
        rows = W.rows_for(circ, 3, 300 + logn, kinds=("sat", "rand", "zero"))
        want = W.oracle_h(circ, rows)
        assert not want[2].any(), "z = 0 gives h = 0"
        # the kernel's own rows per block (one lane per radix-4 unit), and one statement per block with a block of a single wave's lanes
        got = run(shim, circ, rows, default_rpb(logn), 192)
        assert (got == want).all()
        got = run(shim, circ, rows, 1, 64)
        assert (got == want).all()


@pytest.mark.parametrize("logn", [3, 6, 7, 10])
def test_empty_row_and_the_dense_worst_case_row(shim, logn):
    """a matrix row without a term, and a row of num_vars terms of value r - 1 against z = r - 1: the longest lazy sum the row body can be handed"""
    D = 1 << logn
    circ = W.random_circuit(400 + logn, D - 2, 2, D + 5, empty_row=1, dense_row=D // 2)
    rows = W.rows_for(circ, 2, 500 + logn, kinds=("max", "rand"))
    want = W.oracle_h(circ, rows)
    assert (run(shim, circ, rows, default_rpb(logn), 768) == want).all()


def test_rows_per_block_tail_stride_and_both_montgomery_flags(shim):
    """five statements at three per block (a block whose last statement does not exist), rows further apart than num_vars with bit 255 set in between,
    inputs as Fr limbs, h as Fr limbs"""
    circ = W.one_past(600, 5)
    rows = W.rows_for(circ, 5, 601)
    want = W.oracle_h(circ, rows)
    assert (run(shim, circ, rows, 3, 128, row_stride=circ.num_vars + 3) == want).all()
    assert (run(shim, circ, rows, 3, 128, mont=True) == want).all()
    assert (run(shim, circ, rows, 8, 192, mont=True, out_mont=True) == O.fr_to_mont(want)).all()
