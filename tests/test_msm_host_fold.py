"""CPU: the host-side folds of the MSM driver (crypto_amd/csrc/msm_host_fold.hpp) against the oracle, for G1 (hostf::Fq) and G2 (hostf::Fq2).
tests/native/msm_host_fold_driver.cpp is built with the host compiler from that header alone — once plainly, once with AddressSanitizer + UBSan, each
run as a program of its own — and fed the smallest shapes that reach every branch of host_fold, host_fold_shared, host_fold_marginals,
host_fold_jacobian and host_lincomb.  Window sums are affine multiples of the generator with zz = zzz = 1; flagged identities carry garbage
coordinates.  Every result must equal the oracle's (msm / mul / add) word for word after to_affine, be normalised (Z = 1), and the identity must come
out as (1, 1, 0)."""
import os
import re
import shutil
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_c as O  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "msm_host_fold_driver.cpp")
ABI = open(os.path.join(ROOT, "include", "dock_gpu.h")).read()
MAX_LINCOMB = int(re.search(r"^#define\s+DGPU_MAX_LINCOMB\s+(\d+)", ABI, re.M).group(1))
BADARG = int(re.search(r"^#define\s+DGPU_E_BADARG\s+(-?\d+)", ABI, re.M).group(1))
BUILDS = {"plain": ([], {}),
          "asan_ubsan": (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], {"ASAN_OPTIONS": "detect_leaks=1 exitcode=67"})}


def limbs(v):
    return np.array(O.int_to_limbs(v, 4), dtype=np.uint64)


class Cases:
    """the input words of one curve's run and, per case, (expected return code, expected Jacobian or None)"""

    def __init__(self, G):
        self.G, self.F = G, G.AW // 2
        fp_one = O.fp_to_mont(np.array([1, 0, 0, 0, 0, 0], dtype=np.uint64))
        self.one = np.concatenate([fp_one, np.zeros(self.F - 6, dtype=np.uint64)])
        self.gen = G.generator()
        self.words, self.expect = [], []
        self.identity = np.concatenate([self.one, self.one, np.zeros(self.F, dtype=np.uint64)])

    def aff(self, m):
        a, inf = self.G.to_affine(self.G.mul(self.gen, limbs(m)))
        assert not inf
        return a

    def xyzz(self, m):
        """the window sum m G in ABI XYZZ words; m = None: a flagged identity with garbage coordinates"""
        if m is None:
            return np.full(4 * self.F, 0xdeadbeefdeadbeef, dtype=np.uint64)
        return np.concatenate([self.aff(m), self.one, self.one])

    def weighted(self, ms, weights):
        """sum_i weights[i] * ms[i] G by the oracle's msm (None = identity)"""
        bases = np.stack([self.gen if m is None else self.aff(m) for m in ms])
        inf = np.array([m is None for m in ms], dtype=np.uint8)
        return self.G.msm(bases, np.stack([limbs(w) for w in weights]), is_inf=inf)

    def add(self, op, p0, p1, arrays, rc, jac):
        self.words += [np.array([op, p0, p1, 0], dtype=np.uint64)] + [np.asarray(a, dtype=np.uint64).reshape(-1) for a in arrays]
        self.expect.append((rc, jac))

    def flags(self, ms):
        return np.array([m is None for m in ms], dtype=np.uint64)

    def build(self):
        G, F = self.G, self.F
        pts = lambda ms: np.concatenate([self.xyzz(m) for m in ms])  # noqa: E731
        # host_fold: W = 3, c = 7 — every window live; the top one an identity (the doublings are passed over while the accumulator is the identity);
        # the middle one; all of them
        for ms in ([5, 11, 3], [5, 11, None], [5, None, 3], [None, None, None]):
            self.add(1, 3, 7, [pts(ms), self.flags(ms)], 0, self.weighted(ms, [1 << (7 * w) for w in range(3)]))
        # host_fold_shared: PW = 1 (no weighted term: S_0 is never read); PW = 4, lb = 2 with one A_j and one S_j an identity
        for PW, lb, A, S in ((1, 2, [9], [13]), (4, 2, [3, None, 9, 2], [4, 6, None, 10])):
            self.add(2, PW, lb, [pts(A), self.flags(A), pts(S), self.flags(S)], 0, self.weighted(A + S, [1] * PW + [j << lb for j in range(PW)]))
        # host_fold_marginals: P + 2^shift sum_t 2^t M_t — nm = 0; nm = 3 with shift 0 and 2; P an identity; every marginal an identity
        for shift, ms in ((2, [7]), (0, [7, 3, 5, 9]), (2, [7, 3, 5, 9]), (2, [None, 3, 5, 9]), (2, [7, None, None, None])):
            self.add(3, len(ms) - 1, shift, [pts(ms), self.flags(ms)], 0, self.weighted(ms, [1] + [1 << (shift + t) for t in range(len(ms) - 1)]))
        # host_fold_jacobian: k = 0; k = 3 with a normalised triple, a Z = 0 entry (garbage X, Y) and a triple with Z != 1 (the oracle's raw 12 G)
        self.add(4, 0, 0, [], 0, self.identity)
        j0 = np.concatenate([self.aff(5), self.one])
        j1 = np.concatenate([np.full(2 * F, 0x1234567, dtype=np.uint64), np.zeros(F, dtype=np.uint64)])
        j2 = G.mul(self.gen, limbs(12))
        assert not (j2[2 * F:] == self.one).all() and j2[2 * F:].any(), "the oracle's raw product is expected to have Z != 0, 1"
        self.add(4, 3, 0, [j0, j1, j2], 0, G.add(j0, j2))
        # host_lincomb: k = 0; k = 3 with a zero scalar, an all-zero point and a flagged identity (nothing live); the same three among three live terms;
        # one term too many
        sc = O.rand_scalars(77, MAX_LINCOMB + 1)
        self.add(5, 0, 0, [], 0, self.identity)
        dead_pts = np.stack([self.aff(21), np.zeros(2 * F, dtype=np.uint64), self.aff(22)])
        dead_sc = sc[:3].copy(); dead_sc[0] = 0
        self.add(5, 3, 1, [dead_pts, [0, 0, 1], dead_sc], 0, self.identity)
        live_pts = np.stack([self.aff(31), self.aff(32), self.aff(33)])
        order = [0, 3, 1, 4, 2, 5]                                   # live and dead terms interleaved
        mix_pts = np.concatenate([live_pts, dead_pts])[order]
        mix_sc = np.concatenate([sc[3:6], dead_sc])[order]
        mix_inf = np.array([0, 0, 0, 0, 0, 1], dtype=np.uint64)[order]
        self.add(5, 6, 1, [mix_pts, mix_inf, mix_sc], 0, G.msm(live_pts, sc[3:6]))
        many = np.stack([self.aff(40 + i) for i in range(MAX_LINCOMB + 1)])
        self.add(5, MAX_LINCOMB + 1, 0, [many, np.zeros(MAX_LINCOMB + 1, dtype=np.uint64), sc], BADARG, None)
        return self


@pytest.fixture(scope="module", params=["g1", "g2"])
def cases(request):
    return request.param, Cases(O.G1 if request.param == "g1" else O.G2).build()


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("needs a host C++ compiler")
    d = tmp_path_factory.mktemp("msm_host_fold")
    exe = {}
    for name, (flags, _) in BUILDS.items():
        exe[name] = str(d / ("mhf_" + name))
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-mbmi2", "-madx"] + flags + ["-o", exe[name], SRC])
    return exe


@pytest.mark.parametrize("build", list(BUILDS))
def test_host_folds_equal_the_oracle(build, cases, drivers, tmp_path):
    curve, cs = cases
    G, F = cs.G, cs.F
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.array([len(cs.expect)], dtype=np.uint64)] + cs.words).tofile(fin)
    r = subprocess.run([drivers[build], curve, fin, fout], env=dict(os.environ, **BUILDS[build][1]), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "msm_host_fold_driver: ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = np.fromfile(fout, dtype=np.uint64).reshape(len(cs.expect), 1 + 3 * F)
    for i, (rc, want) in enumerate(cs.expect):
        assert int(out[i, 0].astype(np.int64)) == rc, (i, out[i, 0])
        if want is None:
            continue
        got = out[i, 1:]
        ga, ginf = G.to_affine(got)
        wa, winf = G.to_affine(want)
        assert ginf == winf and (ga == wa).all(), "case %d" % i
        if ginf:
            assert (got == cs.identity).all(), "case %d: the identity is (1, 1, 0)" % i
        else:
            assert (got[:2 * F] == wa).all() and (got[2 * F:] == cs.one).all(), "case %d: not normalised" % i
