"""The dgpu_bpp_range_proofs_* calls on one device, beside the same work done the only way the library allowed before them — the caller's chain of public calls
from the same build, with a PCIe round trip and host work between each:
  chain   host: the 9 + NG shared and m + 4 + 2 K own scalars of every proof from the closed form of tests/bpp_model.py (Python integers), status 2 decided there
          -> dgpu_msm_g1_handle_many over the resident setup: P_i per proof
          -> dgpu_msm_g1_segments over [V .., D, M, R, S, X .., R .., P_i], one (own + 1)-term segment per proof
          -> host: status from the segments' identity flags
The chain must give the each call's statuses (asserted; a moved point, a moved n0, a moved challenge and a status-2 proof among the proofs).  The shape is
proof_system's: base 2, 64 bits, two values (NG = 128, K = 7: 137 shared and 20 own terms).  The n proofs are POOL distinct proofs of the model's prover taken in
turn — the verifier's work does not depend on whether two proofs are equal, the prover's Python time does.  Timed: each, the batch that verifies, the batch that
refuses (one bad proof at the end), the chain with its host share on its own, and — outside the calls — the host's Merlin time for the same proofs
(crypto_amd.bpp_range_proof.challenges over the C transcript).  The points are multiples of the generator made by the library's own window table; the first are
compared with the oracle.  Host clock round synchronous calls; the sides of a comparison ALTERNATE inside one loop after a warm call of each, and the median of
--reps is kept.  Stage times come from a second pass on the development build.  No pass / fail threshold: the numbers are written down.  Writes
profiles/bpp_timing.json.

    python tests/perf/bpp_timing.py [--rows 64,1024,4096] [--reps 7] [--out profiles/bpp_timing.json]
"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import crypto_amd as ca                    # noqa: E402
import oracle_c as O                       # noqa: E402
import bpp_model as BM                     # noqa: E402
from crypto_amd import bpp_range_proof as BRP   # noqa: E402
from crypto_amd import G1 as CG1           # noqa: E402
from crypto_amd.msm import msm_segments, DeviceBases   # noqa: E402
from crypto_amd.fixed_base import WindowTable  # noqa: E402
from crypto_amd.aggregation.transcript import NativeMerlinTranscript, build_helper   # noqa: E402
from crypto_amd._native import twin        # noqa: E402

R = BM.R
PREFIXES = ("bpp.", "msm.")
RHO = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567
SHAPE = (2, 64, 2)
POOL = 32


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def alternate(fns, reps):
    """median milliseconds of each function, the functions taking turns inside one loop; each has had its warm call (the assertions in front of the loop)"""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t0 = time.perf_counter(); f(); ts[k].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="64,1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpp_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    build_helper()
    ns = [int(v) for v in args.rows.split(",")]
    s = BM.Shape(*SHAPE)
    rnd = BM.make_rnd(271828)
    T1 = WindowTable(CG1, O.G1.generator())

    def g1_times(scalars):
        out, inf = T1.multiply_many(limbs([k % R for k in scalars]))
        out[inf.astype(bool)] = 0
        return out
    msetup = BM.Setup(s, rnd)
    spts = g1_times(msetup.logs())
    assert (spts[0] == O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(msetup.g, 4)))[0]).all()
    res = {"reps": args.reps, "shape": {"base": s.base, "num_bits": s.num_bits, "m": s.m, "NG": s.NG, "K": s.K, "shared": s.shared, "own": s.own}, "pool": POOL}
    t0 = time.perf_counter()
    good = [BM.prove(s, msetup, [rnd() & ((1 << 64) - 1) for _ in range(s.m)], rnd) for _ in range(POOL)]
    res["prove_in_python_s_per_proof"] = (time.perf_counter() - t0) / POOL
    pool = list(good)
    pool[1] = BM.tamper(good[1], "M")
    pool[3] = BM.tamper(good[3], "n0")
    pool[5] = BM.tamper(good[5], "gamma3")
    pool[7] = good[7].copy(); pool[7].chal[6] = 0                           # t = 0: status 2
    want_pool = [BM.status(s, msetup, p) for p in pool]
    assert sorted(set(want_pool)) == [0, 1, 2]

    def arrays(proofs):
        pts = g1_times([v for p in proofs for v in p.own_points()]).reshape(len(proofs), s.own, 12)
        return pts, limbs([v for p in proofs for v in (p.l0, p.n0)]).reshape(len(proofs), 2, 4), limbs([c for p in proofs for c in p.chal]).reshape(len(proofs), 7 + s.K, 4)
    ppts, pln, pch = arrays(pool)
    gpts, gln, gch = arrays(good)
    setup = BRP.Setup(spts[0], spts[9:], spts[1:9])                          # in libdock_gpu_bpp.so
    chain_setup = DeviceBases(CG1, spts)                                     # in the product: what the chain's many-row call runs over
    one = limbs([1])[0]

    for n in ns:
        row = {}
        idx = np.arange(n) % POOL
        take = lambda pts, ln, ch: BRP.Proofs(s.base, s.num_bits, s.m, pts[idx][:, :s.m], pts[idx][:, s.m:s.m + 4], pts[idx][:, s.m + 4:], ln[idx].reshape(-1, 4), ch[idx].reshape(-1, 4))
        pr, prg = take(ppts, pln, pch), take(gpts, gln, gch)
        bad_last = take(gpts, gln, gch)
        bad_last.round_points = bad_last.round_points.copy()
        bad_last.round_points[4 * (n - 1) + 1] = ppts[1][s.m + 1]           # the last proof's M moved: the batch refuses
        own_pts = np.ascontiguousarray(ppts[idx])
        want = [want_pool[i] for i in idx]
        host_ms = []

        def chain():
            t0 = time.perf_counter()
            rows, own, two = np.zeros((n, s.shared, 4), np.uint64), np.zeros((n, s.own + 1, 4), np.uint64), np.zeros(n, bool)
            for i in range(n):
                sc = BM.verify_closed(s, pool[idx[i]])
                if sc is None:
                    two[i] = True
                    continue
                rows[i] = limbs(sc[0]); own[i, :s.own] = limbs(sc[1]); own[i, s.own] = one
            host_ms.append((time.perf_counter() - t0) * 1e3)
            P, pinf = chain_setup.msm_many(rows, flags=True)
            bases = np.zeros((n, s.own + 1, 12), np.uint64)
            bases[:, :s.own] = own_pts
            bases[:, s.own] = P[:, :12]
            bases[pinf.astype(bool), s.own] = 0
            _, sinf = msm_segments(CG1, bases.reshape(-1, 12), own.reshape(-1, 4), [(s.own + 1) * (k + 1) for k in range(n)], flags=True)
            t0 = time.perf_counter()
            out = [2 if two[i] else 0 if sinf[i] else 1 for i in range(n)]
            host_ms[-1] += (time.perf_counter() - t0) * 1e3
            return out
        each = lambda: BRP.verify_each(setup, s.base, s.num_bits, pr)
        batch_ok = lambda: BRP.verify_batch(setup, s.base, s.num_bits, prg, random=RHO)
        batch_no = lambda: BRP.verify_batch(setup, s.base, s.num_bits, bad_last, random=RHO)
        assert each().tolist() == want and chain() == want
        assert batch_ok() and not batch_no() and not BRP.verify_batch(setup, s.base, s.num_bits, pr, random=RHO)
        host_ms.clear()
        row["each_ms"], row["batch_verifies_ms"], row["batch_refuses_ms"], row["chain_ms"] = alternate([each, batch_ok, batch_no, chain], args.reps)
        row["chain_host_ms"] = float(np.median(host_ms))
        proofs_d = [dict(V=ppts[i][:s.m], D=ppts[i][s.m], M=ppts[i][s.m + 1], R=ppts[i][s.m + 2], S=ppts[i][s.m + 3], X=ppts[i][s.m + 4:s.m + 4 + s.K], Rr=ppts[i][s.m + 4 + s.K:])
                    for i in range(POOL)]
        t0 = time.perf_counter()
        for i in idx:
            BRP.challenges(NativeMerlinTranscript(b"BPP"), s.base, s.num_bits, proofs_d[i])
        row["host_merlin_ms"] = (time.perf_counter() - t0) * 1e3
        with twin(bpp=True):                                                 # the stage timers live on the development build
            tsetup = BRP.Setup(spts[0], spts[9:], spts[1:9])
            for cname, fn in (("each", lambda: BRP.verify_each(tsetup, s.base, s.num_bits, pr)),
                              ("batch", lambda: BRP.verify_batch(tsetup, s.base, s.num_bits, prg, random=RHO))):
                fn()
                ca.prof.enable(True); ca.prof.reset()
                for _ in range(3):
                    fn()
                stg = ca.prof.read()
                ca.prof.enable(False)
                row[cname + "_stages_ms"] = {k: v[0] / 3 for k, v in stg.items() if k.startswith(PREFIXES)}
            tsetup.free()
        res["n=%d" % n] = row
        print(n, json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    setup.free(); chain_setup.free(); T1.free()


if __name__ == "__main__":
    main()
