"""The dgpu_smc_range_proofs_* calls on one device, beside the same work done the only way the library allowed before them — the caller's chain of public calls
from the same build, with a PCIe round trip and host work between each:
  chain   dgpu_accumulator_membership_proofs_verify_each_g1 with V = g1 over the n S l digit proofs (the digit proof IS that membership proof)
          -> host: the sides' own scalars (a c, b c + sum_j w_j z2_j, e zr, -1) with Python integers
          -> dgpu_msm_g1_segments over [C, g, h, D_s], one 4-term segment per side
          -> host: the fold of a proof's S l + S results into (status, detail) in the reference's order of errors
The chain must give the exact call's statuses (asserted; a bad D, a bad z1, an identity A' and a signature under another key among the proofs).  The statements
are CLS and CCS at base 4 over the 32-bit range [0, 2^32): l = 16 (S l = 16) and l = 17 (S l = 34).  The exact form, the merged form and the batch stand beside
the chain; the batch that is timed is the one that verifies.  The points are multiples of the generator made by the library's own window table; the first are
compared with the oracle.  Host clock round synchronous calls; the sides of a comparison ALTERNATE inside one loop after a warm call of each, and the median of
--reps is kept.  Stage times come from a second pass on the development build.  No pass / fail threshold: the numbers are written down.  Writes
profiles/smc_timing.json.

    python tests/perf/smc_timing.py [--rows 64,1024,4096] [--reps 7] [--out profiles/smc_timing.json]
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
import smc_model as SM                     # noqa: E402
from crypto_amd import smc_range_proof as SRP, accumulator as ACC   # noqa: E402
from crypto_amd import G1 as CG1           # noqa: E402
from crypto_amd.msm import msm_segments    # noqa: E402
from crypto_amd.fixed_base import WindowTable  # noqa: E402
from crypto_amd._native import twin        # noqa: E402

R = SM.R
PREFIXES = ("smc.", "bbs.", "msm.")
RHO = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543211234567


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def alternate(fns, reps):
    """median milliseconds of each function, the functions taking turns inside one loop after a warm call of each"""
    for f in fns:
        f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t0 = time.perf_counter(); f(); ts[k].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="64,1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smc_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    rng = np.random.default_rng(161803)
    ns = [int(v) for v in args.rows.split(",")]
    key = SM.Key(*rand(rng, 4))
    T1 = WindowTable(CG1, O.G1.generator())

    def g1_times(scalars):
        out, inf = T1.multiply_many(limbs([k % R for k in scalars]))
        out[inf.astype(bool)] = 0
        return out
    g2 = O.G2.generator()
    pk = O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(key.alpha, 4)))[0]
    g1, g, h = g1_times([key.gamma, key.kg, key.kh])
    assert (g1 == O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(key.gamma, 4)))[0]).all()
    params, vkey = SRP.Params(g1, g2, pk, g, h), ACC.VerifierKey(pk, g2)
    res = {"reps": args.reps, "statements": {}}

    for name, kind in (("cls", SM.CLS), ("ccs", SM.CCS)):
        st = SM.Statement(kind, 0, 2 ** 32, 4)
        S, l, D = st.sides, st.l, st.D
        srow = {"sides": S, "l": l}
        nmax = max(ns)
        t0 = time.perf_counter()
        proofs = []
        for i in range(nmax):
            b = rand(rng, 1 + S * (1 + 3 * l) + 2)
            proofs.append(SM.prove(key, st, int(rng.integers(0, 2 ** 32)), b[-1], b[-2], lambda j: b[j], other_key=(i == 5)))
        proofs[1] = SM.tamper(proofs[1], "D", s=S - 1)
        proofs[3] = SM.tamper(proofs[3], "z1", D - 1)
        proofs[7] = SM.tamper(proofs[7], "A_identity", 2)
        srow["prove_in_python_s"] = time.perf_counter() - t0
        pts = g1_times([p.C for p in proofs] + [v for p in proofs for v in p.D] + [v for p in proofs for d in p.digits for v in (d.ap, d.abar, d.t)])
        Cs, Ds, dig = pts[:nmax], pts[nmax:nmax + nmax * S].reshape(nmax, S, 12), pts[nmax + nmax * S:].reshape(nmax, D, 3, 12)
        c, zr = limbs([p.c for p in proofs]), limbs([v for p in proofs for v in p.zr]).reshape(nmax, S, 4)
        z = limbs([v for p in proofs for d in p.digits for v in (d.z1, d.z2)]).reshape(nmax, D, 2, 4)
        want_all = [p.status(key, st) for p in proofs]
        good = np.array([w == (0, 0) for w in want_all])
        rnd = limbs(rand(rng, nmax))
        pos = [st.ref_position(d) for d in range(D)]

        for n in ns:
            row = {}
            pr = SRP.Proofs(st.as_tuple(), Cs[:n], c[:n], Ds[:n], zr[:n].reshape(-1, 4), dig[:n], z[:n].reshape(-1, 4))
            gn = good[:n]
            prg = SRP.Proofs(st.as_tuple(), Cs[:n][gn], c[:n][gn], Ds[:n][gn], zr[:n][gn].reshape(-1, 4), dig[:n][gn], z[:n][gn].reshape(-1, 4))
            host_ms = []

            def chain():
                dst = ACC.membership_proofs_verify_each(vkey, g1, dig[:n].reshape(-1, 3, 12), z[:n].reshape(-1, 2, 4), np.repeat(c[:n], D, axis=0))
                t0 = time.perf_counter()
                sc = []
                for p in proofs[:n]:
                    sc += p.own(st)[:4 * S]
                bases = np.empty((n, S, 4, 12), np.uint64)
                bases[:, :, 0], bases[:, :, 1], bases[:, :, 2], bases[:, :, 3] = Cs[:n, None], g, h, Ds[:n]
                scl = limbs(sc)
                host_ms.append((time.perf_counter() - t0) * 1e3)
                _, sinf = msm_segments(CG1, bases.reshape(-1, 12), scl, [4 * (k + 1) for k in range(n * S)], flags=True)
                t0 = time.perf_counter()
                out = []
                dst, sinf = dst.reshape(n, D).tolist(), np.asarray(sinf).reshape(n, S).tolist()
                for i in range(n):
                    bad = [s for s in range(S) if not sinf[i][s]]
                    ks = [4 * pos[d] + k for d, k in enumerate(dst[i]) if k]
                    out.append((1, bad[0] + 1) if bad else (2, min(ks)) if ks else (0, 0))
                host_ms[-1] += (time.perf_counter() - t0) * 1e3
                return out
            tup = lambda sd: list(zip(sd[0].tolist(), sd[1].tolist()))
            exact = lambda: SRP.verify_each(params, st.as_tuple(), pr)
            merged = lambda: SRP.verify_each(params, st.as_tuple(), pr, random=rnd[:n])
            batch = lambda: SRP.verify_batch(params, st.as_tuple(), prg, RHO)
            want = want_all[:n]
            assert tup(exact()) == want and chain() == want and len({w for w in want}) == 5
            assert tup(merged()) == [p.status(key, st, random=int(sum(int(x) << (64 * k) for k, x in enumerate(r)))) for p, r in zip(proofs[:n], rnd[:n])]
            assert batch() and not SRP.verify_batch(params, st.as_tuple(), pr, RHO)
            host_ms.clear()
            row["each_exact_ms"], row["each_merged_ms"], row["batch_ms"], row["chain_ms"] = alternate([exact, merged, batch, chain], args.reps)
            row["chain_host_ms"] = float(np.median(host_ms))
            row["slices"] = n * D
            with twin(smc=True):                                        # the stage timers live on the development build
                for cname, fn in (("each_exact", exact), ("each_merged", merged), ("batch", batch)):
                    fn()
                    ca.prof.enable(True); ca.prof.reset()
                    for _ in range(3):
                        fn()
                    stg = ca.prof.read()
                    ca.prof.enable(False)
                    row[cname + "_stages_ms"] = {k: v[0] / 3 for k, v in stg.items() if k.startswith(PREFIXES)}
            srow["n=%d" % n] = row
            print(name, n, json.dumps(row), flush=True)
        res["statements"][name] = srow
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    T1.free()


if __name__ == "__main__":
    main()
