"""dgpu_bbs_plus_pok_verify_each_g1 and dgpu_bbs_plus_pok_verify_batch_g1 on one device, beside the same work done the only way the library allowed before them
— the caller's chain of public calls with a PCIe round trip and host scalar work between each — on the same box in the same process:
  chain    host: the rows (c, z4, y ..) with y = c m on the revealed entries, the own-point scalars (z1, z2, -c, c, -1 | z3, -1), the gather of the own points
           dgpu_msm_g1_handle_many over the rows -> dgpu_msm_g1_segments over the 2 n own-point segments -> dgpu_multi_pairing_segments over the n segments
           ((A', w), (Abar, -g2)) (at most 4096 segments a call: longer batches go in pieces); host: the comparison Q_i = -P_i and the order of the four checks.
           The host scalar work counts inside the clock, because the new call replaces it; it is Python-integer work here where a native caller has field
           arithmetic, so it is ALSO reported on its own (chain_host_scalars_ms) and the chain's time can be read with and without it.
At every shape the chain must give the call's statuses (a row that fails its second Schnorr check and one made from a non-signature among them).  Host clock round
synchronous calls; the sides of a comparison ALTERNATE inside one loop after a warm call of each, and the median of --reps is kept.  Stage times come from a second
pass on the development twin (StageTimer marks).  No pass / fail threshold: the numbers are written down.  Writes profiles/bbs_pok_timing.json.

    python tests/perf/bbs_pok_timing.py [--rows 64,1024,16384] [--messages 30] [--revealed 5] [--reps 7] [--out profiles/bbs_pok_timing.json]
"""
import argparse
import ctypes as C
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
import bbs_model as BM                     # noqa: E402
import bbs_pok_model as PM                 # noqa: E402
from crypto_amd import bbs_plus as BBS     # noqa: E402
from crypto_amd import G1 as CG1           # noqa: E402
from crypto_amd.msm import msm_segments    # noqa: E402
from crypto_amd._native import lib         # noqa: E402

R = BM.R
P_LIMBS = [0xB9FEFFFFFFFFAAAB, 0x1EABFFFEB153FFFF, 0x6730D2A0F6B0F624, 0x64774B84F38512BF, 0x4B1BA7B6434BACD7, 0x1A0111EA397FE69A]
p_ = lambda a: a.ctypes.data_as(C.c_void_p)
PREFIXES = ("bbs.", "msm.")


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def g_times(scalars):
    out, inf = O.g1_scale_batch(np.tile(O.G1.generator(), (len(scalars), 1)), limbs([k % R for k in scalars]), threads=16)
    out[inf.astype(bool)] = 0
    return out


def neg_fq(y):
    """p - y on (n, 6) uint64 limbs, limb by limb with a borrow"""
    out, borrow = np.empty_like(y), np.zeros(len(y), np.uint64)
    for k in range(6):
        pk = np.uint64(P_LIMBS[k])
        t = pk - y[:, k]
        b1 = y[:, k] > pk
        out[:, k] = t - borrow
        borrow = (b1 | (t < borrow)).astype(np.uint64)
    return out


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
    ap.add_argument("--rows", default="64,1024,16384")
    ap.add_argument("--messages", type=int, default=30)
    ap.add_argument("--revealed", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bbs_pok_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    Lm = args.messages
    rng = np.random.default_rng(161803)
    x, gamma = rand(rng, 2)
    key = BM.Key(x, gamma, rand(rng, Lm + 1))
    pts = g_times(key.params_scalars(Lm))
    g2 = O.G2.generator()
    w = O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(x, 4)))[0]
    neg_g2 = O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(R - 1, 4)))[0]
    one = O.fp12_one()
    revealed = sorted({(j * Lm) // args.revealed for j in range(args.revealed)})
    res = {"reps": args.reps, "messages": Lm, "revealed": len(revealed), "shapes": {}}

    def make(n):
        """n proofs from known discrete logs; row n // 2 fails its second Schnorr check, row 1 (n > 2) comes from a non-signature"""
        proofs = []
        for i in range(n):
            e, s, r1, r2, c = rand(rng, 5)
            m = rand(rng, Lm)
            a = key.a(e, s, m)
            if n > 2 and i == 1:
                a = (a + 1) % R
            proofs.append(PM.prove(key, a, e, s, m, set(revealed), r1, r2, rand(rng, 4 + Lm), c))
        proofs[n // 2].pts[4] = (proofs[n // 2].pts[4] + 1) % R
        points = g_times([k for p in proofs for k in p.pts]).reshape(n, 5, 12)
        fixed = limbs([z for p in proofs for z in p.fixed]).reshape(n, 4, 4)
        values = limbs([v for p in proofs for v in p.values]).reshape(n, Lm, 4)
        mask = np.array([p.mask for p in proofs], np.uint8)
        chal = limbs([p.c for p in proofs])
        return proofs, points, fixed, values, mask, chal

    def run(P, n, row, data):
        proofs, points, fixed, values, mask, chal = data
        rho = limbs(rand(rng, 1))[0]
        qa = np.ascontiguousarray(np.tile(np.stack([w, neg_g2]), (n, 1)))
        pair_ends = (2 * np.arange(1, n + 1)).astype(np.uint64)
        seg_ends = np.stack([7 * np.arange(n) + 5, 7 * np.arange(n) + 7], axis=1).reshape(-1).astype(np.uint64)
        minus_one = limbs([R - 1])[0]
        host_ms = []

        def chain():
            t0 = time.perf_counter()
            # the host's scalar work: c m on the revealed entries, -c; everything else is copied as it stands
            cs = [O.limbs_to_int(v) for v in chal]
            rows = np.empty((n, Lm + 2, 4), np.uint64)
            rows[:, 0], rows[:, 1], rows[:, 2:] = chal, fixed[:, 3], values
            for j in revealed:
                rows[:, 2 + j] = limbs([c * O.limbs_to_int(v) % R for c, v in zip(cs, values[:, j])])
            own = np.empty((n, 7, 4), np.uint64)
            own[:, 0], own[:, 1], own[:, 2], own[:, 3], own[:, 4], own[:, 5], own[:, 6] = fixed[:, 0], fixed[:, 1], limbs([(R - c) % R for c in cs]), chal, minus_one, fixed[:, 2], minus_one
            bases = np.empty((n, 7, 12), np.uint64)
            bases[:, 0], bases[:, 1], bases[:, 2], bases[:, 3], bases[:, 4], bases[:, 5], bases[:, 6] = points[:, 0], pts[1], points[:, 1], points[:, 2], points[:, 3], points[:, 2], points[:, 4]
            host_ms.append((time.perf_counter() - t0) * 1e3)
            pj, pinf = P.bases.msm_many(rows, flags=True)
            sj, sinf = msm_segments(CG1, bases.reshape(-1, 12), own.reshape(-1, 4), seg_ends, flags=True)
            pa = np.ascontiguousarray(points[:, :2])
            out = np.zeros((n, 72), np.uint64)
            for lo in range(0, n, 4096):                             # (the call takes at most 4096 segments)
                k = min(4096, n - lo)
                assert lib().dgpu_multi_pairing_segments(p_(pa[lo:]), p_(qa[2 * lo:]), None, 2 * k, p_(pair_ends), k, p_(out[lo:])) == 0
            pairing = (out == one).all(axis=1)
            q, qinf = sj[1::2], sinf[1::2].astype(bool)
            second = np.where(pinf.astype(bool) | qinf, pinf.astype(bool) & qinf, (pj[:, :6] == q[:, :6]).all(axis=1) & (neg_fq(pj[:, 6:12]) == q[:, 6:12]).all(axis=1))
            a_inf = ~points[:, 0].any(axis=1)
            return np.where(a_inf, 1, np.where(sinf[0::2] == 0, 2, np.where(~second, 3, np.where(~pairing, 4, 0)))).astype(np.uint8)

        want = np.array([p.status(key) for p in proofs], np.uint8)
        each_new = lambda: BBS.pok_verify_each(P, points, fixed, values, mask, chal)
        batch_bad = lambda: BBS.pok_verify_batch(P, points, fixed, values, mask, chal, rho)
        # the batch that is timed is the one that VERIFIES (a failing G1 equation returns before the pairing): the valid rows, the two others replaced by row 0
        good = [i if want[i] == 0 else 0 for i in range(n)]
        gp, gf, gv, gm, gc = points[good], fixed[good], values[good], mask[good], chal[good]
        batch_new = lambda: BBS.pok_verify_batch(P, gp, gf, gv, gm, gc, rho)
        assert want[n // 2] == 3 and (n <= 2 or want[1] == 4) and int((want != 0).sum()) == (2 if n > 2 else 1)
        assert (each_new() == want).all() and (chain() == want).all() and not batch_bad() and batch_new()      # the chain and the call: the same statuses
        host_ms.clear()
        row["pok_verify_each_ms"], row["pok_verify_batch_ms"], row["pok_verify_batch_refusing_ms"], row["chain_ms"] = alternate([each_new, batch_new, batch_bad, chain], args.reps)
        row["chain_host_scalars_ms"] = float(np.median(host_ms))
        return each_new, batch_new

    for n in [int(v) for v in args.rows.split(",")]:
        row = {}
        data = make(n)
        with BBS.Params(pts[0], pts[1], pts[2:], g2, w) as P:
            run(P, n, row, data)
        with ca.twin():                                             # the stage timers live on the twin: parameters of its own
            with BBS.Params(pts[0], pts[1], pts[2:], g2, w) as P:
                calls = run(P, n, {}, data)
                for name, fn in zip(("pok_verify_each", "pok_verify_batch"), calls):
                    ca.prof.enable(True); ca.prof.reset()
                    for _ in range(args.reps):
                        fn()
                    st = ca.prof.read()
                    ca.prof.enable(False)
                    row[name + "_stages_ms"] = {k: v[0] / args.reps for k, v in st.items() if k.startswith(PREFIXES)}
        res["shapes"]["n=%d" % n] = row
        print(n, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
