"""The seven dgpu_bbs23_* calls on one device, each beside (a) the same work done the only way the library allowed before them — the caller's chain of public
calls with a PCIe round trip and host scalar work between each — and (b) its BBS+ counterpart at the same n and L from the same build, on the same box in the same
process:
  sign chain     dgpu_msm_g1_handle_many over the rows (1, m ..) -> dgpu_g1_mul_add_batch by 1 / (x + e) (the inverses are made before the clock starts)
  verify chain   dgpu_msm_g1_handle_many -> dgpu_g1_mul_add_batch (e A - b) -> dgpu_multi_pairing_segments (at most 4096 segments a call)
  proof chains   host: the rows (c, y ..) with y = c m on the revealed entries, the own scalars (z1, z2, -c, -1 | z3, -1) or (z_a, z_b, -1), the gather of
                 the own points; dgpu_msm_g1_handle_many -> dgpu_msm_g1_segments -> dgpu_multi_pairing_segments; host: Q_i = -P_i and the order of the checks.
                 The host scalar work counts inside the clock, because the new call replaces it; it is Python-integer work here, so it is ALSO reported on
                 its own (..._chain_host_scalars_ms).
At every shape a chain must give its call's bytes (a row that fails its Schnorr check over the parameters and one made from a non-signature among them).  Host
clock round synchronous calls; the sides of a comparison ALTERNATE inside one loop after a warm call of each, and the median of --reps is kept.  Stage times come
from a second pass on the development twin (StageTimer marks).  No pass / fail threshold: the numbers are written down.  Writes profiles/bbs23_timing.json.

    python tests/perf/bbs23_timing.py [--rows 64,1024,16384] [--messages 30] [--revealed 5] [--reps 7] [--out profiles/bbs23_timing.json]
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
import bbs23_model as M                    # noqa: E402
from crypto_amd import bbs_plus as BBS     # noqa: E402
from crypto_amd import bbs_23 as B23       # noqa: E402
from crypto_amd import G1 as CG1           # noqa: E402
from crypto_amd.msm import msm_segments    # noqa: E402
from crypto_amd._native import lib         # noqa: E402

R, CDL, IETF = M.R, M.CDL, M.IETF
P_LIMBS = [0xB9FEFFFFFFFFAAAB, 0x1EABFFFEB153FFFF, 0x6730D2A0F6B0F624, 0x64774B84F38512BF, 0x4B1BA7B6434BACD7, 0x1A0111EA397FE69A]
p_ = lambda a: a.ctypes.data_as(C.c_void_p)
PREFIXES = ("bbs.", "bbs23.", "msm.")
ORDER = {CDL: [0, 2, 1, 3, 2, 4], IETF: [0, 1, 2]}                   # the own points in segment order


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bbs23_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    Lm = args.messages
    rng = np.random.default_rng(271828)
    x, gamma, eta0 = rand(rng, 3)
    etas = rand(rng, Lm)
    key = M.Key(x, gamma, etas)
    key_plus = BM.Key(x, gamma, [eta0] + etas)                          # the BBS+ key of the comparison: the same generators and h_0 besides
    pts = g_times(key.params_scalars(Lm))
    h0 = g_times([eta0])[0]
    g2 = O.G2.generator()
    w = O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(x, 4)))[0]
    neg_g2 = O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(R - 1, 4)))[0]
    one = O.fp12_one()
    revealed = sorted({(j * Lm) // args.revealed for j in range(args.revealed)})
    res = {"reps": args.reps, "messages": Lm, "revealed": len(revealed), "shapes": {}}

    def make(n):
        """n rows: messages, e, s (BBS+ only), and the proofs of the three kinds from known discrete logs; per kind row n // 2 fails its Schnorr check over the
        parameters, row 1 (n > 2) comes from a non-signature"""
        d = {"e": rand(rng, n), "s": rand(rng, n), "msgs": [rand(rng, Lm) for _ in range(n)]}
        for kind in (CDL, IETF, "plus"):
            proofs = []
            for i in range(n):
                e, m, c = d["e"][i], d["msgs"][i], rand(rng, 1)[0]
                if kind == "plus":
                    a = key_plus.a(e, d["s"][i], m)
                else:
                    a = key.a(e, m)
                if n > 2 and i == 1:
                    a = (a + 1) % R
                r1, r2 = rand(rng, 2)
                if kind == CDL:
                    proofs.append(M.prove_cdl(key, a, e, m, set(revealed), r1, r2, rand(rng, 3 + Lm), c))
                elif kind == IETF:
                    proofs.append(M.prove_ietf(key, a, e, m, set(revealed), r1, rand(rng, 2 + Lm), c))
                else:
                    proofs.append(PM.prove(key_plus, a, e, d["s"][i], m, set(revealed), r1, r2, rand(rng, 4 + Lm), c))
            last = len(proofs[0].pts) - 1
            proofs[n // 2].pts[last] = (proofs[n // 2].pts[last] + 1) % R
            npts, nresp = len(proofs[0].pts), len(proofs[0].fixed)
            d[kind] = (proofs, g_times([k for p in proofs for k in p.pts]).reshape(n, npts, 12), limbs([z for p in proofs for z in p.fixed]).reshape(n, nresp, 4),
                       limbs([v for p in proofs for v in p.values]).reshape(n, Lm, 4), np.array([p.mask for p in proofs], np.uint8), limbs([p.c for p in proofs]))
        return d

    def mul_add(points, sc, addend):
        n = len(points)
        out, inf = np.zeros((n, 12), np.uint64), np.zeros(n, np.uint8)
        assert lib().dgpu_g1_mul_add_batch(p_(points), None, p_(sc), 4, None if addend is None else p_(addend), None, n, p_(out), p_(inf)) == 0
        return out

    def pairings(pa, qa, ends, n):
        out = np.zeros((n, 72), np.uint64)
        for lo in range(0, n, 4096):                                 # (the call takes at most 4096 segments)
            k = min(4096, n - lo)
            assert lib().dgpu_multi_pairing_segments(p_(pa[lo:]), p_(qa[2 * lo:]), None, 2 * k, p_(ends), k, p_(out[lo:])) == 0
        return (out == one).all(axis=1)

    def run(P, Pp, n, row, d, reps):
        rho = limbs(rand(rng, 1))[0]
        qa = np.ascontiguousarray(np.tile(np.stack([w, neg_g2]), (n, 1)))
        pair_ends = (2 * np.arange(1, n + 1)).astype(np.uint64)
        minus_one = limbs([R - 1])[0]
        e, s, msgs = limbs(d["e"]), limbs(d["s"]), limbs([v for m in d["msgs"] for v in m]).reshape(n, Lm, 4)
        xk = limbs([x])[0]

        # ---- signatures
        rows = np.zeros((n, Lm + 1, 4), np.uint64)
        rows[:, 0, 0] = 1; rows[:, 1:] = msgs
        t = limbs([pow((x + v) % R, R - 2, R) for v in d["e"]])      # (before the clock: see the docstring)
        neg_e = limbs([(R - v) % R for v in d["e"]])
        chain_b = lambda: np.ascontiguousarray(P.bases.msm_many(rows)[:, :12])      # normalised (X, Y, 1): the affine words
        sign_new = lambda: B23.sign_many(P, xk, msgs, e)
        sign_chain = lambda: mul_add(chain_b(), t, None)
        sign_plus = lambda: BBS.sign_many(Pp, xk, msgs, e, s)
        a, bad = sign_new()
        assert not bad.any() and (sign_chain() == a).all()          # the chain and the call: the same signatures
        ap, _ = sign_plus()
        a[n // 2] = pts[0]; ap[n // 2] = pts[0]                      # one signature that does not verify

        def verify_chain():
            nd = mul_add(a, neg_e, chain_b())
            pa = np.empty((n, 2, 12), np.uint64); pa[:, 0] = a; pa[:, 1] = nd
            return pairings(pa, qa, pair_ends, n).astype(np.uint8)
        each_new = lambda: B23.verify_each(P, a, e, msgs)
        batch_new = lambda: B23.verify_batch(P, a, e, msgs, rho)
        each_plus = lambda: BBS.verify_each(Pp, ap, e, s, msgs)
        batch_plus = lambda: BBS.verify_batch(Pp, ap, e, s, msgs, rho)
        want = np.ones(n, np.uint8); want[n // 2] = 0
        assert (each_new() == want).all() and (verify_chain() == want).all() and (each_plus() == want).all() and not batch_new() and not batch_plus()
        row["sign_many_ms"], row["sign_chain_ms"], row["bbs_plus_sign_many_ms"] = alternate([sign_new, sign_chain, sign_plus], reps)
        (row["verify_each_ms"], row["verify_batch_ms"], row["verify_chain_ms"], row["bbs_plus_verify_each_ms"],
         row["bbs_plus_verify_batch_ms"]) = alternate([each_new, batch_new, verify_chain, each_plus, batch_plus], reps)
        calls = {"sign_many": sign_new, "verify_each": each_new, "verify_batch": batch_new}

        # ---- proofs
        fns, names = [], []
        for kind, tag in ((CDL, "pok"), (IETF, "pok_ietf")):
            proofs, points, fixed, values, mask, chal = d[kind]
            own_n, segs = (6, 2) if kind == CDL else (3, 1)
            seg_ends = (np.stack([6 * np.arange(n) + 4, 6 * np.arange(n) + 6], axis=1).reshape(-1) if kind == CDL else 3 * np.arange(1, n + 1)).astype(np.uint64)
            host_ms = []

            def chain(kind=kind, points=points, fixed=fixed, values=values, chal=chal, own_n=own_n, segs=segs, seg_ends=seg_ends, host_ms=host_ms):
                t0 = time.perf_counter()
                # the host's scalar work: c m on the revealed entries, -c; everything else is copied as it stands
                cs = [O.limbs_to_int(v) for v in chal]
                prow = np.empty((n, Lm + 1, 4), np.uint64)
                prow[:, 0], prow[:, 1:] = chal, values
                for j in revealed:
                    prow[:, 1 + j] = limbs([c * O.limbs_to_int(v) % R for c, v in zip(cs, values[:, j])])
                own = np.empty((n, own_n, 4), np.uint64)
                if kind == CDL:
                    own[:, 0], own[:, 1], own[:, 2], own[:, 3], own[:, 4], own[:, 5] = fixed[:, 0], fixed[:, 1], limbs([(R - c) % R for c in cs]), minus_one, fixed[:, 2], minus_one
                else:
                    own[:, 0], own[:, 1], own[:, 2] = fixed[:, 0], fixed[:, 1], minus_one
                bases = np.ascontiguousarray(points[:, ORDER[kind]])
                host_ms.append((time.perf_counter() - t0) * 1e3)
                pj, pinf = P.bases.msm_many(prow, flags=True)
                sj, sinf = msm_segments(CG1, bases.reshape(-1, 12), own.reshape(-1, 4), seg_ends, flags=True)
                pairing = pairings(np.ascontiguousarray(points[:, :2]), qa, pair_ends, n)
                q, qinf = sj[segs - 1::segs], sinf[segs - 1::segs].astype(bool)
                second = np.where(pinf.astype(bool) | qinf, pinf.astype(bool) & qinf, (pj[:, :6] == q[:, :6]).all(axis=1) & (neg_fq(pj[:, 6:12]) == q[:, 6:12]).all(axis=1))
                first = sinf[0::2] != 0 if kind == CDL else np.ones(n, bool)
                a_inf = ~points[:, 0].any(axis=1)
                return np.where(a_inf, 1, np.where(~first, 2, np.where(~second, 3, np.where(~pairing, 4, 0)))).astype(np.uint8)

            each_fn, batch_fn = (B23.pok_verify_each, B23.pok_verify_batch) if kind == CDL else (B23.pok_ietf_verify_each, B23.pok_ietf_verify_batch)
            want = np.array([p.status(key) for p in proofs], np.uint8)
            # the batch that is timed is the one that VERIFIES (a failing G1 equation returns before the pairing): the valid rows, the two others replaced by row 0
            good = [i if want[i] == 0 else 0 for i in range(n)]
            gp, gf, gv, gm, gc = points[good], fixed[good], values[good], mask[good], chal[good]
            pe = lambda f=each_fn, a_=(points, fixed, values, mask, chal): f(P, *a_)
            pb = lambda f=batch_fn, a_=(gp, gf, gv, gm, gc): f(P, *a_, rho)
            assert want[n // 2] == 3 and (n <= 2 or want[1] == 4) and int((want != 0).sum()) == (2 if n > 2 else 1)
            assert (pe() == want).all() and (chain() == want).all() and pb() and not batch_fn(P, points, fixed, values, mask, chal, rho)
            host_ms.clear()
            fns += [pe, pb, chain]; names += [tag + "_verify_each_ms", tag + "_verify_batch_ms", tag + "_chain_ms"]
            row[tag + "_chain_host_scalars_ms"] = host_ms                   # (filled by the loop below; reduced to its median afterwards)
            calls[tag + "_verify_each"], calls[tag + "_verify_batch"] = pe, pb
        proofs, points, fixed, values, mask, chal = d["plus"]
        want = np.array([p.status(key_plus) for p in proofs], np.uint8)
        good = [i if want[i] == 0 else 0 for i in range(n)]
        plus_each = lambda: BBS.pok_verify_each(Pp, points, fixed, values, mask, chal)
        plus_batch = lambda: BBS.pok_verify_batch(Pp, points[good], fixed[good], values[good], mask[good], chal[good], rho)
        assert (plus_each() == want).all() and plus_batch()
        fns += [plus_each, plus_batch]; names += ["bbs_plus_pok_verify_each_ms", "bbs_plus_pok_verify_batch_ms"]
        for name, ms in zip(names, alternate(fns, reps)):
            row[name] = ms
        for tag in ("pok", "pok_ietf"):
            row[tag + "_chain_host_scalars_ms"] = float(np.median(row[tag + "_chain_host_scalars_ms"]))
        return calls

    for n in [int(v) for v in args.rows.split(",")]:
        row = {}
        d = make(n)
        with B23.Params23(pts[0], pts[1:], g2, w) as P, BBS.Params(pts[0], h0, pts[1:], g2, w) as Pp:
            run(P, Pp, n, row, d, args.reps)
        with ca.twin():                                             # the stage timers live on the twin: parameters of its own
            with B23.Params23(pts[0], pts[1:], g2, w) as P, BBS.Params(pts[0], h0, pts[1:], g2, w) as Pp:
                calls = run(P, Pp, n, {}, d, 1)                     # (the same checks against the twin; its timings are not kept)
                for name, fn in calls.items():
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
