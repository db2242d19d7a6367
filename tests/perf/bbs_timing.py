"""dgpu_bbs_plus_sign_many_g1, dgpu_bbs_plus_verify_each_g1 and dgpu_bbs_plus_verify_batch_g1 on one device, each beside the same work done the only way the
library allowed before them — the caller's chain of three calls with a PCIe round trip between each — on the same box in the same process:
  sign     dgpu_msm_g1_handle_many over the rows (1, s_i, m_i ..) -> dgpu_g1_mul_add_batch with the inverses 1 / (x + e_i).  The inverses are made BEFORE the clock
           starts (a caller has a batch inversion for them; Python has not), so the chain is timed without a step the new call contains.
  verify   dgpu_msm_g1_handle_many -> dgpu_g1_mul_add_batch ((-e_i) A_i + b_i) -> dgpu_multi_pairing_segments over the n segments ((A_i, w), (-d_i, -g2)), the
           verdict of a row being "its GT element is one" (that call takes at most 4096 segments: longer batches go in pieces).  verify_each is timed against it, and so is verify_batch (one verdict, where the chain gives n).
At every shape the chain must give the call's signatures and verdicts.  Host clock round synchronous calls; the two sides of a comparison ALTERNATE inside one
loop after a warm call of each, and the median of --reps is kept.  Stage times come from a second pass on the development twin (StageTimer marks).  No pass /
fail threshold: both numbers are written down.  Writes profiles/bbs_timing.json.

    python tests/perf/bbs_timing.py [--rows 64,1024,16384] [--messages 30] [--reps 7] [--out profiles/bbs_timing.json]
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
from crypto_amd import bbs_plus as BBS     # noqa: E402
from crypto_amd._native import lib         # noqa: E402

R = BM.R
p_ = lambda a: a.ctypes.data_as(C.c_void_p)
PREFIXES = ("bbs.", "msm.")


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def scalars(seed, n):
    sc = O.rand_scalars(seed, n)
    sc[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)                     # below r
    return np.ascontiguousarray(sc)


def ints(a):
    return [O.limbs_to_int(row) for row in np.asarray(a).reshape(-1, 4)]


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bbs_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    Lm = args.messages
    G = O.G1
    key = scalars(1, Lm + 4)
    x = O.limbs_to_int(key[0])
    gen = np.tile(G.generator(), (Lm + 2, 1))
    pts, _ = O.g1_scale_batch(gen, key[1:Lm + 3], threads=16)
    g2 = O.G2.generator()
    w = O.G2.to_affine(O.G2.mul(g2, key[0]))[0]
    neg_g2 = O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(R - 1, 4)))[0]
    one = O.fp12_one()
    res = {"reps": args.reps, "messages": Lm, "shapes": {}}

    def chain_b(P, rows):
        jac = P.bases.msm_many(rows)
        return np.ascontiguousarray(jac[:, :12])                 # normalised (X, Y, 1): the affine words

    def mul_add(points, sc, addend):
        n = len(points)
        out, inf = np.zeros((n, 12), np.uint64), np.zeros(n, np.uint8)
        rc = lib().dgpu_g1_mul_add_batch(p_(points), None, p_(sc), 4, None if addend is None else p_(addend), None, n, p_(out), p_(inf))
        assert rc == 0
        return out

    def run(P, n, row):
        e, s, msgs = scalars(10 + n, n), scalars(20 + n, n), scalars(30 + n, n * Lm).reshape(n, Lm, 4)
        rows = np.zeros((n, Lm + 2, 4), np.uint64)
        rows[:, 0, 0] = 1; rows[:, 1] = s; rows[:, 2:] = msgs
        t = limbs([pow((x + v) % R, R - 2, R) for v in ints(e)])     # (before the clock: see the docstring)
        neg_e = limbs([(R - v) % R for v in ints(e)])
        rho = scalars(99, 1)[0]
        qa = np.ascontiguousarray(np.tile(np.stack([w, neg_g2]), (n, 1)))
        ends = (2 * np.arange(1, n + 1)).astype(np.uint64)

        sign_new = lambda: BBS.sign_many(P, key[0], msgs, e, s)
        sign_chain = lambda: mul_add(chain_b(P, rows), t, None)
        a, bad = sign_new()
        assert not bad.any() and (sign_chain() == a).all()          # the chain and the call: the same signatures
        a[n // 2] = pts[0]                                          # one signature that does not verify

        def verify_chain():
            nd = mul_add(a, neg_e, chain_b(P, rows))
            pa = np.empty((n, 2, 12), np.uint64); pa[:, 0] = a; pa[:, 1] = nd
            out = np.zeros((n, 72), np.uint64)
            for lo in range(0, n, 4096):                             # (the call takes at most 4096 segments)
                k = min(4096, n - lo)
                assert lib().dgpu_multi_pairing_segments(p_(pa[lo:]), p_(qa[2 * lo:]), None, 2 * k, p_(ends), k, p_(out[lo:])) == 0
            return (out == one).all(axis=1).astype(np.uint8)
        each_new = lambda: BBS.verify_each(P, a, e, s, msgs)
        batch_new = lambda: BBS.verify_batch(P, a, e, s, msgs, rho)
        want = np.ones(n, np.uint8); want[n // 2] = 0
        assert (each_new() == want).all() and (verify_chain() == want).all() and not batch_new()
        row["sign_many_ms"], row["sign_chain_ms"] = alternate([sign_new, sign_chain], args.reps)
        row["verify_each_ms"], row["verify_batch_ms"], row["verify_chain_ms"] = alternate([each_new, batch_new, verify_chain], args.reps)
        return sign_new, each_new, batch_new

    for n in [int(v) for v in args.rows.split(",")]:
        row = {}
        with BBS.Params(pts[0], pts[1], pts[2:], g2, w) as P:
            run(P, n, row)
        with ca.twin():                                             # the stage timers live on the twin: parameters of its own
            with BBS.Params(pts[0], pts[1], pts[2:], g2, w) as P:
                calls = run(P, n, {})
                for name, fn in zip(("sign_many", "verify_each", "verify_batch"), calls):
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
