"""The four accumulator proof calls (dgpu_accumulator_membership_proofs_verify_each_g1 / _verify_batch_g1 and the two non-membership ones) on one device, beside
the same work done the only way the library allowed before them — the caller's chain of public calls with a PCIe round trip and host scalar work between each —
on the same box in the same process:
  chain    host: the own scalars (z1, -z2, -c, -1), respectively (s_d, -c, -1 | s_r, -s_y, -s_d, -c, -1), the gather of the segments' bases with the shared
           V, P, Q copied into every row
           dgpu_msm_g1_segments over the n (2 n) segments -> dgpu_multi_pairing_segments over the n segments ((A', pk), (Abar, -P~)) (at most 4096 segments a
           call: longer batches go in pieces); host: the zero-point checks and the order of the checks.
           The host scalar work counts inside the clock, because the new call replaces it; it is Python-integer work here where a native caller has field
           arithmetic, so it is ALSO reported on its own (chain_host_scalars_ms) and the chain's time can be read with and without it.
At every shape the chain must give the call's statuses (a row that fails its Schnorr check and one made from a forged witness among them).  Host clock round
synchronous calls; the sides of a comparison ALTERNATE inside one loop after a warm call of each, and the median of --reps is kept.  Stage times come from a second
pass on the development twin (StageTimer marks).  No pass / fail threshold: the numbers are written down.  Writes profiles/acc_pok_timing.json.

    python tests/perf/acc_pok_timing.py [--rows 64,1024,16384] [--reps 7] [--out profiles/acc_pok_timing.json]
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
import acc_pok_model as AM                 # noqa: E402
from bbs_model import R                    # noqa: E402
from crypto_amd import accumulator as ACC  # noqa: E402
from crypto_amd import G1 as CG1           # noqa: E402
from crypto_amd.msm import msm_segments    # noqa: E402
from crypto_amd._native import lib         # noqa: E402

p_ = lambda a: a.ctypes.data_as(C.c_void_p)
PREFIXES = ("acc.", "bbs.", "msm.")
NAMES = {0: "membership", 1: "non_membership"}


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def g_times(scalars):
    out, inf = O.g1_scale_batch(np.tile(O.G1.generator(), (len(scalars), 1)), limbs([k % R for k in scalars]), threads=16)
    out[inf.astype(bool)] = 0
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acc_pok_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    rng = np.random.default_rng(141421)
    key = AM.Key(*rand(rng, 4))
    V, Pp, Q = g_times([key.v, key.pi, key.q])
    g2 = O.G2.generator()
    pk = O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(key.alpha, 4)))[0]
    neg_g2 = O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(R - 1, 4)))[0]
    one = O.fp12_one()
    res = {"reps": args.reps, "shapes": {}}

    def make(kind, n):
        """n proofs from known discrete logs; row n // 2 fails its (long) Schnorr check, row 1 (n > 2) comes from a forged witness"""
        proofs = []
        for i in range(n):
            forged = 1 if n > 2 and i == 1 else 0
            if kind == 0:
                y, r, b_r, b_y, c = rand(rng, 5)
                proofs.append(AM.prove_membership(key, key.membership_witness(y) + forged, y, r, b_r, b_y, c))
            else:
                y, d, r, b_r, b_y, b_d, c = rand(rng, 7)
                proofs.append(AM.prove_non_membership(key, key.non_membership_witness(y, d) + forged, d, y, r, b_r, b_y, b_d, c))
        t = 2 if kind == 0 else 3
        proofs[n // 2].pts[t] = (proofs[n // 2].pts[t] + 1) % R
        npts, nresp = (3, 2) if kind == 0 else (5, 3)
        points = g_times([k for p in proofs for k in p.pts]).reshape(n, npts, 12)
        return proofs, points, limbs([z for p in proofs for z in p.resp]).reshape(n, nresp, 4), limbs([p.c for p in proofs])

    def run(kind, vkey, n, row, data):
        proofs, points, resp, chal = data
        rho = limbs(rand(rng, 1))[0]
        qa = np.ascontiguousarray(np.tile(np.stack([pk, neg_g2]), (n, 1)))
        pair_ends = (2 * np.arange(1, n + 1)).astype(np.uint64)
        minus_one = limbs([R - 1])[0]
        if kind == 0:
            seg_ends = (4 * np.arange(1, n + 1)).astype(np.uint64)
        else:
            seg_ends = np.stack([8 * np.arange(n) + 3, 8 * np.arange(n) + 8], axis=1).reshape(-1).astype(np.uint64)
        host_ms = []
        neg = lambda a: limbs([(R - O.limbs_to_int(v) % R) % R for v in a])

        def chain():
            t0 = time.perf_counter()
            # the host's scalar work: the negations; everything else is copied as it stands
            nc = neg(chal)
            if kind == 0:
                own = np.empty((n, 4, 4), np.uint64)
                own[:, 0], own[:, 1], own[:, 2], own[:, 3] = resp[:, 0], neg(resp[:, 1]), nc, minus_one
                bases = np.empty((n, 4, 12), np.uint64)
                bases[:, 0], bases[:, 1], bases[:, 2], bases[:, 3] = V, points[:, 0], points[:, 1], points[:, 2]
            else:
                own = np.empty((n, 8, 4), np.uint64)
                own[:, 0], own[:, 1], own[:, 2], own[:, 3], own[:, 4], own[:, 5], own[:, 6], own[:, 7] = \
                    resp[:, 2], nc, minus_one, resp[:, 0], neg(resp[:, 1]), neg(resp[:, 2]), nc, minus_one
                bases = np.empty((n, 8, 12), np.uint64)
                bases[:, 0], bases[:, 1], bases[:, 2], bases[:, 3], bases[:, 4], bases[:, 5], bases[:, 6], bases[:, 7] = \
                    Q, points[:, 2], points[:, 4], V, points[:, 0], Pp, points[:, 1], points[:, 3]
            host_ms.append((time.perf_counter() - t0) * 1e3)
            _, sinf = msm_segments(CG1, bases.reshape(-1, 12), own.reshape(-1, 4), seg_ends, flags=True)
            pa = np.ascontiguousarray(points[:, :2])
            out = np.zeros((n, 72), np.uint64)
            for lo in range(0, n, 4096):                             # (the call takes at most 4096 segments)
                k = min(4096, n - lo)
                assert lib().dgpu_multi_pairing_segments(p_(pa[lo:]), p_(qa[2 * lo:]), None, 2 * k, p_(pair_ends), k, p_(out[lo:])) == 0
            pairing = (out == one).all(axis=1)
            w_inf = ~points[:, 0].any(axis=1)
            if kind == 0:
                return np.where(w_inf, 1, np.where(sinf == 0, 2, np.where(~pairing, 3, 0))).astype(np.uint8)
            j_inf = ~points[:, 2].any(axis=1)
            return np.where(w_inf, 1, np.where(j_inf, 2, np.where(sinf[0::2] == 0, 3, np.where(sinf[1::2] == 0, 4, np.where(~pairing, 5, 0))))).astype(np.uint8)

        each_fn = ACC.membership_proofs_verify_each if kind == 0 else ACC.non_membership_proofs_verify_each
        batch_fn = ACC.membership_proofs_verify_batch if kind == 0 else ACC.non_membership_proofs_verify_batch
        head = (vkey, V) if kind == 0 else (vkey, V, Pp, Q)
        want = np.array([p.status(key) for p in proofs], np.uint8)
        each_new = lambda: each_fn(*head, points, resp, chal)
        batch_bad = lambda: batch_fn(*head, points, resp, chal, rho)
        # the batch that is timed is the one that VERIFIES (a failing G1 equation returns before the pairing): the valid rows, the two others replaced by row 0
        good = [i if want[i] == 0 else 0 for i in range(n)]
        gp, gr, gc = points[good], resp[good], chal[good]
        batch_new = lambda: batch_fn(*head, gp, gr, gc, rho)
        long_check, pairing_check = (2, 3) if kind == 0 else (4, 5)
        assert want[n // 2] == long_check and (n <= 2 or want[1] == pairing_check) and int((want != 0).sum()) == (2 if n > 2 else 1)
        assert (each_new() == want).all() and (chain() == want).all() and not batch_bad() and batch_new()      # the chain and the call: the same statuses
        host_ms.clear()
        row["verify_each_ms"], row["verify_batch_ms"], row["verify_batch_refusing_ms"], row["chain_ms"] = alternate([each_new, batch_new, batch_bad, chain], args.reps)
        row["chain_host_scalars_ms"] = float(np.median(host_ms))
        return each_new, batch_new

    for n in [int(v) for v in args.rows.split(",")]:
        for kind in (0, 1):
            row = {}
            data = make(kind, n)
            run(kind, ACC.VerifierKey(pk, g2), n, row, data)
            with ca.twin():                                         # the stage timers live on the twin
                calls = run(kind, ACC.VerifierKey(pk, g2), n, {}, data)
                for name, fn in zip(("verify_each", "verify_batch"), calls):
                    ca.prof.enable(True); ca.prof.reset()
                    for _ in range(args.reps):
                        fn()
                    st = ca.prof.read()
                    ca.prof.enable(False)
                    row[name + "_stages_ms"] = {k: v[0] / args.reps for k, v in st.items() if k.startswith(PREFIXES)}
            res["shapes"].setdefault("n=%d" % n, {})[NAMES[kind]] = row
            print(n, NAMES[kind], json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
