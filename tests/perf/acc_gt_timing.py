"""The four accumulator proof calls with a GT commitment (dgpu_accumulator_gt_membership_proofs_verify_each_g1 / _verify_batch_g1 and the two non-membership ones,
libdock_gpu_acc_gt.so) on one device, beside the same work done the only way the library allowed before them — the caller's chain of public calls with a PCIe
round trip and host scalar work between each — and beside the CDH calls of DESIGN.md 12.3 at the same n, on the same box in the same process:
  chain    host: the 17 (27) own scalars of every row (negations, two sums), the gather of the segments' bases with the shared V, X, Y, Z [, K, P] copied into
           every row
           dgpu_msm_g1_segments over the 6 n (8 n) segments -> host: the last two sums of every row as the pairing's sides -> dgpu_multi_pairing_segments over
           the n segments ((q, pk), (p, P~)) (at most 4096 segments a call: longer batches go in pieces); host: the comparison with R_E and the order of the checks.
           The host scalar work counts inside the clock, because the new call replaces it; it is Python-integer work here where a native caller has field
           arithmetic, so it is ALSO reported on its own (chain_host_scalars_ms) and the chain's time can be read with and without it.
  cdh      dgpu_accumulator_membership_proofs_verify_each_g1 / _verify_batch_g1 (respectively non-membership) over n valid CDH proofs: what the GT form costs
           over the CDH form
At every shape the chain must give the call's statuses (a row that fails a Schnorr check, one from a forged witness and one whose R_E is moved among them).
256 distinct proofs are made; larger shapes take them in turn.  Host clock round synchronous calls; the sides of a comparison ALTERNATE inside one loop after a
warm call of each, and the median of --reps is kept.  Stage times come from a second pass on the development build (StageTimer marks).  No pass / fail
threshold: the numbers are written down.  Writes profiles/acc_gt_timing.json.

    python tests/perf/acc_gt_timing.py [--rows 64,1024,16384] [--reps 7] [--out profiles/acc_gt_timing.json]
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
import crypto_amd as ca                        # noqa: E402
import oracle_c as O                           # noqa: E402
import acc_gt_model as GM                      # noqa: E402
import acc_pok_model as AM                     # noqa: E402
from bbs_model import R                        # noqa: E402
from crypto_amd import accumulator as ACC      # noqa: E402
from crypto_amd import accumulator_gt as AGT   # noqa: E402
from crypto_amd import G1 as CG1               # noqa: E402
from crypto_amd.msm import msm_segments        # noqa: E402
from crypto_amd._native import lib, twin       # noqa: E402

p_ = lambda a: a.ctypes.data_as(C.c_void_p)
PREFIXES = ("acc.", "bbs.", "msm.", "gt.")
NAMES = {0: "membership", 1: "non_membership"}
DISTINCT = 256


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acc_gt_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    rng = np.random.default_rng(173205)
    key = GM.Key(*rand(rng, 7))
    names = ("v", "pi", "x", "yk", "z", "k")
    sh = dict(zip(names, g_times([getattr(key, n) for n in names])))
    g2 = O.G2.generator()
    pk = O.G2.to_affine(O.G2.mul(g2, O.int_to_limbs(key.alpha, 4)))[0]
    e_gen = O.final_exponentiation(O.multi_miller_loop(O.G1.generator().reshape(1, 12), g2.reshape(1, 24)))
    gt_of = lambda log: np.asarray(O.fp12_pow(e_gen, log % R), np.uint64) if log % R else np.asarray(O.fp12_one(), np.uint64)
    one = np.asarray(O.fp12_one(), np.uint64)
    vkey = ACC.VerifierKey(pk, g2)
    # the CDH side: its own key over the same pk
    ckey = AM.Key(key.alpha, key.pi, rand(rng, 1)[0], key.v)
    cV, cP, cQ = g_times([ckey.v, ckey.pi, ckey.q])
    res = {"reps": args.reps, "distinct_proofs": DISTINCT, "shapes": {}}

    def distinct(kind):
        """256 proofs from known discrete logs; row 2 fails a Schnorr check, row 1 comes from a forged witness, row 3 has its R_E moved by a GT factor"""
        proofs = []
        for i in range(DISTINCT):
            proofs.append(GM.prove_row(key, kind, rand(rng, 1)[0], rand(rng, 1)[0] or 1, rand(rng, 12), rand(rng, 1)[0], forged=(i == 1)))
        proofs[2] = GM.tamper(proofs[2], "R_delta_sigma")
        proofs[3] = GM.tamper(proofs[3], "R_E")
        points = g_times([k for p in proofs for k in p.pts]).reshape(DISTINCT, GM.NPTS[kind], 12)
        r_e = np.stack([gt_of(p.re) for p in proofs])
        return proofs, points, r_e, limbs([z for p in proofs for z in p.resp]).reshape(DISTINCT, GM.NRESP[kind], 4), limbs([p.c for p in proofs])

    def distinct_cdh(kind):
        proofs = []
        for i in range(DISTINCT):
            if kind == 0:
                y, r, b_r, b_y, c = rand(rng, 5)
                proofs.append(AM.prove_membership(ckey, ckey.membership_witness(y), y, r, b_r, b_y, c))
            else:
                y, d, r, b_r, b_y, b_d, c = rand(rng, 7)
                proofs.append(AM.prove_non_membership(ckey, ckey.non_membership_witness(y, d), d, y, r, b_r, b_y, b_d, c))
        npts, nresp = (3, 2) if kind == 0 else (5, 3)
        return g_times([k for p in proofs for k in p.pts]).reshape(DISTINCT, npts, 12), limbs([z for p in proofs for z in p.resp]).reshape(DISTINCT, nresp, 4), limbs([p.c for p in proofs])

    def run(kind, n, row, data, cdh):
        proofs, points, r_e, resp, chal = data
        idx = np.arange(n) % DISTINCT
        # only the first turn carries the three bad rows: later turns take row 0 in their place
        idx[(idx >= 1) & (idx <= 3) & (np.arange(n) >= DISTINCT)] = 0
        want = np.array([proofs[i].status(key) for i in idx], np.uint8)
        points, r_e, resp, chal = (np.ascontiguousarray(a[idx]) for a in (points, r_e, resp, chal))
        rho = limbs(rand(rng, 1))[0]
        J, segs = GM.CHECKS[kind], GM.CHECKS[kind] + 2
        tags = {"v": 1000, "pi": 1001, "x": 1002, "yk": 1003, "z": 1004, "k": 1005}
        by_tag = {t: sh[name] for name, t in tags.items()}
        layout = GM.Proof(kind, list(range(GM.NPTS[kind])), 0, [0] * GM.NRESP[kind], 0).bases(GM.Key(0, 0, 0, 0, 0, 0, 0), **tags)
        no = len(layout)
        seg_ends = (no * np.arange(n)[:, None] + np.array(GM.SEG_ENDS[kind])[None, :]).reshape(-1).astype(np.uint64)
        qa = np.ascontiguousarray(np.tile(np.stack([pk, g2]), (n, 1)))
        pair_ends = (2 * np.arange(1, n + 1)).astype(np.uint64)
        minus_one = limbs([R - 1])[0]
        host_ms = []
        ints = lambda a: [O.limbs_to_int(v) % R for v in a]
        neg = lambda a: limbs([(R - v) % R for v in ints(a)])
        neg_sum = lambda a, b: limbs([(2 * R - x - y) % R for x, y in zip(ints(a), ints(b))])
        S = GM

        def chain():
            t0 = time.perf_counter()
            # the host's scalar work: the negations and the two sums; everything else is copied as it stands
            nc = neg(chal)
            four = [resp[:, S.S_SIGMA], nc, minus_one, resp[:, S.S_RHO], nc, minus_one, resp[:, S.S_Y], neg(resp[:, S.S_DSIGMA]), minus_one,
                    resp[:, S.S_Y], neg(resp[:, S.S_DRHO]), minus_one]
            pq = [resp[:, S.S_Y], neg_sum(resp[:, S.S_DSIGMA], resp[:, S.S_DRHO]), nc]
            q = [neg_sum(resp[:, S.S_SIGMA], resp[:, S.S_RHO]), chal]
            if kind == 0:
                cols = four + pq + q
            else:
                cols = [resp[:, S.S_U], resp[:, S.S_V], nc, minus_one, resp[:, S.S_W], resp[:, S.S_U], nc, minus_one] + four + pq + [chal, neg(resp[:, S.S_V])] + q
            own = np.empty((n, no, 4), np.uint64)
            bases = np.empty((n, no, 12), np.uint64)
            for t, (col, src) in enumerate(zip(cols, layout)):
                own[:, t] = col
                bases[:, t] = by_tag[src] if src >= 1000 else points[:, src]
            host_ms.append((time.perf_counter() - t0) * 1e3)
            sums, sinf = msm_segments(CG1, bases.reshape(-1, 12), own.reshape(-1, 4), seg_ends, flags=True)
            sums, sinf = sums.reshape(n, segs, 18), sinf.reshape(n, segs)
            # (X, Y, 1): the affine point is the first 12 words; an identity side is skipped by its flag
            pa = np.ascontiguousarray(np.stack([sums[:, J + 1, :12], sums[:, J, :12]], axis=1))
            skip = np.ascontiguousarray(np.stack([sinf[:, J + 1], sinf[:, J]], axis=1).astype(np.uint8))
            out = np.zeros((n, 72), np.uint64)
            for lo in range(0, n, 4096):                             # (the call takes at most 4096 segments)
                k = min(4096, n - lo)
                assert lib().dgpu_multi_pairing_segments(p_(pa[lo:]), p_(qa[2 * lo:]), p_(skip[lo:]), 2 * k, p_(pair_ends), k, p_(out[lo:])) == 0
            pairing = (out == r_e).all(axis=1)
            st = np.where(pairing, 0, J + 1)
            for j in reversed(range(J)):
                st = np.where(sinf[:, j] == 0, j + 1, st)
            return st.astype(np.uint8)

        prk = np.stack([sh["x"], sh["yk"], sh["z"]] + ([sh["k"]] if kind == 1 else []))
        head = (vkey, sh["v"], prk) if kind == 0 else (vkey, sh["v"], sh["pi"], prk)
        each_fn = AGT.membership_proofs_verify_each if kind == 0 else AGT.non_membership_proofs_verify_each
        batch_fn = AGT.membership_proofs_verify_batch if kind == 0 else AGT.non_membership_proofs_verify_batch
        each_new = lambda: each_fn(*head, points, r_e, resp, chal)
        batch_bad = lambda: batch_fn(*head, points, r_e, resp, chal, rho)
        # the batch that is timed is the one that VERIFIES: the valid rows, the others replaced by row 0
        good = [i if want[i] == 0 else 0 for i in range(n)]
        gp, gg, gr, gc = points[good], r_e[good], resp[good], chal[good]
        batch_new = lambda: batch_fn(*head, gp, gg, gr, gc, rho)
        # ... and one that fails in GT alone (its G1 equation holds): the whole path, with a refusal at the end
        pair_only = [i if want[i] in (0, J + 1) else 0 for i in range(n)]
        pp, pg, pr, pc = points[pair_only], r_e[pair_only], resp[pair_only], chal[pair_only]
        batch_gt_bad = lambda: batch_fn(*head, pp, pg, pr, pc, rho)
        assert sorted(set(want.tolist())) == [0, GM.TAMPERS[kind]["R_delta_sigma"], J + 1] and int((want != 0).sum()) == 3
        assert (each_new() == want).all() and (chain() == want).all() and not batch_bad() and batch_new() and not batch_gt_bad()      # the chain and the call: the same statuses
        host_ms.clear()
        # the CDH calls of 12.3 over n valid proofs of theirs
        cpts, cresp, cchal = (np.ascontiguousarray(a[np.arange(n) % DISTINCT]) for a in cdh)
        chead = (vkey, cV) if kind == 0 else (vkey, cV, cP, cQ)
        ceach_fn = ACC.membership_proofs_verify_each if kind == 0 else ACC.non_membership_proofs_verify_each
        cbatch_fn = ACC.membership_proofs_verify_batch if kind == 0 else ACC.non_membership_proofs_verify_batch
        cdh_each = lambda: ceach_fn(*chead, cpts, cresp, cchal)
        cdh_batch = lambda: cbatch_fn(*chead, cpts, cresp, cchal, rho)
        assert not cdh_each().any() and cdh_batch()
        (row["verify_each_ms"], row["verify_batch_ms"], row["verify_batch_refusing_g1_ms"], row["verify_batch_refusing_gt_ms"], row["chain_ms"], row["cdh_verify_each_ms"],
         row["cdh_verify_batch_ms"]) = alternate([each_new, batch_new, batch_bad, batch_gt_bad, chain, cdh_each, cdh_batch], args.reps)
        row["chain_host_scalars_ms"] = float(np.median(host_ms))
        row["chain_less_host_scalars_ms"] = row["chain_ms"] - row["chain_host_scalars_ms"]
        return each_new, batch_new

    data = {kind: distinct(kind) for kind in (0, 1)}
    cdh = {kind: distinct_cdh(kind) for kind in (0, 1)}
    for n in [int(v) for v in args.rows.split(",")]:
        for kind in (0, 1):
            row = {}
            run(kind, n, row, data[kind], cdh[kind])
            with twin(acc_gt=True):                                 # the stage timers live on the development build
                calls = run(kind, n, {}, data[kind], cdh[kind])
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
