"""dgpu_accumulator_update_witnesses_g1 on one device: the whole call and its stages (StageTimer marks acc.* on the development twin) at
m in {2^10, 2^14, 2^17} holders x n_add = n_rem in {8, 512}; one chunk per element against the automatic split at m = 64 with lists of 2^14; and, as the
yardstick of the G1 half, two dgpu_g1_mul_add_batch calls of the same m (g_i V, then that plus f_i C_i).  Host clock round synchronous calls, median of
--reps after one warm call.  No pass / fail threshold: these are the first numbers anybody has for this call, and the constants of
crypto_amd/csrc/acc_launch.hip.h (ACC_FILL_LANES, ACC_MIN_CHUNK, ACC_SHARE_LANES) are to be tuned from them.  Writes profiles/acc_update_timing.json.

    python tests/perf/acc_update_timing.py [--sizes 1024,16384,131072] [--lists 8,512] [--reps 5] [--out profiles/acc_update_timing.json]
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
from crypto_amd import accumulator as ACC  # noqa: E402
from crypto_amd._native import lib         # noqa: E402

p_ = lambda a: a.ctypes.data_as(C.c_void_p)


def med(fn, reps):
    fn()                                                          # warm: the slot's workspace grows once
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def inputs(m, n, seed):
    """m holders (points of the group with known discrete logs; timing does not need valid witnesses), lists of n additions and n removals"""
    k0, d = O.rand_scalars(seed, 1)[0], O.rand_scalars(seed + 1, 1)[0]
    pts = O.G1.gen_seq(k0, d, m + 1, threads=16)
    sc = O.rand_scalars(seed + 2, m + 2 * n + 1)
    sc[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)                     # below r
    return dict(C=np.ascontiguousarray(pts[:m]), V=np.ascontiguousarray(pts[m]), ys=np.ascontiguousarray(sc[:m]), adds=np.ascontiguousarray(sc[m:m + n]),
                rems=np.ascontiguousarray(sc[m + n:m + 2 * n]), alpha=np.ascontiguousarray(sc[m + 2 * n]))


def call(I):
    return ACC.update_witnesses(I["adds"], I["rems"], I["alpha"], I["ys"], I["C"], I["V"])


def stages(I, reps):
    """per-stage milliseconds per call, from the twin's event timers"""
    with ca.twin():
        call(I)
        ca.prof.enable(True); ca.prof.reset()
        for _ in range(reps):
            call(I)
        rows = ca.prof.read()
        ca.prof.enable(False)
    return {k: v[0] / max(v[1], 1) for k, v in rows.items() if k.startswith("acc.") or k.startswith("fixed.")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,16384,131072")
    ap.add_argument("--lists", default="8,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acc_update_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    L = lib()
    res = {"reps": args.reps, "shapes": {}, "split": {}}
    for m in [int(x) for x in args.sizes.split(",")]:
        for n in [int(x) for x in args.lists.split(",")]:
            I = inputs(m, n, 7 * m + n)
            d, (w, inf) = call(I)
            f, g = ACC.update_factors(I["adds"], I["rems"], I["alpha"], I["ys"])
            assert (f == d).all()
            # the G1 half through the folding-step entry point: T = g V, then T + f C
            Vm = np.ascontiguousarray(np.tile(I["V"], (m, 1)))
            T, Tinf, out, oinf = np.zeros((m, 12), np.uint64), np.zeros(m, np.uint8), np.zeros((m, 12), np.uint64), np.zeros(m, np.uint8)
            def two_mul_adds():
                assert L.dgpu_g1_mul_add_batch(p_(Vm), None, p_(g), 4, None, None, m, p_(T), p_(Tinf)) == 0
                assert L.dgpu_g1_mul_add_batch(p_(I["C"]), None, p_(f), 4, p_(T), p_(Tinf), m, p_(out), p_(oinf)) == 0
            row = {"whole_call_ms": med(lambda: call(I), args.reps), "factors_call_ms": med(lambda: ACC.update_factors(I["adds"], I["rems"], I["alpha"], I["ys"]), args.reps),
                   "two_mul_add_batch_ms": med(two_mul_adds, args.reps), "stages_ms": stages(I, args.reps)}
            assert (out == w).all() and (oinf == inf).all()       # the same points either way
            res["shapes"]["m=%d,n=%d" % (m, n)] = row
            print(m, n, json.dumps(row), flush=True)
    # few holders, long lists: one chunk per element against the automatic split
    I = inputs(64, 1 << 14, 99)
    want = call(I)
    with ca.twin() as T:
        for name, k in (("K=1", 1), ("automatic", 0)):
            assert T.dgpu_dev_set_acc_split(k) == 0
            ms = med(lambda: ACC.update_factors(I["adds"], I["rems"], I["alpha"], I["ys"]), args.reps)
            got = call(I)
            assert (got[0] == want[0]).all() and (got[1][0] == want[1][0]).all()
            res["split"][name] = {"factors_call_ms": ms, "chunks": int(T.dgpu_dev_get_acc_split()), "stages_ms": stages(I, args.reps)}
            print("m=64 n=16384", name, json.dumps(res["split"][name]), flush=True)
        T.dgpu_dev_set_acc_split(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
