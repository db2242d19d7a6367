"""Timing driver (GPU box): dgpu_msm_g*_handle_many against the two ways the same rows can be computed without it, on one box in one run.
Per shape (G1 and G2, n in NS, m in MS), median / min / max of REPS host-clock-synchronised repetitions of
  (a) many      one dgpu_msm_*_handle_many call
  (b) singles   m dgpu_msm_*_handle calls from one thread
  (c) singles6  the same m calls spread over six threads in flight (the in-flight count bench.py uses)
plus one pass of the CPU oracle's m MSMs on 16 threads for orientation (rows beyond ORACLE_TERMS terms are extrapolated from the first rows and marked).
(b) and (c) use entry points that predate the many-row call: they are the baseline.  Writes profiles/msm_many_timing.json and prints a table; `wins`
is (a).max < (c).min, i.e. faster by more than the spread of the two.  ONE=g1:1024:32 runs a single many-call of that shape and exits (for a kernel trace)."""
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import crypto_amd as ca
from crypto_amd._native import lib
import oracle_c as O
import util as U

NS = [int(x) for x in os.environ.get("NS", "4,16,32,128,1024").split(",")]
MS = [int(x) for x in os.environ.get("MS", "16,256,1024,4096").split(",")]
REPS = int(os.environ.get("REPS", "7"))
ORACLE_TERMS = 1 << 18
ca.init(0)
lib().dgpu_set_min_gpu_n(1)
vp = lambda a: a.ctypes.data_as(C.c_void_p)


def timed(fn, reps=REPS):
    fn()                                                   # warm: workspaces, table
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def shape(curve, G, db, bases, n, m, pool):
    sc = O.rand_scalars(1000 * n + m, m * n).reshape(m, n, 4)
    many = curve.fn("dgpu_msm_%s_handle_many"); one = curve.fn("dgpu_msm_%s_handle")
    out = np.zeros((m, curve.JW), np.uint64); out1 = np.zeros((m, curve.JW), np.uint64)
    sp = [C.c_void_p(sc.ctypes.data + 32 * n * j) for j in range(m)]
    op = [C.c_void_p(out1.ctypes.data + 8 * curve.JW * j) for j in range(m)]
    h = db.handle

    def a():
        assert many(h, 0, vp(sc), n, n, m, 0, vp(out), None) == 0

    def rows(lo, hi):
        for j in range(lo, hi):
            assert one(h, 0, sp[j], n, 0, op[j]) == 0

    def b():
        rows(0, m)

    def c():
        cuts = [m * k // 6 for k in range(7)]
        list(pool.map(lambda k: rows(cuts[k], cuts[k + 1]), range(6)))

    res = {"curve": curve.tag, "n": n, "m": m, "many": timed(a), "singles": timed(b), "singles6": timed(c)}
    assert (out == out1).all()                              # the three ways computed the same words
    k = m if m * n <= ORACLE_TERMS else max(8, ORACLE_TERMS // n)
    t0 = time.perf_counter()
    for j in range(k):
        G.msm(bases[:n], sc[j], threads=16)
    res["cpu16_ms"] = (time.perf_counter() - t0) * 1e3 * m / k
    res["cpu16_extrapolated_from_rows"] = k if k < m else None
    res["wins"] = res["many"]["max_ms"] < res["singles6"]["min_ms"]
    return res


def main():
    one = os.environ.get("ONE")
    results = []
    with ThreadPoolExecutor(6) as pool:
        for curve, G in ((ca.G1, O.G1), (ca.G2, O.G2)):
            if one and one.split(":")[0] != curve.tag:
                continue
            bases, _, _ = U.seq_bases(G, max(NS + [int(one.split(":")[2])] if one else NS), 4242, threads=16)
            db = ca.DeviceBases(curve, bases)
            if one:
                m, n = int(one.split(":")[1]), int(one.split(":")[2])
                sc = O.rand_scalars(5, m * n).reshape(m, n, 4)
                db.msm_many(sc); db.msm_many(sc)
                print("one %s many-call m=%d n=%d done" % (curve.tag, m, n))
                return
            for n in NS:
                for m in MS:
                    r = shape(curve, G, db, bases, n, m, pool)
                    results.append(r)
                    print("%s n=%5d m=%5d | many %8.3f [%8.3f %8.3f] | singles %9.3f [%9.3f %9.3f] | six in flight %9.3f [%9.3f %9.3f] | cpu16 %10.1f%s | %s" % (
                        r["curve"], n, m, r["many"]["median_ms"], r["many"]["min_ms"], r["many"]["max_ms"], r["singles"]["median_ms"], r["singles"]["min_ms"], r["singles"]["max_ms"],
                        r["singles6"]["median_ms"], r["singles6"]["min_ms"], r["singles6"]["max_ms"], r["cpu16_ms"], "*" if r["cpu16_extrapolated_from_rows"] else " ",
                        "many wins" if r["wins"] else "MANY DOES NOT WIN"), flush=True)
            db.free()
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "msm_many_timing.json"))
    with open(out, "w") as f:
        json.dump({"unit": "ms", "reps": REPS, "note": "median / min / max of host-clock-synchronised calls; singles6 = the m single calls over six threads; cpu16 = the oracle's m MSMs on 16 threads, one pass", "shapes": results}, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
