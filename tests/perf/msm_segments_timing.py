"""Timing driver (GPU box): dgpu_msm_g*_segments against the only way the same segments are computed on the device without it, on one box in one process.
Per shape (G1 and G2), interleaved, median / min / max of REPS host-clock-synchronised repetitions of
  (a) segments  one dgpu_msm_*_segments call
  (b) singles   the loop of dgpu_msm_* calls over the same segments with the size threshold off
The shapes are the reference's: 34 x 64 (saver/src/encryption.rs:710-740), 256 x 16, 1024 x 16, 1024 x 256, 64 x 4096 and the ragged mix of
tests/test_gpu_msm_segments.py.  `faster` is (a).median < (b).median.
The second part runs on the development twin and times the per-segment fold both ways (host threads' host_fold / k_seg_fold on the device, forced by
dgpu_set_msm_segments) over a sweep of segment counts: the crossover is the first count from which the device fold's median stays below the host's —
msm_many.hip.h SEG_DEVICE_FOLD_MIN is set from it.  Writes profiles/msm_segments_timing.json (OUT=...) and prints a table.
ONE=g1:1024:16 runs a few segmented calls of that shape and exits (for a kernel trace)."""
import ctypes as C
import json
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import crypto_amd as ca
from crypto_amd._native import lib
import oracle_c as O
import util as U

REPS = int(os.environ.get("REPS", "9"))
RAGGED = [0, 1, 5, 64, 65, 511, 512, 513, 4096, 5, 0, 0, 1, 513, 64, 3, 0]
SHAPES = [("34x64", [64] * 34), ("256x16", [16] * 256), ("1024x16", [16] * 1024), ("1024x256", [256] * 1024), ("64x4096", [4096] * 64), ("ragged", RAGGED)]
FOLD_NSEG = [1, 2, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 256]
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
stats = lambda ts: {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def operands(G, lens, seed, pool):
    N = sum(lens)
    reps = -(-N // len(pool))
    bases = np.ascontiguousarray(np.tile(pool, (reps, 1))[:N])          # (distinct scalars on repeated points: the kernels do not care)
    return bases, O.rand_scalars(seed, N), np.cumsum(np.array(lens, np.uint64), dtype=np.uint64)


def shape(curve, G, name, lens, pool):
    bases, sc, se = operands(G, lens, 31 + len(lens), pool)
    N, nseg = len(sc), len(lens)
    seg = curve.fn("dgpu_msm_%s_segments"); one = curve.fn("dgpu_msm_%s")
    out = np.zeros((nseg, curve.JW), np.uint64); out1 = np.zeros((nseg, curve.JW), np.uint64)
    lo = np.concatenate([[0], se[:-1]]).astype(np.int64)
    args = [(C.c_void_p(bases.ctypes.data + 8 * curve.AW * int(lo[g])), C.c_void_p(sc.ctypes.data + 32 * int(lo[g])), int(lens[g]), C.c_void_p(out1.ctypes.data + 8 * curve.JW * g)) for g in range(nseg)]

    def a():
        assert seg(vp(bases), None, vp(sc), N, vp(se), nseg, 0, vp(out), None) == 0

    def b():
        for bp, sp, n, op in args:
            assert one(bp, None, sp, n, op) == 0

    a(); b()                                                            # warm: workspaces
    ta, tb = [], []
    for _ in range(REPS):                                               # interleaved: both see the same box at the same time
        t0 = time.perf_counter(); a(); ta.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); b(); tb.append((time.perf_counter() - t0) * 1e3)
    assert (out == out1).all()                                          # both ways computed the same words
    r = {"curve": curve.tag, "shape": name, "nseg": nseg, "terms": N, "segments": stats(ta), "singles": stats(tb)}
    r["ratio_singles_over_segments"] = r["singles"]["median_ms"] / r["segments"]["median_ms"]
    r["faster"] = r["segments"]["median_ms"] < r["singles"]["median_ms"]
    return r


def fold_sweep(T, curve, G, pool, terms):
    rows = []
    for nseg in FOLD_NSEG:
        lens = [terms] * nseg
        bases, sc, se = operands(G, lens, 77 + nseg, pool)
        seg = getattr(T, "dgpu_msm_%s_segments" % curve.tag)
        outs = {}
        ts = {1: [], 2: []}
        for fold in (1, 2):
            outs[fold] = np.zeros((nseg, curve.JW), np.uint64)
            assert T.dgpu_set_msm_segments(fold, 0) == 0
            assert seg(vp(bases), None, vp(sc), len(sc), vp(se), nseg, 0, vp(outs[fold]), None) == 0
        for _ in range(REPS):
            for fold in (1, 2):
                assert T.dgpu_set_msm_segments(fold, 0) == 0
                t0 = time.perf_counter()
                assert seg(vp(bases), None, vp(sc), len(sc), vp(se), nseg, 0, vp(outs[fold]), None) == 0
                ts[fold].append((time.perf_counter() - t0) * 1e3)
        assert (outs[1] == outs[2]).all()
        rows.append({"curve": curve.tag, "nseg": nseg, "terms_per_segment": terms, "host_fold": stats(ts[1]), "device_fold": stats(ts[2])})
        print("fold %s nseg=%4d x %3d | host %8.3f [%8.3f %8.3f] | device %8.3f [%8.3f %8.3f]" % (
            curve.tag, nseg, terms, rows[-1]["host_fold"]["median_ms"], rows[-1]["host_fold"]["min_ms"], rows[-1]["host_fold"]["max_ms"],
            rows[-1]["device_fold"]["median_ms"], rows[-1]["device_fold"]["min_ms"], rows[-1]["device_fold"]["max_ms"]), flush=True)
    T.dgpu_set_msm_segments(0, 0)
    return rows


def crossover(rows):
    """the first segment count from which the device fold's median stays below the host fold's for every larger count measured"""
    best = None
    for r in reversed(rows):
        if r["device_fold"]["median_ms"] < r["host_fold"]["median_ms"]:
            best = r["nseg"]
        else:
            break
    return best


def main():
    ca.init(0)
    lib().dgpu_set_min_gpu_n(0)
    one = os.environ.get("ONE")
    pools = {c.tag: U.seq_bases(G, 4096, 4343, threads=16)[0] for c, G in ((ca.G1, O.G1), (ca.G2, O.G2))}
    if one:
        tag, nseg, n = one.split(":")
        curve, G = (ca.G1, O.G1) if tag == "g1" else (ca.G2, O.G2)
        bases, sc, se = operands(G, [int(n)] * int(nseg), 5, pools[tag])
        for _ in range(3):
            ca.msm_segments(curve, bases, sc, se)
        print("one %s segmented call nseg=%s n=%s done" % (tag, nseg, n))
        return
    results = []
    for curve, G in ((ca.G1, O.G1), (ca.G2, O.G2)):
        for name, lens in SHAPES:
            r = shape(curve, G, name, lens, pools[curve.tag])
            results.append(r)
            print("%s %-9s | segments %9.3f [%9.3f %9.3f] | singles %9.3f [%9.3f %9.3f] | x%6.2f | %s" % (
                r["curve"], name, r["segments"]["median_ms"], r["segments"]["min_ms"], r["segments"]["max_ms"], r["singles"]["median_ms"], r["singles"]["min_ms"],
                r["singles"]["max_ms"], r["ratio_singles_over_segments"], "segments faster" if r["faster"] else "SEGMENTS NOT FASTER"), flush=True)
    folds, cross = [], {}
    with ca.twin() as T:
        T.dgpu_set_min_gpu_n(0)
        for curve, G in ((ca.G1, O.G1), (ca.G2, O.G2)):
            for terms in (16, 64):
                rows = fold_sweep(T, curve, G, pools[curve.tag], terms)
                folds += rows
                cross["%s_x%d" % (curve.tag, terms)] = crossover(rows)
    print("fold crossover (segments per chunk from which the device fold is the shorter):", cross)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "msm_segments_timing.json"))
    with open(out, "w") as f:
        json.dump({"unit": "ms", "reps": REPS, "note": "median / min / max of host-clock-synchronised calls, (a) and (b) interleaved; singles = the loop of dgpu_msm_g* calls over the same segments, threshold off; the fold sweep forces the fold through the development twin",
                   "shapes": results, "fold_sweep": folds, "fold_crossover_nseg": cross}, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
