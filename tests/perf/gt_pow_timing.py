"""dgpu_fp12_pow_batch, dgpu_fp12_multi_pow_device and dgpu_gt_in_subgroup_device against their host counterparts on the same box: a 16-thread loop
of dgpu_fp12_pow, dgpu_fp12_multi_pow, dgpu_gt_in_subgroup.  Interleaved (device, host, device, ...), median of 7, host clock round synchronous
calls.  Sizes 64 .. 65536; the knob's bases per group swept at 4096 and 65536 on the development twin.  Writes profiles/gt_pow_timing.json.

    python tests/perf/gt_pow_timing.py [--sizes 64,256,...] [--reps 7] [--out profiles/gt_pow_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import crypto_amd as ca                    # noqa: E402
import oracle_c as O                       # noqa: E402
from crypto_amd._native import lib         # noqa: E402

p_ = lambda a: a.ctypes.data_as(C.c_void_p)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def inputs(n):
    """n members of GT (powers of four pairings) and n exponents below r"""
    g1 = lambda k: O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(k, 4)))[0]
    g2 = lambda k: O.G2.to_affine(O.G2.mul(O.G2.generator(), O.int_to_limbs(k, 4)))[0]
    seeds = [np.asarray(O.final_exponentiation(O.multi_miller_loop(g1(3 + i).reshape(1, 12), g2(5 + i).reshape(1, 24))), np.uint64).reshape(72) for i in range(4)]
    rng = np.random.default_rng(n)
    e = np.zeros((n, 4), np.uint64)
    for i in range(n):
        v = int.from_bytes(rng.bytes(40), "little") % R
        e[i] = [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    a = np.ascontiguousarray(np.stack(seeds)[np.arange(n) % 4])
    # distinct bases: a_i = seed^(e_i) computed on the device itself (checked against the host on the first 8)
    out = np.zeros((n, 72), np.uint64)
    assert lib().dgpu_fp12_pow_batch(p_(a), p_(e), 4, n, p_(out)) == 0
    for i in range(min(n, 8)):
        w = np.zeros(72, np.uint64)
        assert lib().dgpu_fp12_pow(p_(a[i]), p_(e[i]), p_(w)) == 0 and (w == out[i]).all()
    return out, np.ascontiguousarray(np.roll(e, 1, axis=0))


def med(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,1024,4096,16384,65536")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-max", type=int, default=65536, help="largest n at which the host counterparts run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_pow_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    L = lib()
    res = {"reps": args.reps, "sizes": {}, "k_sweep": {}}
    pool = ThreadPoolExecutor(16)
    for n in [int(x) for x in args.sizes.split(",")]:
        a, e = inputs(n)
        out_d, out_h, one_d, one_h = np.zeros((n, 72), np.uint64), np.zeros((n, 72), np.uint64), np.zeros(72, np.uint64), np.zeros(72, np.uint64)
        ok_d, ok_h = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        def host_pow():
            def part(t):
                for i in range(t, n, 16):
                    L.dgpu_fp12_pow(p_(a[i]), p_(e[i]), p_(out_h[i]))
            list(pool.map(part, range(16)))
        calls = {"pow_batch": (lambda: L.dgpu_fp12_pow_batch(p_(a), p_(e), 4, n, p_(out_d)), host_pow),
                 "multi_pow": (lambda: L.dgpu_fp12_multi_pow_device(p_(a), p_(e), n, p_(one_d)), lambda: L.dgpu_fp12_multi_pow(p_(a), p_(e), n, p_(one_h))),
                 "in_subgroup": (lambda: L.dgpu_gt_in_subgroup_device(p_(a), n, p_(ok_d)), lambda: L.dgpu_gt_in_subgroup(p_(a), n, p_(ok_h)))}
        row = {}
        for name, (dev, host) in calls.items():
            dev()                                                     # warm: the slot's workspace grows once
            td, th = [], []
            for _ in range(args.reps):                                # interleaved
                t0 = time.perf_counter(); dev(); td.append((time.perf_counter() - t0) * 1e3)
                if n <= args.host_max:
                    t0 = time.perf_counter(); host(); th.append((time.perf_counter() - t0) * 1e3)
            row[name] = {"device_ms": float(np.median(td)), "host_ms": float(np.median(th)) if th else None}
        if n <= args.host_max:
            assert (out_d == out_h).all() and (one_d == one_h).all() and (ok_d == ok_h).all() and ok_d.all(), n
        res["sizes"][str(n)] = row
        print(n, json.dumps(row), flush=True)
        if n in (4096, 65536):
            with ca.twin() as T:
                sweep = {}
                for k in (1, 2, 4, 8):
                    assert T.dgpu_set_gt_pow(0, k, 0) == 0
                    w = np.zeros(72, np.uint64)
                    f = lambda: T.dgpu_fp12_multi_pow_device(p_(a), p_(e), n, p_(w))
                    f()
                    sweep[str(k)] = med(f, args.reps)[0]
                    assert n > args.host_max or (w == one_h).all()
                T.dgpu_set_gt_pow(0, 0, 0)
                res["k_sweep"][str(n)] = sweep
                print(n, "k sweep", json.dumps(sweep), flush=True)
    # the smallest measured n from which the device call is faster than its host counterpart and stays faster
    cross = {}
    for name in ("pow_batch", "multi_pow", "in_subgroup"):
        ns = [int(k) for k in res["sizes"] if res["sizes"][k][name]["host_ms"] is not None]
        c = None
        for n in sorted(ns, reverse=True):
            r = res["sizes"][str(n)][name]
            if r["device_ms"] < r["host_ms"]:
                c = n
            else:
                break
        cross[name] = c
    res["crossover_n"] = cross
    print("crossover", json.dumps(cross))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
