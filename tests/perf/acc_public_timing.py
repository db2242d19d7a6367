"""dgpu_accumulator_omega_g1 and dgpu_accumulator_update_witnesses_public_g1 on one device: the whole call and its stages (StageTimer marks on the
development twin).
  Omega           n_add = n_rem in {2^8, 2^11, 2^14}.  There is no yardstick in this repository (the reference's Omega::new is Rust on rayon threads and is
                  not built here): its time is reported alone.
  public update   m in {2^10, 2^14} holders x n_omega in {2^8, 2^11}, against today's recipe on the same box, whole: the host computes f_i, s_i = 1 / d_D(y_i) and
                  the m x n_omega scaled powers natively on 16 threads (tests/native/acc_rows_host.cpp, the library's own host field), the rows go through
                  dgpu_msm_g1_handle_many over a resident omega, then dgpu_g1_mul_add_batch gives f_i C_i + T_i.  The recipe's host part is also reported alone.
                  At every shape the recipe must give the call's points.
Host clock round synchronous calls, median of --reps after one warm call.  No pass / fail threshold and no ratio fixed in advance: both numbers are
written down.  Writes profiles/acc_public_timing.json.

    python tests/perf/acc_public_timing.py [--omega 256,2048,16384] [--holders 1024,16384] [--lengths 256,2048] [--reps 5] [--out profiles/acc_public_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
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
PREFIXES = ("acc.", "msm.many", "msm.small_subtable", "msm.prep_bases", "fixed.")


def med(fn, reps):
    fn()                                                          # warm: the slot's workspace grows once
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def scalars(seed, n):
    sc = O.rand_scalars(seed, n)
    sc[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)                     # below r
    return np.ascontiguousarray(sc)


def points(seed, n):
    k0, d = O.rand_scalars(seed, 1)[0], O.rand_scalars(seed + 1, 1)[0]
    return np.ascontiguousarray(O.G1.gen_seq(k0, d, n, threads=16))


def stages(fn, reps):
    """per-stage milliseconds per call, from the twin's event timers"""
    with ca.twin():
        fn()
        ca.prof.enable(True); ca.prof.reset()
        for _ in range(reps):
            fn()
        rows = ca.prof.read()
        ca.prof.enable(False)
    return {k: v[0] / reps for k, v in rows.items() if k.startswith(PREFIXES)}


def host_lib():
    src = os.path.join(ROOT, "tests", "native", "acc_rows_host.cpp")
    so = os.path.join(ROOT, "tests", "native", "libacc_rows_host.so")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-mbmi2", "-madx", "-pthread", "-shared", "-fPIC", "-o", so, src])
    H = C.CDLL(so)
    H.acc_rows_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    H.acc_rows_host.restype = None
    return H


def host_part(H, adds, rems, ys, n, f, rows):
    """the recipe's host share: f, s and the scaled powers, 16 native threads"""
    H.acc_rows_host(p_(adds), len(adds), p_(rems), len(rems), p_(ys), len(ys), n, 16, p_(f), p_(rows))


def recipe(L, handle, rows, n, f, Cw):
    """today's device route: T = rows x omega (one many-row call over the resident omega), then f C + T"""
    m = len(f)
    T, Tinf = np.zeros((m, 18), np.uint64), np.zeros(m, np.uint8)
    assert L.dgpu_msm_g1_handle_many(handle, 0, p_(rows), n, n, m, 0, p_(T), p_(Tinf)) == 0
    Ta = np.ascontiguousarray(T[:, :12])                           # the rows come back normalised: (X, Y, 1)
    out, oinf = np.zeros((m, 12), np.uint64), np.zeros(m, np.uint8)
    assert L.dgpu_g1_mul_add_batch(p_(Cw), None, p_(f), 4, p_(Ta), p_(Tinf), m, p_(out), p_(oinf)) == 0
    return out, oinf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--omega", default="256,2048,16384")
    ap.add_argument("--holders", default="1024,16384")
    ap.add_argument("--lengths", default="256,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acc_public_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    L = lib()
    res = {"reps": args.reps, "omega": {}, "public_update": {}}
    V = points(5, 1)[0]
    for n in [int(x) for x in args.omega.split(",")]:
        sc = scalars(100 + n, 2 * n + 1)
        fn = lambda: ACC.omega(sc[:n], sc[n:2 * n], sc[2 * n], V)
        pts, inf = fn()
        assert len(pts) == n and not inf.any()
        row = {"whole_call_ms": med(fn, args.reps), "stages_ms": stages(fn, args.reps)}
        res["omega"]["n_add=n_rem=%d" % n] = row
        print("omega", n, json.dumps(row), flush=True)
    H = host_lib()
    for m in [int(x) for x in args.holders.split(",")]:
        for n in [int(x) for x in args.lengths.split(",")]:
            sc = scalars(1000 * m + n, 2 * n + 1 + m)
            adds, rems, alpha, ys = sc[:n], sc[n:2 * n], sc[2 * n], sc[2 * n + 1:]
            Cw = points(11 + m, m)
            om = ACC.omega(adds, rems, alpha, V)
            fn = lambda: ACC.update_witnesses_public(adds, rems, om, ys, Cw)
            d, (w, winf), ok = fn()
            assert ok.all()
            f, rows = np.zeros((m, 4), np.uint64), np.zeros((m * n, 4), np.uint64)
            h = C.c_uint64(0)
            assert L.dgpu_bases_upload_g1(p_(om[0]), p_(om[1]), n, C.byref(h)) == 0

            def whole_recipe():
                host_part(H, adds, rems, ys, n, f, rows)
                return recipe(L, h.value, rows, n, f, Cw)
            out, oinf = whole_recipe()
            assert (f == d).all() and (out == w).all() and (oinf == winf).all()      # the same factors and points either way
            row = {"whole_call_ms": med(fn, args.reps), "recipe_ms": med(whole_recipe, args.reps),
                   "recipe_host_part_ms": med(lambda: host_part(H, adds, rems, ys, n, f, rows), args.reps),
                   "rows_uploaded_by_the_recipe_bytes": int(m * n * 32), "stages_ms": stages(fn, args.reps)}
            L.dgpu_bases_free(h.value)
            res["public_update"]["m=%d,n_omega=%d" % (m, n)] = row
            print("public", m, n, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
