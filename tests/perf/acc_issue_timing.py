"""dgpu_accumulator_d_for_batch[_resident], dgpu_accumulator_non_membership_witnesses_g1 and dgpu_accumulator_membership_witnesses_g1 on one device: the
whole call and its stages (StageTimer marks on the development twin), each against today's recipe on the same box in the same run.
  d        m in {64, 2^10, 2^14} non-members x n in {2^14, 2^20} members, the members from the host and resident.  The yardstick is the detour through
           dgpu_accumulator_update_witnesses_public_g1 with additions = members, no removals and no omega, whose d_factors are d: its whole time (what a
           caller pays today) and its acc.pub_factors stage (kernel against kernel: acc.d_eval).
  unroll   the two forms of k_acc_d (one and four non-members per lane) against each other, forced on the twin, at m in {2^10, 2^14} x n in
           {2^14, 2^16, 2^18, 2^20}: the same words, and the times the automatic switch is set from.
  points   m in {64, 2^10, 2^14}: the yardstick is the host's inversions and scalars natively on 16 threads (tests/native/acc_issue_host.cpp, the library's
           own host field), then dgpu_window_table_g1 + dgpu_window_table_mul_g1.
At every shape the recipe must give the call's words.  Host clock round synchronous calls, median of --reps after one warm call.  No pass / fail threshold
and no ratio fixed in advance: both numbers are written down.  Writes profiles/acc_issue_timing.json.

    python tests/perf/acc_issue_timing.py [--non-members 64,1024,16384] [--members 16384,1048576] [--unroll-non-members 1024,16384] [--unroll-members 16384,65536,262144,1048576] [--reps 5] [--out profiles/acc_issue_timing.json]
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
from crypto_amd.fixed_base import WindowTable  # noqa: E402

p_ = lambda a: a.ctypes.data_as(C.c_void_p)
PREFIXES = ("acc.", "fixed.")


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


def stages(fn, reps, knob=None):
    """per-stage milliseconds per call and the whole call's median, on the twin (knob: a function of the twin, called before and undone after)"""
    with ca.twin() as T:
        if knob:
            knob(T, True)
        try:
            whole = med(fn, reps)
            ca.prof.enable(True); ca.prof.reset()
            for _ in range(reps):
                fn()
            rows = ca.prof.read()
            ca.prof.enable(False)
        finally:
            if knob:
                knob(T, False)
    return whole, {k: v[0] / reps for k, v in rows.items() if k.startswith(PREFIXES)}


def host_lib():
    src = os.path.join(ROOT, "tests", "native", "acc_issue_host.cpp")
    so = os.path.join(ROOT, "tests", "native", "libacc_issue_host.so")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-mbmi2", "-madx", "-pthread", "-shared", "-fPIC", "-o", so, src])
    H = C.CDLL(so)
    H.acc_issue_scalars_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    H.acc_issue_scalars_host.restype = C.c_int
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--non-members", default="64,1024,16384")
    ap.add_argument("--members", default="16384,1048576")
    ap.add_argument("--unroll-non-members", default="1024,16384")
    ap.add_argument("--unroll-members", default="16384,65536,262144,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acc_issue_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    L = lib()
    ms = [int(x) for x in args.non_members.split(",")]
    res = {"reps": args.reps, "d": {}, "unroll": {}, "points": {}}
    for n in [int(x) for x in args.members.split(",")]:
        members = scalars(7 + n, n)
        for m in ms:
            ys = scalars(1000 * m + n, m)
            wit = np.zeros((m, 12), np.uint64)
            none = np.zeros((0, 12), np.uint64)
            host = lambda: ACC.d_for_batch(members, ys)
            detour = lambda: ACC.update_witnesses_public(members, [], none, ys, wit)
            d, nz = host()
            f, _, ok = detour()
            assert nz.all() and ok.all() and (f == d).all()                 # the recipe and the call: the same words
            res_h = ca.DeviceScalars(members)
            resident = lambda: ACC.d_for_batch(res_h, ys)
            assert (resident()[0] == d).all()
            row = {"host_call_ms": med(host, args.reps), "resident_call_ms": med(resident, args.reps), "detour_call_ms": med(detour, args.reps),
                   "members_uploaded_by_the_host_form_bytes": int(n * 32)}
            res_h.free()
            _, row["host_stages_ms"] = stages(host, args.reps)
            _, row["detour_stages_ms"] = stages(detour, args.reps)
            res["d"]["m=%d,n=%d" % (m, n)] = row
            print("d", m, n, json.dumps(row), flush=True)
    # one against four non-members per lane, forced on the twin: where the automatic choice (acc_launch.hip.h acc_d_unroll) comes from
    for m in [int(x) for x in args.unroll_non_members.split(",")]:
        for n in [int(x) for x in args.unroll_members.split(",")]:
            members, ys = scalars(7 + n, n), scalars(1000 * m + n, m)
            host = lambda: ACC.d_for_batch(members, ys)
            row, words = {}, []
            for u in (1, 4):
                knob = lambda T, on, u=u: T.dgpu_dev_set_acc_d_unroll(u if on else 0)
                with ca.twin() as T:
                    T.dgpu_dev_set_acc_d_unroll(u); words.append(host()[0]); row["chunks_%d" % u] = T.dgpu_dev_get_acc_split(); T.dgpu_dev_set_acc_d_unroll(0)
                whole, st = stages(host, args.reps, knob)
                row["unroll_%d" % u] = {"host_call_ms_on_the_twin": whole, "acc.d_eval": st.get("acc.d_eval")}
            assert (words[0] == words[1]).all()
            res["unroll"]["m=%d,n=%d" % (m, n)] = row
            print("unroll", m, n, json.dumps(row), flush=True)
    H = host_lib()
    k0, dd = O.rand_scalars(5, 1)[0], O.rand_scalars(6, 1)[0]
    base = np.ascontiguousarray(O.G1.gen_seq(k0, dd, 1, threads=1))[0]
    for m in ms:
        sc = scalars(31 * m, 2 * m + 2)
        d, ys, f_v, alpha = sc[:m], sc[m:2 * m], sc[2 * m], sc[2 * m + 1]
        for with_d, name in ((1, "non_membership"), (0, "membership")):
            call = (lambda: ACC.non_membership_witnesses(d, ys, f_v, alpha, base)[0]) if with_d else (lambda: ACC.membership_witnesses(ys, alpha, base))
            s = np.zeros((m, 4), np.uint64)

            def host_part():
                assert H.acc_issue_scalars_host(p_(d), p_(ys), m, p_(f_v), p_(alpha), with_d, 16, p_(s)) == 0

            def recipe():
                host_part()
                t = WindowTable(ca.G1, base)
                try:
                    return t.multiply_many(s)
                finally:
                    t.free()
            got, want = call(), recipe()
            assert (got[0] == want[0]).all() and (np.asarray(got[1]) == np.asarray(want[1])).all()      # the same points either way
            row = {"whole_call_ms": med(call, args.reps), "recipe_ms": med(recipe, args.reps), "recipe_host_part_ms": med(host_part, args.reps)}
            _, row["stages_ms"] = stages(call, args.reps)
            res["points"]["%s,m=%d" % (name, m)] = row
            print(name, m, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
