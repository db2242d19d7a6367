"""dgpu_witness_map_r1cs_many against a loop of m dgpu_witness_map_r1cs calls in the same process (the single call is what the library offered before
the many-row call existed), on a resident circuit with D = 512 and about three non-zeros per row.  Interleaved (one call, loop, one call, ...), median
of 7, host clock round synchronous calls; every row of the one call is compared with the loop's.  m = 16, 256, 4096; the rows per block swept at 4096 on
the development twin.  Writes profiles/witness_map_many_timing.json.

    python tests/perf/witness_map_many_timing.py [--rows 16,256,4096] [--reps 7] [--out profiles/witness_map_many_timing.json]
    python tests/perf/witness_map_many_timing.py --trace-rows 256      # one many-row call and one single call, nothing else: the run to put under a kernel trace
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
import wm_many_circuits as W               # noqa: E402
from crypto_amd import qap                 # noqa: E402
from crypto_amd._native import lib         # noqa: E402

p_ = lambda a: a.ctypes.data_as(C.c_void_p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="16,256,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-rows", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_map_many_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    circ = W.random_circuit(1, 510, 2, 600, terms=3)        # D = 512; A and B three terms per row, C one
    assert circ.D == 512
    sizes = [args.trace_rows] if args.trace_rows else [int(x) for x in args.rows.split(",")]
    rng = np.random.default_rng(2)
    base = W.rows_for(circ, 16, 3, kinds=("sat", "rand"))
    z_all = np.ascontiguousarray(base[rng.integers(0, 16, max(sizes))])
    D, nv = circ.D, circ.num_vars

    def calls(L, dev, m):
        z = z_all[:m]
        out_many, out_loop = np.zeros((m, D, 4), np.uint64), np.zeros((m, D, 4), np.uint64)
        n = C.c_size_t(0)
        def many():
            assert L.dgpu_witness_map_r1cs_many(dev.handle, p_(z), nv, nv, m, 0, p_(out_many), None, C.byref(n)) == 0
        def loop():
            for j in range(m):
                assert L.dgpu_witness_map_r1cs(dev.handle, p_(z[j]), nv, 0, p_(out_loop[j]), None, None) == 0
        return many, loop, out_many, out_loop

    if args.trace_rows:
        dev = qap.DeviceR1cs(*circ.mats, nv, circ.num_inputs, circ.num_constraints)
        many, _, out_many, out_loop = calls(lib(), dev, args.trace_rows)
        many()
        assert lib().dgpu_witness_map_r1cs(dev.handle, p_(z_all[0]), nv, 0, p_(out_loop[0]), None, None) == 0
        assert (out_many[0] == out_loop[0]).all()
        return
    res = {"reps": args.reps, "D": D, "num_vars": nv, "nnz": [int(len(m[1])) for m in circ.mats], "rows": {}, "rows_per_block_sweep": {}}
    dev = qap.DeviceR1cs(*circ.mats, nv, circ.num_inputs, circ.num_constraints)
    for m in sizes:
        many, loop, out_many, out_loop = calls(lib(), dev, m)
        many(); loop()                                              # warm: the slots' workspaces grow once
        tm, tl = [], []
        for _ in range(args.reps):                                  # interleaved
            t0 = time.perf_counter(); many(); tm.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); loop(); tl.append((time.perf_counter() - t0) * 1e3)
        assert (out_many == out_loop).all(), m
        row = {"many_ms": float(np.median(tm)), "loop_ms": float(np.median(tl)), "many_all_ms": tm, "loop_all_ms": tl}
        row["loop_over_many"] = row["loop_ms"] / row["many_ms"]
        res["rows"][str(m)] = row
        print(m, json.dumps({k: row[k] for k in ("many_ms", "loop_ms", "loop_over_many")}), flush=True)
    dev.free()
    m = max(sizes)
    with ca.twin() as T:
        devt = qap.DeviceR1cs(*circ.mats, nv, circ.num_inputs, circ.num_constraints)
        many, _, _, _ = calls(T, devt, m)
        for rpb in (1, 2):
            assert T.dgpu_set_wm_many(0, rpb) == 0
            many()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter(); many(); ts.append((time.perf_counter() - t0) * 1e3)
            res["rows_per_block_sweep"][str(rpb)] = float(np.median(ts))
        T.dgpu_set_wm_many(0, 0)
        devt.free()
    print("rows per block at m = %d" % m, json.dumps(res["rows_per_block_sweep"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
