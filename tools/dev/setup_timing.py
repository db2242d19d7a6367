"""Wall time of LegoGroth16 key generation: legogroth16.generate_parameters (host scalar half + device fixed-base products) against
generate_parameters_r1cs (dgpu_legogroth16_setup: everything on the device), and the device instance map alone, at D = 2^16, 2^18, 2^20 on the
`nconstraints` circuit (tests/bigcase.py).  Device calls: median of --reps runs after one warm-up; the instance map
also without its host copies; the stage timers of both calls (development twin, mean per call).  Writes the JSON to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import crypto_amd as ca  # noqa: E402
from crypto_amd import legogroth16 as LG, qap  # noqa: E402
import lego_setup as LS  # noqa: E402
import oracle_c as O  # noqa: E402
from bigcase import big_circuit  # noqa: E402


def med(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,18,20")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-max-log", type=int, default=18, help="time the Python generate_parameters up to this size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setup_timing.json"))
    a = ap.parse_args()
    ca.init(0)
    R = LS.R
    w = [(0x1234567 * (k + 3) ** 40) % R for k in range(6)]
    g1 = O.G1.to_affine(O.G1.generator())[0]
    g2 = O.G2.to_affine(O.G2.generator())[0]
    rows = []
    for lg in (int(x) for x in a.logs.split(",")):
        m = (1 << lg) - 3
        z, A, B, Cm, n_inst, nc = big_circuit(m, 7)
        dr = qap.DeviceR1cs(A, B, Cm, len(z), n_inst, nc)
        im_ms, im_all = med(lambda: dr.instance_map(w[5]), a.reps)

        def dev_in(circuit):
            pk, _ = LG.generate_parameters_r1cs(circuit, 2, *w, g1, g2)
            for q in (pk.a_query, pk.b_g1_query, pk.b_g2_query, pk.h_query, pk.l_query):
                q.free()
        dev_ms, dev_all = med(lambda: dev_in(dr), a.reps)
        row = {"log_d": lg, "m": m, "instance_map_ms": im_ms, "instance_map_runs_ms": im_all, "generate_parameters_r1cs_ms": dev_ms, "generate_parameters_r1cs_runs_ms": dev_all}
        if lg <= a.host_max_log:
            cs = LS.circuit(m, 7)
            t0 = time.perf_counter()
            pk, _ = LG.generate_parameters(cs["A"], cs["B"], cs["C"], n_inst, len(z) - n_inst, 2, *w, g1, g2)
            row["generate_parameters_python_ms"] = (time.perf_counter() - t0) * 1e3
            for q in (pk.a_query, pk.b_g1_query, pk.b_g2_query, pk.h_query, pk.l_query):
                q.free()
        # the instance map without its three host copies (outputs NULL): the kernels, the call's one allocation and its synchronisations
        tw = LG._sc(w[5])
        Dn = C.c_size_t(0)
        row["instance_map_no_host_outputs_ms"], _ = med(lambda: ca._native.lib().dgpu_qap_instance_map(dr.handle, tw.ctypes.data_as(C.c_void_p), 0, None, None, None, None, C.byref(Dn)), a.reps)
        dr.free()
        # the library's stage timers (HIP events on the call's stream; development twin): where the device time of both calls goes
        with ca.twin():
            dt = qap.DeviceR1cs(A, B, Cm, len(z), n_inst, nc)
            dt.instance_map(w[5]); dev_in(dt)
            ca.prof.enable(True)
            ca.prof.reset()
            for _ in range(a.reps):
                dt.instance_map(w[5])
            row["stages_instance_map_call_ms"] = {k: v[0] / a.reps for k, v in ca.prof.read().items() if v[1]}
            ca.prof.reset()
            for _ in range(a.reps):
                dev_in(dt)
            row["stages_setup_call_ms"] = {k: v[0] / a.reps for k, v in ca.prof.read().items() if v[1]}
            ca.prof.enable(False)
            dt.free()
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "LegoGroth16 key generation wall time (ms), nconstraints circuit, one MI355X", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
