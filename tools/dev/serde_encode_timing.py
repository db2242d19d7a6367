"""Wall times of point encoding out of a resident plain handle (dgpu_bases_serialize_g*), next to a device-to-host copy of the same number of bytes
(torch, into pageable memory like the call's own output) and to the host encoder over the same words (dgpu_g*_serialize), plus dgpu_g*_serialize_device
and dgpu_bases_read_g*.  Host clock around calls that end in a device synchronise; one warm-up call each, the best of --reps.  Prints one JSON line.
Usage: python tools/dev/serde_encode_timing.py [--g1-log 20] [--g2-log 20] [--reps 5] [--host-reps 1]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch  # noqa: E402  (its HIP runtime first, as in the tests)
import crypto_amd as ca  # noqa: E402
from crypto_amd._native import lib  # noqa: E402
import oracle_c as O  # noqa: E402


def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return round(min(ts) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1-log", type=int, default=20)
    ap.add_argument("--g2-log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    ca.init(0)
    L = lib()
    out = {"reps": a.reps}
    for curve, G, lg in ((ca.G1, O.G1, a.g1_log), (ca.G2, O.G2, a.g2_log)):
        n, t = 1 << lg, curve.tag
        pts = np.ascontiguousarray(G.gen_seq(O.rand_scalars(lg, 1)[0], O.rand_scalars(lg + 1, 1)[0], n, threads=16))
        db = ca.DeviceBases(curve, pts)
        sz = (48 if t == "g1" else 96)
        buf = np.zeros(n * sz, np.uint8)
        dev = torch.empty(n * sz, dtype=torch.uint8, device="cuda")
        host = torch.empty(n * sz, dtype=torch.uint8)

        def d2h():
            host.copy_(dev)
            torch.cuda.synchronize()
        ser, hser, sdev = getattr(L, "dgpu_bases_serialize_%s" % t), getattr(L, "dgpu_%s_serialize" % t), getattr(L, "dgpu_%s_serialize_device" % t)
        key = "%s_2p%d_compressed" % (t, lg)
        out[key + "_bases_serialize_ms"] = best(lambda: ser(db.handle, 0, n, 1, p_(buf)), a.reps)
        got = buf.tobytes()
        out[key + "_d2h_same_bytes_ms"] = best(d2h, a.reps)
        out[key + "_host_serialize_ms"] = best(lambda: hser(p_(pts), None, n, 1, p_(buf)), a.host_reps)
        assert buf.tobytes() == got
        out[key + "_serialize_device_ms"] = best(lambda: sdev(p_(pts), None, n, 1, p_(buf)), a.reps)
        assert buf.tobytes() == got
        xy, inf = np.zeros((n, curve.AW), np.uint64), np.zeros(n, np.uint8)
        out["%s_2p%d_bases_read_ms" % (t, lg)] = best(lambda: getattr(L, "dgpu_bases_read_%s" % t)(db.handle, 0, n, p_(xy), p_(inf)), a.reps)
        assert (xy == pts).all()
        out[key + "_vs_d2h"] = round(out[key + "_bases_serialize_ms"] / out[key + "_d2h_same_bytes_ms"], 2)
        out[key + "_host_over_device"] = round(out[key + "_host_serialize_ms"] / out[key + "_bases_serialize_ms"], 1)
        db.free()
        del dev
    print(json.dumps(out))


if __name__ == "__main__":
    main()
