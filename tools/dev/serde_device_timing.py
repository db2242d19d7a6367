"""Wall times of point decoding on the host (dgpu_g*_deserialize) and on the device (dgpu_g*_deserialize_device), validated and Validate::No, and of the
serialized upload against dgpu_bases_upload_* of the same points.  Host clock around calls that end in a device synchronise; one warm-up call each.
Prints one JSON line.  Usage: python tools/dev/serde_device_timing.py [--g1-log 20] [--g2-log 18] [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import torch  # noqa: F401,E402  (its HIP runtime first, as in the tests)
import crypto_amd as ca  # noqa: E402
from crypto_amd import serde  # noqa: E402
from crypto_amd._native import lib  # noqa: E402
from crypto_amd.fixed_base import WindowTable  # noqa: E402
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
    ap.add_argument("--g2-log", type=int, default=18)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    ca.init(0)
    L = lib()
    out = {"reps": a.reps}
    for curve, G, lg in ((ca.G1, O.G1, a.g1_log), (ca.G2, O.G2, a.g2_log)):
        n = 1 << lg
        sc = [int(x) for x in np.random.default_rng(lg).integers(1, 1 << 62, n)]
        with WindowTable(curve, G.generator()) as t:
            pts, inf = t.multiply_many(sc)
        data = np.frombuffer(serde.serialize(curve, pts, inf, True), np.uint8)
        xy, finf, bad, h = np.zeros((n, curve.AW), np.uint64), np.zeros(n, np.uint8), C.c_size_t(0), C.c_uint64(0)
        t = curve.tag
        hfn, dfn = getattr(L, "dgpu_%s_deserialize" % t), getattr(L, "dgpu_%s_deserialize_device" % t)
        ufn, upl = getattr(L, "dgpu_bases_upload_%s_serialized" % t), getattr(L, "dgpu_bases_upload_%s" % t)
        for mode, tag in ((1, "validated"), (3, "no_validate")):
            out["%s_2p%d_host_%s_ms" % (t, lg, tag)] = best(lambda: hfn(p_(data), n, mode, p_(xy), p_(finf)), a.host_reps)
            out["%s_2p%d_device_%s_ms" % (t, lg, tag)] = best(lambda: dfn(p_(data), n, mode, p_(xy), p_(finf), C.byref(bad)), a.reps)
            assert bad.value == n and (xy == pts).all()

        def up_ser():
            assert ufn(p_(data), n, 1, None, None, C.byref(h), C.byref(bad)) == 0
            L.dgpu_bases_free(h.value)

        def up_words():
            assert upl(p_(pts), p_(inf), n, C.byref(h)) == 0
            L.dgpu_bases_free(h.value)
        out["%s_2p%d_upload_serialized_ms" % (t, lg)] = best(up_ser, a.reps)
        out["%s_2p%d_upload_words_ms" % (t, lg)] = best(up_words, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
