"""dgpu_final_exponentiation_batch against n host calls on 16 threads, and dgpu_legogroth16_verify_each against dgpu_legogroth16_verify_batch and n
single dgpu_legogroth16_verify calls: host clock round calls that end in a device synchronise, median of 7 runs (min, max beside it); one JSON line."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
import ctypes as C
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import torch  # noqa: F401  (before the library: see tests/conftest.py)
import crypto_amd as ca
from crypto_amd import pairing, legogroth16 as LG
from crypto_amd._native import lib
import test_gpu_verify_each as T

RUNS = 7


def timed(fn):
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ca.init(0)
    out = {"runs": RUNS, "final_exponentiation_batch": {}, "host_pool_16": {}, "verify_each": {}, "verify_batch": {}, "single_calls": {}}
    rng = np.random.default_rng(1)
    pool = ThreadPoolExecutor(16)
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)

    def host(fs):
        def one(f):
            o = np.zeros(72, np.uint64); lib().dgpu_final_exponentiation(p_(f), p_(o))
        list(pool.map(one, list(fs)))
    for n in (64, 256, 1024, 4096, 65536):
        fs = T.rand_f12(rng, n)
        pairing.final_exponentiation_batch(fs)
        out["final_exponentiation_batch"][n] = timed(lambda: pairing.final_exponentiation_batch(fs))
        out["host_pool_16"][n] = timed(lambda: host(fs))
    st = T.statement(1)
    for n in (64, 1024, 4096, 20000):
        cols, pubs = T.columns(st, n)
        pk = (cols["A"], cols["B"], cols["C"], cols["D"], pubs)
        LG.verify_proofs_each_abi(st["pvk"], None, None, packed=pk)
        out["verify_each"][n] = timed(lambda: LG.verify_proofs_each_abi(st["pvk"], None, None, packed=pk))
        out["verify_batch"][n] = timed(lambda: LG.verify_proofs_batch_abi(st["pvk"], None, None, 12345, packed=pk))
        if n <= 1024:
            proofs = [{k.lower(): cols[k][t] for k in "ABCD"} for t in range(n)]
            t0 = time.perf_counter()
            for t in range(n):
                LG.verify_proof_abi(st["pvk"], proofs[t], pubs[t])
            out["single_calls"][n] = {"total_ms": round((time.perf_counter() - t0) * 1e3, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
