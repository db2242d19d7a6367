"""The dgpu_saver_* calls on one device, each beside the same work done the only way the library allowed before them — the caller's chain of public calls from
the same build, with a PCIe round trip and host work between each:
  decrypt chain      dgpu_g1_scale_batch (-rho c_0_i) -> dgpu_multi_pairing_segments over (c_ij, V_2_j), (-rho c_0_i, V_1_j), one segment per chunk (at most 4096
                     segments a call) -> host: a dictionary from the first 16 bytes of every table entry (read back once, outside the timed region) to m,
                     confirmed by comparing the whole entry
  commitment chain   dgpu_multi_pairing_segments with one segment of K + 2 pairs per row against the affine [Z_0 .. Z_K, H]
dgpu_saver_verify_decryption_each and dgpu_saver_verify_commitments_batch have no chain of their own: they stand beside decrypt_many and verify_commitment_each.
A chain must give its call's bytes (asserted; one ciphertext that does not decrypt and one bad commitment among the rows).  The oracle's two-pair pairings on 16
host threads are timed ONCE, at the smallest n, and reported per ciphertext (the reference pays them per chunk on CPU threads).  The points are multiples of the
generators made by the library's own window tables; the first rows are compared with the oracle.  Host clock round synchronous calls; the sides of a comparison
ALTERNATE inside one loop after a warm call of each, and the median of --reps is kept.  Key creation (prepare, bases, table, index) is timed per shape, median of
three.  Stage times come from a second pass on the development twin; saver.lines is the per-column line launches.  No pass / fail threshold: the numbers are
written down.  Writes profiles/saver_timing.json.

    python tests/perf/saver_timing.py [--shapes 8x32,16x16] [--rows 64,1024,4096] [--reps 7] [--out profiles/saver_timing.json]
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
import oracle_c as O                       # noqa: E402
import saver_model as M                    # noqa: E402
from crypto_amd import saver as S          # noqa: E402
from crypto_amd import G1 as CG1, G2 as CG2   # noqa: E402
from crypto_amd.fixed_base import WindowTable  # noqa: E402
from crypto_amd._native import lib         # noqa: E402

R = M.R
p_ = lambda a: a.ctypes.data_as(C.c_void_p)
PREFIXES = ("saver.", "bbs.", "msm.")


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def alternate(fns, reps):
    """median milliseconds of each function, the functions taking turns inside one loop after a warm call of each"""
    for f in fns:
        f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t0 = time.perf_counter(); f(); ts[k].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts]


def segments(pa, qa, per):
    """the pairing value of every segment of `per` pairs: (n, 72)"""
    n = len(pa) // per
    out = np.zeros((n, 72), np.uint64)
    for lo in range(0, n, 4096):                                     # (the call takes at most 4096 segments)
        k = min(4096, n - lo)
        ends = (per * np.arange(1, k + 1)).astype(np.uint64)
        assert lib().dgpu_multi_pairing_segments(p_(pa[lo * per:]), p_(qa[lo * per:]), None, per * k, p_(ends), k, p_(out[lo:])) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x32,16x16")
    ap.add_argument("--rows", default="64,1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "saver_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    rng = np.random.default_rng(271828)
    one = np.asarray(O.fp12_one(), np.uint64)
    res = {"reps": args.reps, "shapes": {}}
    ns = [int(v) for v in args.rows.split(",")]

    for shape in args.shapes.split(","):
        b, K = (int(v) for v in shape.split("x"))
        d, h, rho = rand(rng, 3)
        key = M.Key(rand(rng, K), d, h, rho, rand(rng, K), rand(rng, K + 1), rand(rng, K), b)
        T1, T2 = WindowTable(CG1, O.G1.generator()), WindowTable(CG2, O.G2.generator())

        def g1_times(scalars):
            out, inf = T1.multiply_many(limbs([k % R for k in scalars]))
            out[inf.astype(bool)] = 0
            return out

        def g2_times(scalars):
            out, inf = T2.multiply_many(limbs([k % R for k in scalars]))
            out[inf.astype(bool)] = 0
            return out
        g = g1_times(key.a)
        g2 = g2_times([key.H(), key.V_0()] + key.V_1() + key.V_2() + key.Z())
        H, V0, V1, V2, Z = g2[0], g2[1], g2[2:2 + K], g2[2 + K:2 + 2 * K], g2[2 + 2 * K:]
        assert (V2[0] == O.G2.to_affine(O.G2.mul(O.G2.generator(), O.int_to_limbs(key.V_2()[0], 4)))[0]).all()
        T1.free(); T2.free()
        srow = {"table_bytes": 576 * K * key.E}
        make = lambda: S.DecryptionKey(g, H, V0, V1, V2, b)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter(); k0 = make(); ts.append((time.perf_counter() - t0) * 1e3); k0.free()
        srow["dk_create_ms"] = float(np.median(ts))
        dk, ck = make(), S.CommitmentKey(Z, H)
        # the caller's dictionary: the first 16 bytes of every entry -> m (confirmed against the whole entry)
        t0 = time.perf_counter()
        tabs = [dk.powers(j) for j in range(K)]
        dicts = []
        for j in range(K):
            dd = {}
            heads = np.ascontiguousarray(tabs[j][:, :2]).view(np.dtype((np.void, 16))).reshape(-1)
            for m, hd in enumerate(heads):
                dd.setdefault(hd.tobytes(), []).append(m + 1)
            dicts.append(dd)
        srow["chain_dictionary_build_ms"] = (time.perf_counter() - t0) * 1e3
        g2_commit = np.concatenate([Z, H.reshape(1, 24)])

        for n in ns:
            row = {}
            T1 = WindowTable(CG1, O.G1.generator())
            msgs = [[int(x) % (key.E + 1) for x in rng.integers(0, 1 << 16, K)] for _ in range(n)]
            msgs[n // 2][0] = key.E + 1                                  # one ciphertext that does not decrypt
            logs = [key.encrypt(m, r) for m, r in zip(msgs, rand(rng, n))]
            logs[n // 3][K + 1] = (logs[n // 3][K + 1] + 1) % R          # one bad commitment
            ct = g1_times([v for r_ in logs for v in r_]).reshape(n, K + 2, 12)
            T1.free()
            assert (ct[0][1] == O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(logs[0][1], 4)))[0]).all()
            neg_rho = limbs([(R - key.rho) % R])
            lookup_ms, pair_ms = [], []

            def decrypt_chain():
                c0 = np.ascontiguousarray(ct[:, 0])
                side, sinf = np.zeros((n, 12), np.uint64), np.zeros(n, np.uint8)
                assert lib().dgpu_g1_scale_batch(p_(c0), None, p_(neg_rho), 0, None, n, p_(side), p_(sinf)) == 0
                t0 = time.perf_counter()
                pa = np.empty((n, K, 2, 12), np.uint64); pa[:, :, 0] = ct[:, 1:K + 1]; pa[:, :, 1] = side[:, None]
                qa = np.empty((n, K, 2, 24), np.uint64); qa[:, :, 0] = V2[None]; qa[:, :, 1] = V1[None]
                vals = segments(pa.reshape(-1, 12), qa.reshape(-1, 24), 2).reshape(n, K, 72)
                pair_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                chunks, status = np.zeros((n, K), np.uint16), np.zeros(n, np.uint8)
                is_one = (vals == one).all(axis=2)
                heads = np.ascontiguousarray(vals[:, :, :2]).view(np.dtype((np.void, 16))).reshape(n, K)
                for i in range(n):
                    for j in range(K):
                        if is_one[i, j]:
                            continue
                        hit = [m for m in dicts[j].get(heads[i, j].tobytes(), ()) if (tabs[j][m - 1] == vals[i, j]).all()]
                        if hit:
                            chunks[i, j] = hit[0]
                        else:
                            status[i] = 1
                chunks[status != 0] = 0
                lookup_ms.append((time.perf_counter() - t0) * 1e3)
                return chunks, status
            dec_new = lambda: S.decrypt_chunks_many(dk, ct, key.rho)
            chunks, nu, status = dec_new()
            cc, cs = decrypt_chain()
            want_status = [1 if i == n // 2 else 0 for i in range(n)]
            assert status.tolist() == want_status and (cc == chunks).all() and (cs == status).all()
            assert chunks[0].tolist() == msgs[0]
            ver_new = lambda: S.verify_decryption_each(dk, ct, chunks, nu)
            assert ver_new().tolist() == [1 - s for s in want_status]
            lookup_ms.clear(); pair_ms.clear()
            row["decrypt_many_ms"], row["verify_decryption_each_ms"], row["decrypt_chain_ms"] = alternate([dec_new, ver_new, decrypt_chain], args.reps)
            row["decrypt_chain_pairings_ms"], row["decrypt_chain_host_lookup_ms"] = float(np.median(pair_ms)), float(np.median(lookup_ms))

            neg_psi = ct[:, K + 1].copy()
            neg = O.g1_scale_batch(neg_psi, limbs([R - 1]), threads=16)[0]          # -psi, once, outside the timed region

            def commit_chain():
                pa = ct.copy(); pa[:, K + 1] = neg
                qa = np.broadcast_to(g2_commit[None], (n, K + 2, 24))
                vals = segments(pa.reshape(-1, 12), np.ascontiguousarray(qa).reshape(-1, 24), K + 2)
                return (vals == one).all(axis=1).astype(np.uint8)
            each_new = lambda: S.verify_commitment_each(ck, ct)
            good = np.array([i != n // 3 for i in range(n)])
            w = [pow(7, i, R) for i in range(n)]
            wl = limbs(w)
            batch_new = lambda: S.verify_commitments_batch(ck, ct[good], wl[good])      # the batch that is timed is the one that verifies
            want = good.astype(np.uint8)
            assert (each_new() == want).all() and (commit_chain() == want).all() and batch_new() and not S.verify_commitments_batch(ck, ct, wl)
            row["verify_commitment_each_ms"], row["verify_commitments_batch_ms"], row["commitment_chain_ms"] = alternate([each_new, batch_new, commit_chain], args.reps)

            if n == ns[0]:
                # the reference's cost: one two-pair pairing per chunk and one (K + 2)-pair product per commitment, on 16 host threads, ONCE
                m = min(n, 64)
                t0 = time.perf_counter()
                side = O.g1_scale_batch(np.ascontiguousarray(ct[:m, 0]), neg_rho, threads=16)[0]
                for i in range(m):
                    for j in range(K):
                        v = O.final_exponentiation(O.multi_miller_loop(np.stack([ct[i, 1 + j], side[i]]), np.stack([V2[j], V1[j]]), threads=2))
                        if i == 0 and j == 0:
                            assert (np.asarray(v, np.uint64) == tabs[0][msgs[0][0] - 1]).all() if msgs[0][0] else (np.asarray(v, np.uint64) == one).all()
                srow["oracle_decrypt_pairings_ms_per_ciphertext"] = (time.perf_counter() - t0) * 1e3 / m
                t0 = time.perf_counter()
                for i in range(m):
                    pa = ct[i].copy(); pa[K + 1] = neg[i]
                    O.final_exponentiation(O.multi_miller_loop(pa, g2_commit, threads=16))
                srow["oracle_commitment_ms_per_ciphertext"] = (time.perf_counter() - t0) * 1e3 / m
                srow["oracle_rows"] = m

            with ca.twin(saver=True):                                   # the stage timers live on the SAVER library's development build: a key of its own
                with make() as dkt:
                    ckt = S.CommitmentKey(Z, H)
                    calls = {"decrypt_many": lambda: S.decrypt_chunks_many(dkt, ct, key.rho), "verify_decryption_each": lambda: S.verify_decryption_each(dkt, ct, chunks, nu),
                             "verify_commitment_each": lambda: S.verify_commitment_each(ckt, ct), "verify_commitments_batch": lambda: S.verify_commitments_batch(ckt, ct[good], wl[good])}
                    assert (calls["decrypt_many"]()[0] == chunks).all()
                    for name, fn in calls.items():
                        fn()
                        ca.prof.enable(True); ca.prof.reset()
                        for _ in range(3):
                            fn()
                        st = ca.prof.read()
                        ca.prof.enable(False)
                        row[name + "_stages_ms"] = {k: v[0] / 3 for k, v in st.items() if k.startswith(PREFIXES)}
                    if n == ns[0]:
                        ca.prof.enable(True); ca.prof.reset()
                        make().free()
                        st = ca.prof.read()
                        ca.prof.enable(False)
                        srow["dk_create_stages_ms"] = {k: v[0] for k, v in st.items() if k.startswith(PREFIXES)}
            srow["n=%d" % n] = row
            print(shape, n, json.dumps(row), flush=True)
        dk.free()
        del tabs, dicts
        res["shapes"]["b=%d,K=%d" % (b, K)] = srow
        print(shape, json.dumps({k: v for k, v in srow.items() if not k.startswith("n=")}), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
