"""The four dgpu_ps_* calls on one device, each beside the same work done the only way the library allowed before them — the caller's chain of public calls
from the same build, with a PCIe round trip and host work between each:
  sign chain     host: u_i = r_i (x + sum_j y_j m_ij) (Python-integer work here, so it is ALSO reported on its own: sign_chain_host_scalars_ms)
                 -> dgpu_window_table_mul_g1 twice (the r_i, the u_i)
  verify chain   dgpu_msm_g2_handle_many over the rows (1, m ..) -> dgpu_multi_pairing_segments over (sigma_1, Q_i), (-sigma_2, g_tilde) (at most 4096 segments a call)
  proof chain    host: the rows S_i, R_i (a masked copy) and -c_i; dgpu_msm_g2_handle_many over both -> dgpu_g2_mul_add_batch twice (S_i - c_i k_i; R_i + k_i)
                 -> dgpu_multi_pairing_segments; host: the comparison with t_i and the order of the checks
dgpu_ps_verify_batch has no chain of its own: it stands beside dgpu_ps_verify_each.  At every shape a chain must give its call's bytes (asserted; a row that fails
and one made from a non-signature among them).  The points are multiples of the generators made by the library's own window tables (the oracle's G2 scalar
multiplication takes a millisecond a point); the first rows are compared with the oracle.  Host clock round synchronous calls; the sides of a comparison ALTERNATE
inside one loop after a warm call of each, and the median of --reps is kept.  Stage times come from a second pass on the development twin (StageTimer marks).
No pass / fail threshold: the numbers are written down.  Writes profiles/ps_timing.json.

    python tests/perf/ps_timing.py [--rows 64,1024,16384] [--messages 30] [--revealed 5] [--reps 7] [--out profiles/ps_timing.json]
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
import ps_model as M                       # noqa: E402
from crypto_amd import ps as PS            # noqa: E402
from crypto_amd import G1 as CG1, G2 as CG2   # noqa: E402
from crypto_amd.fixed_base import WindowTable  # noqa: E402
from crypto_amd._native import lib         # noqa: E402

R = M.R
P_LIMBS = [0xB9FEFFFFFFFFAAAB, 0x1EABFFFEB153FFFF, 0x6730D2A0F6B0F624, 0x64774B84F38512BF, 0x4B1BA7B6434BACD7, 0x1A0111EA397FE69A]
p_ = lambda a: a.ctypes.data_as(C.c_void_p)
PREFIXES = ("ps.", "bbs.", "msm.", "fixed.")


def limbs(vals):
    return np.array([[(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def neg_fq(y):
    """p - y on (n, 6) uint64 limbs, limb by limb with a borrow (no row is the identity)"""
    out, borrow = np.empty_like(y), np.zeros(len(y), np.uint64)
    for k in range(6):
        pk = np.uint64(P_LIMBS[k])
        t = pk - y[:, k]
        b1 = y[:, k] > pk
        out[:, k] = t - borrow
        borrow = (b1 | (t < borrow)).astype(np.uint64)
    return out


def alternate(fns, reps):
    """median milliseconds of each function, the functions taking turns inside one loop after a warm call of each"""
    for f in fns:
        f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t0 = time.perf_counter(); f(); ts[k].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="64,1024,16384")
    ap.add_argument("--messages", type=int, default=30)
    ap.add_argument("--revealed", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ps_timing.json"))
    args = ap.parse_args()
    ca.init(0)
    Lm = args.messages
    rng = np.random.default_rng(314159)
    x, gamma, gamma_t = rand(rng, 3)
    key = M.Key(x, rand(rng, Lm), gamma, gamma_t)
    one = O.fp12_one()
    revealed = sorted({(j * Lm) // args.revealed for j in range(args.revealed)})
    res = {"reps": args.reps, "messages": Lm, "revealed": len(revealed), "shapes": {}}

    def tables():
        return WindowTable(CG1, O.G1.generator()), WindowTable(CG2, O.G2.generator())

    def g1_times(T1, scalars):
        out, inf = T1.multiply_many(limbs([k % R for k in scalars]))
        out[inf.astype(bool)] = 0
        return out

    def g2_times(T2, scalars):
        out, inf = T2.multiply_many(limbs([k % R for k in scalars]))
        out[inf.astype(bool)] = 0
        return out

    def make(n, T1, T2):
        """n rows: messages, r, the signatures and the proofs from known discrete logs; row n // 2 fails its Schnorr check (and its signature does not verify),
        row 1 (n > 2) comes from a non-signature"""
        d = {"r": rand(rng, n), "msgs": [rand(rng, Lm) for _ in range(n)]}
        logs = [key.sign(r, m) for r, m in zip(d["r"], d["msgs"])]
        proofs = []
        for i in range(n):
            rp, rbar, c = rand(rng, 3)
            forge = 1 if n > 2 and i == 1 else 0
            proofs.append(M.prove(key, (logs[i][0], logs[i][1] + forge), d["msgs"][i], set(revealed), rp, rbar, rand(rng, Lm + 1), c))
        proofs[n // 2].t = (proofs[n // 2].t + 1) % R
        d["sigs"] = g1_times(T1, [v for s in logs for v in s]).reshape(n, 2, 12)
        d["proofs"] = proofs
        d["psig"] = g1_times(T1, [v for p in proofs for v in p.sig]).reshape(n, 2, 12)
        d["g2pts"] = g2_times(T2, [v for p in proofs for v in (p.k, p.t)]).reshape(n, 2, 24)
        # the library's tables made these points: the first rows against the oracle's scalar multiplication
        for i in range(min(n, 3)):
            assert (d["g2pts"][i][0] == O.G2.to_affine(O.G2.mul(O.G2.generator(), O.int_to_limbs(proofs[i].k, 4)))[0]).all()
            assert (d["sigs"][i][1] == O.G1.to_affine(O.G1.mul(O.G1.generator(), O.int_to_limbs(logs[i][1], 4)))[0]).all()
        return d

    def pairings(pa, qa, n):
        ends = (2 * np.arange(1, min(n, 4096) + 1)).astype(np.uint64)
        out = np.zeros((n, 72), np.uint64)
        for lo in range(0, n, 4096):                                 # (the call takes at most 4096 segments)
            k = min(4096, n - lo)
            assert lib().dgpu_multi_pairing_segments(p_(pa[lo:]), p_(qa[lo:]), None, 2 * k, p_(ends), k, p_(out[lo:])) == 0
        return (out == one).all(axis=1)

    def mul_add_g2(points, sc, stride, addend, add_inf):
        n = len(points)
        out, inf = np.zeros((n, 24), np.uint64), np.zeros(n, np.uint8)
        assert lib().dgpu_g2_mul_add_batch(p_(points), None, p_(sc), stride, p_(addend), p_(add_inf), n, p_(out), p_(inf)) == 0
        return out, inf

    def run(P, n, row, d, reps):
        rho = limbs(rand(rng, 1))[0]
        msgs = limbs([v for m in d["msgs"] for v in m]).reshape(n, Lm, 4)
        r, sk = limbs(d["r"]), limbs(key.sk(Lm))
        g_tilde = P.points[Lm + 1]

        # ---- signing
        host_ms = []

        def sign_chain():
            t0 = time.perf_counter()
            u = limbs([M.sign_scalars(key.x, key.ys, ri, m)[1] for ri, m in zip(d["r"], d["msgs"])])
            host_ms.append((time.perf_counter() - t0) * 1e3)
            out = np.empty((n, 2, 12), np.uint64)
            out[:, 0], _ = Tg.multiply_many(r)
            out[:, 1], _ = Tg.multiply_many(u)
            return out
        sign_new = lambda: PS.sign_many(P, sk, msgs, r)
        Tg = WindowTable(CG1, P.g)                                      # the caller's own table of g
        a, bad = sign_new()
        assert not bad.any() and (sign_chain() == a).all() and (a == d["sigs"]).all()
        host_ms.clear()
        row["sign_many_ms"], row["sign_chain_ms"] = alternate([sign_new, sign_chain], reps)
        row["sign_chain_host_scalars_ms"] = float(np.median(host_ms))
        Tg.free()

        # ---- verification
        a = a.copy()
        a[n // 2][1] = d["sigs"][(n // 2 + 1) % n][1] if n > 1 else O.G1.generator()      # one signature that does not verify
        rows = np.zeros((n, Lm + 1, 4), np.uint64)
        rows[:, 0, 0] = 1; rows[:, 1:] = msgs
        neg2 = a[:, 1].copy(); neg2[:, 6:] = neg_fq(a[:, 1, 6:])

        def verify_chain():
            q = np.ascontiguousarray(P.bases.msm_many(rows)[:, :24])                 # normalised (X, Y, 1): the affine words
            pa = np.empty((n, 2, 12), np.uint64); pa[:, 0] = a[:, 0]; pa[:, 1] = neg2
            qa = np.empty((n, 2, 24), np.uint64); qa[:, 0] = q; qa[:, 1] = g_tilde
            return pairings(pa, qa, n).astype(np.uint8)
        each_new = lambda: PS.verify_each(P, a, msgs)
        batch_new = lambda: PS.verify_batch(P, d["sigs"], msgs, rho)                  # the batch that is timed is the one that verifies
        want = np.ones(n, np.uint8); want[n // 2] = 0
        assert (each_new() == want).all() and (verify_chain() == want).all() and batch_new() and not PS.verify_batch(P, a, msgs, rho)
        row["verify_each_ms"], row["verify_batch_ms"], row["verify_chain_ms"] = alternate([each_new, batch_new, verify_chain], reps)

        # ---- proofs
        proofs = d["proofs"]
        z, values = limbs([p.z_r for p in proofs]), limbs([v for p in proofs for v in p.values]).reshape(n, Lm, 4)
        mask, chal = np.array([p.mask for p in proofs], np.uint8), limbs([p.c for p in proofs])
        psig, g2pts = d["psig"], d["g2pts"]
        pneg2 = psig[:, 1].copy(); pneg2[:, 6:] = neg_fq(psig[:, 1, 6:])
        one_sc = limbs([1])
        pok_host_ms = []

        def pok_chain():
            t0 = time.perf_counter()
            both = np.zeros((2 * n, Lm + 2, 4), np.uint64)
            both[:n, 1:Lm + 1] = np.where(mask[:, :, None] == 0, values, 0)
            both[:n, Lm + 1] = z
            both[n:, 0, 0] = 1
            both[n:, 1:Lm + 1] = np.where(mask[:, :, None] != 0, values, 0)
            neg_c = limbs([(R - p.c) % R for p in proofs])
            pok_host_ms.append((time.perf_counter() - t0) * 1e3)
            sj, sinf = P.bases.msm_many(both, flags=True)
            aff = np.ascontiguousarray(sj[:, :24])
            k = np.ascontiguousarray(g2pts[:, 0])
            got, ginf = mul_add_g2(k, neg_c, 4, np.ascontiguousarray(aff[:n]), np.ascontiguousarray(sinf[:n]))
            q, _ = mul_add_g2(k, one_sc, 0, np.ascontiguousarray(aff[n:]), np.ascontiguousarray(sinf[n:]))
            pa = np.empty((n, 2, 12), np.uint64); pa[:, 0] = psig[:, 0]; pa[:, 1] = pneg2
            qa = np.empty((n, 2, 24), np.uint64); qa[:, 0] = q; qa[:, 1] = g_tilde
            pairing = pairings(pa, qa, n)
            schnorr = (ginf == 0) & (got == g2pts[:, 1]).all(axis=1)
            return np.where(~schnorr, 3, np.where(~pairing, 4, 0)).astype(np.uint8)          # (no signature element of these rows is the identity)
        pok_new = lambda: PS.pok_verify_each(P, psig, g2pts, z, values, mask, chal)
        want = np.array([p.status(key) for p in proofs], np.uint8)
        assert want[n // 2] == 3 and (n <= 2 or want[1] == 4) and int((want != 0).sum()) == (2 if n > 2 else 1)
        assert (pok_new() == want).all() and (pok_chain() == want).all()
        pok_host_ms.clear()
        row["pok_verify_each_ms"], row["pok_chain_ms"] = alternate([pok_new, pok_chain], reps)
        row["pok_chain_host_rows_ms"] = float(np.median(pok_host_ms))
        return {"sign_many": sign_new, "verify_each": each_new, "verify_batch": batch_new, "pok_verify_each": pok_new}

    def pk_points(T2):
        return g2_times(T2, key.pk_scalars(Lm))

    for n in [int(v) for v in args.rows.split(",")]:
        row = {}
        T1, T2 = tables()
        d = make(n, T1, T2)
        pk, g = pk_points(T2), g1_times(T1, [key.gamma])[0]
        with PS.PsParams(g, pk[Lm + 1], pk[0], pk[1:Lm + 1]) as P:
            run(P, n, row, d, args.reps)
        T1.free(); T2.free()
        with ca.twin():                                             # the stage timers live on the twin: parameters of its own
            with PS.PsParams(g, pk[Lm + 1], pk[0], pk[1:Lm + 1]) as P:
                calls = run(P, n, {}, d, 1)                     # (the same checks against the twin; its timings are not kept)
                for name, fn in calls.items():
                    ca.prof.enable(True); ca.prof.reset()
                    for _ in range(args.reps):
                        fn()
                    st = ca.prof.read()
                    ca.prof.enable(False)
                    row[name + "_stages_ms"] = {k: v[0] / args.reps for k, v in st.items() if k.startswith(PREFIXES)}
        res["shapes"]["n=%d" % n] = row
        print(n, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
