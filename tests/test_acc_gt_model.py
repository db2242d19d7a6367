"""CPU: the big-integer model of the accumulator proof calls with a GT commitment (tests/acc_gt_model.py) against itself and against the oracle's group arithmetic
on the reference's equations (vb_accumulator/src/proofs.rs:890-996, :697-724, :1516-1580).  Nothing of the library runs here: these are checks of the yardstick
the other tests measure with."""
import numpy as np
import pytest
import oracle_c as O
import acc_gt_model as GM
from acc_gt_model import MEM, NM
from bbs_model import R

G = O.G1
lim = lambda v: O.int_to_limbs(v % R, 4)
TAMPERS, prove, tamper = GM.TAMPERS, GM.prove_row, GM.tamper


def rand(rng, n):
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


def scenario(kind, n, seed):
    rng = np.random.default_rng(seed)
    key = GM.Key(*rand(rng, 7))
    rows = [dict(y=rand(rng, 1)[0], d=rand(rng, 1)[0] or 1, rnd=rand(rng, 12), c=rand(rng, 1)[0]) for _ in range(n)]
    if n > 2:
        rows[1]["y"], rows[2]["y"] = 0, R - 1
    if n > 5:
        rows[5]["rnd"] = [0] * 12                        # no randomisation, zero blindings: every commitment but E_C [, E_d, E_d_inv] is the identity, R_E = 1
    if n > 9:
        rows[8]["c"], rows[9]["c"] = 0, R - 1
    return key, rows, [prove(key, kind, r["y"], r["d"], r["rnd"], r["c"]) for r in rows]


@pytest.mark.parametrize("kind", [MEM, NM])
def test_valid_proofs_verify_and_every_single_tamper_breaks_its_check(kind):
    key, rows, proofs = scenario(kind, 12, 31 + kind)
    for k, p in enumerate(proofs):
        assert p.checks(key) == [True] * (GM.CHECKS[kind] + 1) and p.status(key) == 0, k
    assert proofs[5].re == 0 and proofs[5].pts[GM.R_SIGMA] == 0
    for k, (what, status) in enumerate(TAMPERS[kind].items()):
        r = rows[k % 12]
        bad = prove(key, kind, r["y"], r["d"], r["rnd"], r["c"], forged=True) if what == "forged" else tamper(proofs[k % 12], what)
        assert bad.status(key) == status, what
    # a wrong shared point handed to the verifier fails every row at its first check that reads it
    wrong = {MEM: {"x": 1, "yk": 2, "z": 5, "v": 5}, NM: {"pi": 1, "k": 1, "x": 3, "yk": 4, "z": 7, "v": 7}}[kind]
    for name, status in wrong.items():
        assert [p.status(key, **{name: getattr(key, name) + 1}) for p in proofs[:5]] == [status] * 5, name


@pytest.mark.parametrize("kind", [MEM, NM])
def test_two_tampers_give_the_lower_number(kind):
    key, rows, proofs = scenario(kind, 4, 77 + kind)
    pairs = [("R_rho", "R_E"), ("s_delta_rho", "R_sigma"), ("E_C", "R_delta_sigma")] + ([("R_B", "R_A"), ("s_w", "R_E")] if kind == NM else [])
    for a, b in pairs:
        assert tamper(tamper(proofs[0], a), b).status(key) == min(TAMPERS[kind][a], TAMPERS[kind][b]), (a, b)


@pytest.mark.parametrize("kind", [MEM, NM])
def test_the_closed_form_batch_agrees_with_all_statuses_zero(kind):
    """random rho: the batch verifies iff every proof does; the sums of two chunks add up to the whole (what the second pass relies on)"""
    key, rows, proofs = scenario(kind, 40, 5 + kind)
    rng = np.random.default_rng(9)
    for rho in [1, 2, R - 1] + rand(rng, 3):
        assert GM.batch_verdict(key, proofs, rho)
        assert GM.batch_verdict(key, proofs[:1], rho)
    rho = rand(rng, 1)[0]
    for what in TAMPERS[kind]:
        for i in (0, 17, 39):
            r = rows[i]
            bad = list(proofs)
            bad[i] = prove(key, kind, r["y"], r["d"], r["rnd"], r["c"], forged=True) if what == "forged" else tamper(proofs[i], what)
            assert bad[i].status(key) != 0 and not GM.batch_verdict(key, bad, rho), (what, i)
    for name in ("v", "x", "yk", "z") + (("pi", "k") if kind == NM else ()):
        assert not GM.batch_verdict(key, proofs, rho, **{name: getattr(key, name) + 1}), name
    s, w, wp, wq, tp = GM.batch(proofs, 3)
    s0, w0, wp0, wq0, tp0 = GM.batch(proofs[:25], 3)
    s1, w1, wp1, wq1, tp1 = GM.batch(proofs[25:], 3, i0=25)
    assert [(a + b) % R for a, b in zip(s0, s1)] == s and w0 + w1 == w and wp0 + wp1 == wp and wq0 + wq1 == wq and tp0 + tp1 == tp
    assert tp[39] == pow(3, 39, R) and [len(x) for x in w] == [GM.NPTS[kind]] * 40


@pytest.mark.parametrize("kind", [MEM, NM])
def test_a_cancelling_pair_passes_at_rho_one_and_fails_at_two(kind):
    """two rows whose errors cancel unweighted — in a commitment of the G1 equation, and in R_E — pass under rho = 1, as they would in the reference's checker
    with that scalar, and fail under rho = 2; each row alone has a non-zero status"""
    key, rows, proofs = scenario(kind, 20, 55 + kind)
    X = 0x123456789
    for field in ("R_delta_rho", "R_E"):
        bad = [p.copy() for p in proofs]
        for i, dx in ((3, X), (11, -X)):
            if field == "R_E":
                bad[i].re = (bad[i].re + dx) % R
            else:
                bad[i].pts[GM.R_DRHO] = (bad[i].pts[GM.R_DRHO] + dx) % R
        want = TAMPERS[kind][field]
        assert [p.status(key) for p in bad] == [want if i in (3, 11) else 0 for i in range(20)]
        assert GM.batch_verdict(key, bad, 1) and not GM.batch_verdict(key, bad, 2), field


# ---- over real points ----
def mul(k):
    if k % R == 0:
        return np.zeros(12, np.uint64)
    return G.to_affine(G.mul(G.generator(), lim(k)))[0]


def msm_point(bases, scalars):
    """(affine words, is the identity) of sum scalars_k bases_k"""
    live = [(b, s) for b, s in zip(bases, scalars) if b.any() and s % R]
    if not live:
        return np.zeros(12, np.uint64), True
    aff, inf = G.to_affine(G.msm(np.stack([b for b, _ in live]), np.stack([lim(s) for _, s in live])))
    return (np.zeros(12, np.uint64), True) if inf else (aff, False)


@pytest.mark.parametrize("kind", [MEM, NM])
def test_the_model_against_the_oracle_over_real_points(kind):
    """a handful of proofs: every segment of the reference's equations by the oracle's MSM over real points, e(p, P~) e(q, pk) by its Miller loop and final
    exponentiation, R_E = e(G, P~)^re by its fp12_pow; a forged witness and a moved R_E fail the pairing alone"""
    key, rows, proofs = scenario(kind, 7, 2024 + kind)
    g2 = O.G2.generator()
    pk = O.G2.to_affine(O.G2.mul(g2, lim(key.alpha)))[0]
    e_gen = O.final_exponentiation(O.multi_miller_loop(G.generator().reshape(1, 12), g2.reshape(1, 24)))
    gt_of = lambda log: np.asarray(O.fp12_pow(e_gen, log % R), np.uint64) if log % R else np.asarray(O.fp12_one(), np.uint64)
    shared = {n: mul(getattr(key, n)) for n in ("v", "pi", "x", "yk", "z", "k")}

    def real_checks(p):
        pts = [mul(v) for v in p.pts]
        logs = p.bases(key)
        lookup = {getattr(key, n): shared[n] for n in shared}
        lookup.update({v: q for v, q in zip(p.pts, pts)})
        bases, own = [lookup[v] for v in logs], p.own()
        sums, lo = [], 0
        for hi in GM.SEG_ENDS[kind]:
            sums.append(msm_point(bases[lo:hi], own[lo:hi]))
            lo = hi
        (pp, pinf), (qq, qinf) = sums[-2:]
        live = [(a, b) for (a, inf), b in (((pp, pinf), g2), ((qq, qinf), pk)) if not inf]
        gt = O.final_exponentiation(O.multi_miller_loop(np.stack([a for a, _ in live]), np.stack([b for _, b in live]))) if live else O.fp12_one()
        return [inf for _, inf in sums[:-2]] + [bool((np.asarray(gt, np.uint64) == gt_of(p.re)).all())]

    for k in (0, 3, 5):
        assert real_checks(proofs[k]) == proofs[k].checks(key) == [True] * (GM.CHECKS[kind] + 1), k
    r = rows[1]
    forged = prove(key, kind, r["y"], r["d"], r["rnd"], r["c"], forged=True)
    assert real_checks(forged) == forged.checks(key) == [True] * GM.CHECKS[kind] + [False]
    moved = tamper(proofs[2], "R_E")
    assert real_checks(moved) == moved.checks(key) == [True] * GM.CHECKS[kind] + [False]
    bad = tamper(proofs[6], "s_delta_sigma")
    got = real_checks(bad)
    assert got == bad.checks(key) and got.index(False) + 1 == TAMPERS[kind]["s_delta_sigma"]
