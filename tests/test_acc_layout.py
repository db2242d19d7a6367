"""CPU: util.acc_layout, the model of the accumulate stage's chunking that tests/test_gpu_heavy_buckets.py builds its cases with — hand-worked layouts
(every count below was worked out on paper from the rule "thread t owns terms [t ch, (t + 1) ch)", not read off the model), and the model's chunk slots
against a term-by-term walk written after k_accumulate (crypto_amd/csrc/msm_kernels.hip.h K5)."""
import random
import numpy as np
import util as U

C8 = 8                       # B = 128 buckets per window, W = 32 windows


def scalars_of(counts, c=C8, window=0, seed=1):
    """counts[m] terms with digit m + 1 in `window` and nothing elsewhere, shuffled"""
    out = [(m + 1) << (c * window) for m, k in enumerate(counts) for _ in range(k)]
    random.Random(seed).shuffle(out)
    return out


def view(L, b):
    k = L.buckets[b]
    return (k.terms, k.t0, k.t1, k.pieces, k.cls)


def test_chunk_borders_by_hand():
    """ch = 4 (heavy from 64 terms).  Terms 0 .. 217 in bucket order:
    b0 0..3 (starts and ends on a border), b1, b2 empty, b3 4..9 (starts on a border), b4 10..11 (ends on a border), b5 12..14, b6 empty, b7 15..20 (a middle
    chunk wholly inside it), b8 21..23, b9 24..87 (64 terms, aligned), b10 88..150 (63 terms), b11 151..215 (65 terms), window 1's first bucket 216..217"""
    counts = [4, 0, 0, 6, 2, 3, 0, 6, 3, 64, 63, 65]
    sc = scalars_of(counts) + scalars_of([2], window=1)
    L = U.acc_layout(sc, C8, 4, shared=False)
    assert (L.E, L.T, L.NB, len(L.off)) == (218, 55, 32 * 128, 32 * 128 + 1)
    assert L.off[:13].tolist() == [0, 4, 4, 4, 10, 12, 15, 15, 21, 24, 88, 151, 216] and L.off[128] == 216 and L.off[129] == 218 and L.off[-1] == 218
    assert sorted(L.buckets) == [0, 3, 4, 5, 7, 8, 9, 10, 11, 128]
    assert view(L, 0) == (4, 0, 0, 1, "direct")
    assert view(L, 3) == (6, 1, 2, 2, "fixup")
    assert view(L, 4) == (2, 2, 2, 1, "direct")
    assert view(L, 5) == (3, 3, 3, 1, "direct")
    assert view(L, 7) == (6, 3, 5, 3, "fixup")
    assert view(L, 8) == (3, 5, 5, 1, "direct")
    assert view(L, 9) == (64, 6, 21, 16, "heavy")
    assert view(L, 10) == (63, 22, 37, 16, "fixup")            # one term short of heavy, as many pieces
    assert view(L, 11) == (65, 37, 53, 17, "heavy")
    assert view(L, 128) == (2, 54, 54, 1, "direct")            # the last, partial chunk
    assert L.heavy == [9, 11] and L.multi == [] and all(k.ranges is None for k in L.buckets.values())
    # started_before / complete of k_accumulate: (head slot, tail slot) per chunk
    assert L.chunk_slots(0) == (None, None)                    # b0 fills the chunk: written by the chunk itself
    assert L.chunk_slots(1) == (None, 3)                       # starts on the border, cut on the right
    assert L.chunk_slots(2) == (3, None)                       # b3's rest, then b4 ends with the chunk
    assert L.chunk_slots(3) == (None, 7)                       # b5 whole, empty b6 passed over, b7 cut on the right
    assert L.chunk_slots(4) == (7, None)                       # cut on both sides: the head slot alone
    assert L.chunk_slots(5) == (7, None)
    assert L.chunk_slots(6) == (None, 9) and L.chunk_slots(7) == (9, None) and L.chunk_slots(21) == (9, None)
    assert L.chunk_slots(22) == (None, 10)
    assert L.chunk_slots(37) == (10, 11)                       # the neighbour's head slot and the heavy bucket's tail slot in one chunk
    assert L.chunk_slots(53) == (11, None) and L.chunk_slots(54) == (None, None)


def test_windows_carries_shared_set_and_identity_rows():
    """1 -> digit 1 in window 0; 2^8 -> digit 1 in window 1; 2^9 + 1 -> digits 1 and 2; 200 -> digit -56 in window 0 and the carry, digit 1, in window 1"""
    sc = [1, 1 << 8, (2 << 8) | 1, 200, 0]
    L = U.acc_layout(sc, C8, 16, shared=False)
    assert {b: k.terms for b, k in L.buckets.items()} == {0: 2, 55: 1, 128: 2, 129: 1} and (L.E, L.T) == (6, 1)
    S = U.acc_layout(sc, C8, 16, shared=True)
    assert {b: k.terms for b, k in S.buckets.items()} == {0: 4, 1: 1, 55: 1} and S.NB == 128 and (S.E, S.T) == (6, 1)
    D = U.acc_layout(sc, C8, 16, shared=True, identity_rows=(3,))
    assert {b: k.terms for b, k in D.buckets.items()} == {0: 3, 1: 1} and D.E == 4
    assert U.acc_layout([0, 0], C8, 16, shared=False).E == 0


def test_ranges_by_hand():
    """ch = 2 (heavy from 32 terms; a range = chunks 512 k .. 512 k + 511).  b0 0..2, b1 3..2052 (chunks 1 .. 1026), b2 2053..3076 (chunks 1026 .. 1538),
    b3 3077..4098 (chunks 1538 .. 2049: 512 pieces across the border at 2048, one block), b4 4099..4129 (31 terms)"""
    L = U.acc_layout(scalars_of([3, 2050, 1024, 1022, 31]), C8, 2, shared=False)
    assert view(L, 0) == (3, 0, 1, 2, "fixup")
    assert view(L, 1) == (2050, 1, 1026, 1026, "multi") and L.buckets[1].ranges == [(0, 511), (1, 512), (2, 3)]
    assert view(L, 2) == (1024, 1026, 1538, 513, "multi") and L.buckets[2].ranges == [(2, 510), (3, 3)]
    assert view(L, 3) == (1022, 1538, 2049, 512, "heavy") and L.buckets[3].ranges is None
    assert view(L, 4) == (31, 2049, 2064, 16, "fixup")
    assert L.heavy == [1, 2, 3] and L.multi == [1, 2]
    assert L.chunk_slots(1026) == (1, 2) and L.chunk_slots(1538) == (2, 3)         # a long bucket ends and the next starts inside range 2, and inside range 3


def walk_like_k_accumulate(off, NB, ch):
    """(head_b, tail_b) per chunk and the buckets the chunks write themselves, term by term as K5 does (started_before / complete)"""
    E = int(off[NB])
    T = (E + ch - 1) // ch
    slots, direct = [], set()
    for t in range(T):
        start, end = t * ch, min((t + 1) * ch, E)
        b = max(i for i in range(NB) if off[i] <= start)
        bend, started_before, hb, tb = off[b + 1], off[b] < start, None, None
        for pos in range(start, end):
            if pos == bend:
                if started_before:
                    hb, started_before = b, False
                else:
                    direct.add(b)
                b += 1
                while off[b + 1] == pos:
                    b += 1
                bend = off[b + 1]
        if started_before:
            hb = b
        elif end == bend:
            direct.add(b)
        else:
            tb = b
        slots.append((hb, tb))
    return slots, direct


def test_slots_and_classes_against_a_term_by_term_walk():
    rng = random.Random(7)
    for trial in range(60):
        ch = rng.choice([1, 2, 3, 4, 5, 16])
        counts = [rng.choice([0, 0, 1, 2, ch - 1, ch, ch + 1, 2 * ch, 3 * ch + 1, 16 * ch - 1, 16 * ch, 16 * ch + 1]) for _ in range(rng.randrange(1, 14))]
        if not any(counts):
            counts[0] = 1
        L = U.acc_layout(scalars_of(counts, seed=trial), C8, ch, shared=True)
        slots, direct = walk_like_k_accumulate(L.off.tolist(), L.NB, ch)
        assert [L.chunk_slots(t) for t in range(L.T)] == slots, (ch, counts)
        assert direct == {b for b, k in L.buckets.items() if k.cls == "direct"}, (ch, counts)
        for b, k in L.buckets.items():
            assert k.terms == counts[b] and (k.cls in ("heavy", "multi")) == (k.terms >= 16 * ch)
            if k.cls != "direct":           # the pieces the folds read: the tail slot of chunk t0, then the head slots of t0 + 1 .. t1
                assert slots[k.t0][1] == b and all(slots[t][0] == b for t in range(k.t0 + 1, k.t1 + 1)) and k.pieces >= 2, (ch, counts, b)
                assert k.t1 + 1 == L.T or slots[k.t1 + 1][0] != b


def test_accessor_lives_in_the_twin_only():
    """dgpu_dev_get_acc_last: declared in include/dock_gpu_dev.h, exported by the development twin and not by the product; NULL is refused before anything else"""
    from crypto_amd._native import lib, dev_lib, DEV_SYMBOLS
    assert "dgpu_dev_get_acc_last" in DEV_SYMBOLS and hasattr(dev_lib(), "dgpu_dev_get_acc_last") and not hasattr(lib(), "dgpu_dev_get_acc_last")
    assert dev_lib().dgpu_dev_get_acc_last(None) == -3


def test_closed_form_for_repeated_bases():
    import oracle_c as O
    bases, k0, d = U.seq_bases(O.G1, 4, 77, threads=1)
    sc = [5, 0, (1 << 200) + 3, U.R - 1]
    limbs = np.stack([O.int_to_limbs(s, 4) for s in sc])
    assert U.closed_form_dlogs(O.G1, sc, [k0 + i * d for i in range(4)]) == U.closed_form(O.G1, limbs, k0, d)
    assert U.closed_form_dlogs(O.G1, [3, U.R - 3], [k0, k0]) is None           # + and - the same multiple of one base: the identity
