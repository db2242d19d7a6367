"""GPU parity: fixed-base batch multiplication (WindowTable, utils/src/msm.rs:8-62; FixedBase::msm of
legogroth16/src/generator.rs:335-399) against the CPU oracle's double-and-add, through the C ABI.

Follows the reference's own test (utils/src/msm.rs:196-231: `table.multiply_many(&scalars)[i] == g * scalars[i]`).

The second half checks EVERY row of dgpu_window_table_mul_*, dgpu_fixed_base_* and the resident form (dgpu_window_table_mul_to_bases_*, read back with
dgpu_bases_read_*) against the oracle at the sizes around k_fb_mul's 64-lane blocks, on the byte-digit edges of each of the 32 windows, on bases whose
table rows coincide, and on canonical scalars at and above r — the only inputs that take xyzz_madd's P = Q and P = -Q fix-ups in k_fb_mul."""
import numpy as np
import pytest
import torch
import oracle_c as O
import util as U
import crypto_amd as ca
from crypto_amd import fixed_base as fb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available()
    ca.init(0)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _expect(grp, base, scalars):
    exp = [grp.to_affine(grp.mul(base, s)) for s in scalars]
    return np.stack([e[0] for e in exp]), np.array([e[1] for e in exp], dtype=np.uint8)


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_multiply_many_matches_double_and_add(curve):
    grp, cv = (O.G1, ca.G1) if curve == "g1" else (O.G2, ca.G2)
    base = grp.to_affine(grp.mul(grp.generator(), O.int_to_limbs(0xB16B00B5, 4)))[0]
    n = 300
    s = O.rand_scalars(0x51DE + (curve == "g2"), n)
    # edge scalars: 0, 1, r-1, a single top byte, all bytes 0xff below r, zero bytes inside
    edge = [0, 1, R - 1, 0x73 << 248, (1 << 248) - 1, 0x0100000000000000FF, 2, 255, 256]
    for k, v in enumerate(edge):
        s[k] = O.int_to_limbs(v, 4)
    exp_xy, exp_inf = _expect(grp, base, s)
    with fb.WindowTable(cv, base, n) as t:
        out, inf = t.multiply_many(s)
        assert (inf == exp_inf).all() and inf[0] == 1 and inf[1:].sum() == 0
        assert (out == exp_xy).all()
        one, one_inf = t.multiply(5)
        assert not one_inf and (one == grp.to_affine(grp.mul(base, O.int_to_limbs(5, 4)))[0]).all()
        # Montgomery-form scalars (what &[Fr] holds)
        out_m, inf_m = t.multiply_many(O.fr_to_mont(s), montgomery=True)
        assert (out_m == exp_xy).all() and (inf_m == exp_inf).all()
    out2, inf2 = fb.multiply_field_elems_with_same_group_elem(cv, base, s)
    assert (out2 == exp_xy).all() and (inf2 == exp_inf).all()


def test_identity_base_and_empty():
    s = O.rand_scalars(7, 10)
    out, inf = fb.multiply_field_elems_with_same_group_elem(ca.G1, np.zeros(12, dtype=np.uint64), s)
    assert inf.all() and not out.any()
    out, inf = fb.multiply_field_elems_with_same_group_elem(ca.G2, O.G2.generator(), np.zeros((0, 4), dtype=np.uint64))
    assert out.shape == (0, 24) and inf.shape == (0,)


def test_large_batch_sum_property():
    """n = 2^16: sum_i (s_i * B) == (sum_i s_i) * B  (checked with the oracle's point addition through an MSM of ones)"""
    n = 1 << 16
    s = O.rand_scalars(99, n)
    base = O.G1.generator()
    out, inf = fb.multiply_field_elems_with_same_group_elem(ca.G1, base, s)
    assert not inf.any()
    ones = np.zeros((n, 4), dtype=np.uint64); ones[:, 0] = 1
    total = ca.msm_bigint(ca.G1, out, ones)
    ssum = sum(O.limbs_to_int(x) for x in s) % R
    exp = O.G1.to_affine(O.G1.mul(base, O.int_to_limbs(ssum, 4)))[0]
    assert (O.G1.to_affine(total)[0] == exp).all()
    # spot-check individual outputs
    for i in (0, 1, n // 2, n - 1):
        assert (out[i] == O.G1.to_affine(O.G1.mul(base, s[i]))[0]).all()


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_products_as_resident_bases(curve):
    """multiply_many_to_bases + MSM on the handle == MSM over the downloaded products == (sum_i t_i s_i) * B"""
    grp, cv = (O.G1, ca.G1) if curve == "g1" else (O.G2, ca.G2)
    n = 5000
    s = O.rand_scalars(11, n); t = O.rand_scalars(12, n)
    s[3] = 0                                  # an identity among the bases
    with fb.WindowTable(cv, grp.generator()) as tab:
        db = tab.multiply_many_to_bases(s)
        got = db.msm_bigint(t)
        out, inf = tab.multiply_many(s)
        assert inf[3] == 1
        assert (got == ca.msm_bigint(cv, out, t, is_inf=inf)).all()
        acc = sum(O.limbs_to_int(a) * O.limbs_to_int(b) for a, b in zip(s, t)) % R
        assert (grp.to_affine(got)[0] == grp.to_affine(grp.mul(grp.generator(), O.int_to_limbs(acc, 4)))[0]).all()
        db.free()


# ================================================ every row, every entry point ================================================
def lim(vals):
    """ints below 2^256 -> (n, 4) canonical limbs, NOT reduced mod r"""
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def rows_oracle(grp, base, values):
    """(rows, flags) of (v mod r) * base by the oracle's double-and-add on a pool of host threads: what `the integer v times the base` is in a group
    of order r; an identity row is zero words with the flag set"""
    if not np.asarray(base).any():
        return np.zeros((len(values), grp.AW), np.uint64), np.ones(len(values), np.uint8)
    sc = lim([v % R for v in values])
    return U.plus_addends(grp, U.scaled_jac(grp, np.broadcast_to(np.asarray(base, np.uint64), (len(values), grp.AW)), None, sc), None, None)


def every_way(cv, base, sc):
    """[(entry point, rows, flags)] of the same canonical scalars through the table, the one-shot call and the resident form read back"""
    with fb.WindowTable(cv, base, len(sc)) as t:
        out = [("dgpu_window_table_mul",) + t.multiply_many(sc)]
        db = t.multiply_many_to_bases(sc)
        try:
            out.append(("dgpu_window_table_mul_to_bases + dgpu_bases_read",) + tuple(db.read()))
        finally:
            db.free()
    out.append(("dgpu_fixed_base",) + fb.multiply_field_elems_with_same_group_elem(cv, base, sc))
    return out


def check_rows(cv, base, values, want, what):
    sc = lim(values)
    for name, got, ginf in every_way(cv, base, sc):
        bad = U.first_bad(got, ginf, want[0], want[1])
        assert len(bad) == 0, (what, name, [(int(i), hex(values[int(i)])) for i in bad])


def some_base(grp, k=0xB16B00B5):
    return grp.to_affine(grp.mul(grp.generator(), O.int_to_limbs(k, 4)))[0]


@pytest.mark.parametrize("curve,n", [("g1", n) for n in (1, 63, 64, 65, 4097)] + [("g2", n) for n in (1, 63, 65, 1025)])
def test_every_row_at_the_block_borders(curve, n):
    """k_fb_mul runs one scalar per lane in blocks of 64: a block short of one lane, full, one lane into the next, many blocks and one lane; the
    scalar 0 (the identity: no table entry is read) at the first and last row and on both sides of the first and the last 64-lane border"""
    grp, cv = (O.G1, ca.G1) if curve == "g1" else (O.G2, ca.G2)
    base = some_base(grp)
    values = [O.limbs_to_int(x) for x in O.rand_scalars(0xF1B + n + (curve == "g2"), n)]
    zeros = sorted(i for i in {0, n - 1, 63, 64, 64 * ((n - 1) // 64) - 1, 64 * ((n - 1) // 64)} if 0 <= i < n)
    if n > 1:
        for i in zeros:
            values[i] = 0
    want = rows_oracle(grp, base, values)
    if n > 1:
        assert want[1][zeros].all() and want[1].sum() == len(zeros)
    check_rows(cv, base, values, want, (curve, n))
    with fb.WindowTable(cv, base) as t:                                  # Montgomery-form scalars (what &[Fr] holds) through the same launch
        got, ginf = t.multiply_many(O.fr_to_mont(lim(values)), montgomery=True)
        assert len(U.first_bad(got, ginf, want[0], want[1])) == 0
    if n == 1:                                                          # ... and the lone row as the identity
        check_rows(cv, base, [0], rows_oracle(grp, base, [0]), (curve, n, "zero"))


# a single non-zero byte at each of the 32 positions with the smallest and the largest digit (255 << 248 is above r: see SPECIAL), every byte 255
# below r and the neighbours of r - 1, alternating zero / non-zero bytes in both phases
DIGIT_EDGES = [d << (8 * k) for k in range(32) for d in (1, 255)] + [(1 << 248) - 1, R - 1, R - 2, R - 3, R - 256, R - 257] + \
              [int.from_bytes(bytes(pat) * 16, "little") for pat in ((0xFF, 0), (0, 0xFF), (1, 0), (0, 1), (0x5A, 0), (0, 0x5A))]
# canonical scalars at and above r.  k_fb_mul adds the table entry of the top byte d last, to the running sum (s mod 2^248) B:
#   r, 2 r                             the sum is minus the entry: the identity must come out
#   (d << 248) + (d 2^248 - j r)       (d, j) = (0x74, 1), (0xE8, 2): the sum IS the entry, the addition must double
# (no other 256-bit value reaches either case: test_scalars_at_and_above_r enumerates the top byte), and their neighbours
SPECIAL = [R, 2 * R, (0x74 << 248) + ((0x74 << 248) - R), (0xE8 << 248) + ((0xE8 << 248) - 2 * R), R + 1, 2 * R - 1, 2 * R + 1, 1 << 255, (1 << 256) - 1]


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_byte_digit_edges_of_every_window(curve):
    grp, cv = (O.G1, ca.G1) if curve == "g1" else (O.G2, ca.G2)
    base = some_base(grp)
    check_rows(cv, base, DIGIT_EDGES, rows_oracle(grp, base, DIGIT_EDGES), curve)


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_scalars_at_and_above_r(curve):
    """canonical mode takes any 256-bit integer (include/dock_gpu.h): the product is the integer times the base.  The values are repeated over more
    than two blocks so that each meets different lanes."""
    reach = {(d << 248) + low for d in range(1, 256) for low in (((d << 248) % R), ((-d << 248) % R)) if low < (1 << 248)}
    assert reach == set(SPECIAL[:4]) and all(v < (1 << 256) for v in SPECIAL)
    grp, cv = (O.G1, ca.G1) if curve == "g1" else (O.G2, ca.G2)
    base = some_base(grp)
    values = (SPECIAL * 15)[:131]
    want = rows_oracle(grp, base, values)
    assert all(bool(want[1][i]) == (v % R == 0) for i, v in enumerate(values))
    dbl = grp.to_affine(grp.mul(base, O.int_to_limbs((2 * (0x74 << 248)) % R, 4)))[0]
    assert (want[0][2] == dbl).all()                                    # (what the doubling case must give: twice the top byte's entry)
    check_rows(cv, base, values, want, curve)


@pytest.mark.parametrize("curve", ["g1", "g2"])
@pytest.mark.parametrize("k", [0, 1, 2, 255])
def test_bases_whose_table_rows_coincide(curve, k):
    """the identity as the base (k = 0: every product is the identity) and k G for small k (T[0][1] of G is T[0][0] of 2 G, T[1][0] of G is 256 G,
    next to T[0][254] of ...): nothing special is expected, every row is the oracle's"""
    grp, cv = (O.G1, ca.G1) if curve == "g1" else (O.G2, ca.G2)
    base = some_base(grp, k) if k else np.zeros(grp.AW, np.uint64)
    values = DIGIT_EDGES[::3] + SPECIAL + [O.limbs_to_int(x) for x in O.rand_scalars(0xBA5E + k, 40)] + [0, 1, 2, 255, 256, 257]
    want = rows_oracle(grp, base, values)
    if not k:
        assert want[1].all()
    check_rows(cv, base, values, want, (curve, k))
