"""tests/g2_special.py yields what tests/test_gpu_g2_branches.py relies on (CPU only): every crafted category is non-empty,
holds what its name says and gets its expected status / bytes from the oracle, so that no GPU test there can pass for lack of
reaching its branch.  Also the two host-side compressors of the C ABI on the crafted points (no device work)."""
import ctypes as C

import numpy as np

from oracle import g1, g2
from tests import g2_special as S

P = g1.P


def test_rhs_in_fp_points_reach_the_a1_zero_branch():
    r = S.rhs_in_fp_points()
    assert sorted(r) == ["imag", "real"] and len(r["real"]) == 2 and len(r["imag"]) == 2
    xs = set()
    for kind in ("real", "imag"):
        for x, y in r[kind]:
            xs.add(x)
            assert 0 < x[0] < P and 0 < x[1] < P
            a = S.g2_rhs(x)
            assert a[1] == 0 and a[0] != 0                          # the decoder's `a1 == 0` branch
            assert g2.is_on_curve((x, y)) and g2.f2_sqr(y) == a
            is_residue = pow(a[0], (P - 1) // 2, P) == 1
            if kind == "real":
                assert is_residue and y[1] == 0 and y[0] != 0       # y = (t, 0): the sign rule falls to y.c0
            else:
                assert not is_residue and y[0] == 0 and y[1] != 0   # y = (0, t): negating must leave y.c0 = 0, not p
            encs = [g2.compress((x, y)), g2.compress(g2.neg((x, y)))]
            assert encs[0][1:] == encs[1][1:] and encs[0][0] ^ encs[1][0] == 0x20     # bit 5 only
            assert {e[0] & 0x20 for e in encs} == {0, 0x20}
            for pt, e in zip([(x, y), g2.neg((x, y))], encs):
                assert g2.decompress(e) == pt
                half = pt[1][0] if kind == "real" else pt[1][1]
                assert bool(e[0] & 0x20) == (half > (P - 1) // 2)
    assert len(xs) == 4


def test_shared_half_points():
    s = S.shared_half_points()
    assert sorted(s) == ["c0", "c1"]
    (p, q), (v, w) = s["c0"], s["c1"]
    assert p[0][0] == q[0][0] and p[0][1] != q[0][1]                # x differs in the c1 half only
    assert v[0][1] == w[0][1] and v[0][0] != w[0][0]                # x differs in the c0 half only
    for a, b in (s["c0"], s["c1"]):
        assert a != b and g2.is_on_curve(a) and g2.is_on_curve(b)
        assert a[1][0] and a[1][1] and b[1][0] and b[1][1]          # generic ordinates: the general root branch
        t = g2.add(a, b)
        assert t is not None and g2.is_on_curve(t) and t == g2.add(b, a)
        assert g2.add(a, g2.neg(a)) is None


def test_expected_values_of_the_gpu_tests_are_curve_points():
    """oracle.g2.add / double are plain curve arithmetic: they hold outside the r-torsion, where the crafted points lie."""
    pts = S.crafted_points()
    assert len(pts) == 8 and len({name for name, _ in pts}) == 8 and len({p for _, p in pts}) == 8
    outside = 0
    for _, p in pts:
        d = g2.double(p)
        assert d is not None and g2.is_on_curve(d) and d == g2.add(p, p) == g2.mul(2, p)
        assert g2.add(p, g2.neg(p)) is None and g2.add(g2.neg(p), p) is None
        assert g2.sum_points([p, g2.neg(p), g2.G2]) == g2.G2
        in_g2 = g2.mul(g1.R_ORDER, p) is None
        assert (g2.mul(g1.R_ORDER, d) is None) == in_g2
        outside += not in_g2
    assert outside >= 1                                             # the subgroup test sees at least one status 3


def _oracle_says(decompress, enc):
    try:
        return decompress(enc), None
    except ValueError as err:
        return None, str(err)


def test_boundary_encodings_carry_the_oracles_status():
    for make, dec, comp, width in ((S.g1_boundary_encodings, g1.decompress, g1.compress, 48),
                                   (S.g2_boundary_encodings, g2.decompress, g2.compress, 96)):
        cases = make()
        names = [n for n, _, _ in cases]
        assert len(cases) >= 20 and len(set(names)) == len(names) and len({e for _, e, _ in cases}) == len(cases)
        assert {st for _, _, st in cases} == {0, 1, 2}
        for name, enc, st in cases:
            assert len(enc) == width
            pt, err = _oracle_says(dec, enc)
            assert st == (0 if err is None else 2 if err == "not on the curve" else 1), name
            if err is None:
                assert comp(pt) == enc, name                        # accepted encodings are the canonical ones
    g1c = {n: (e, st) for n, e, st in S.g1_boundary_encodings()}
    s0, s1 = S.g1_small_abscissas(2)
    assert s0 == 0 and s1 > 0
    for s in (s0, s1):
        assert g1.is_on_curve(g1.decompress(S._be48(s, 0x80)))
    # what the decoders must REJECT although the reduced x is a fine abscissa
    assert g1c["x=p"][1] == 1 and g1c["x=p+s"][1] == 1 and g1c["x=0"][1] == 0 and g1c["x=s"][1] == 0
    assert int.from_bytes(g1c["x=p+s"][0], "big") & ((1 << 381) - 1) == P + s1
    assert g1c["infinity,last_byte"][1] == 1 and g1c["infinity,sign"][1] == 1 and g1c["no_flags,x=G"][1] == 1
    assert g1c["x=G"][1] == 0 and g1c["x=G,sign"][1] == 0
    g2c = {n: (e, st) for n, e, st in S.g2_boundary_encodings()}
    assert g2c["valid"][1] == 0 and g2c["valid,sign"][1] == 0
    for name in ("c1=p", "c0=p", "c0=p+s", "c1=p+s", "c0|0x80", "c0|0x40", "c0|0x20", "infinity,c0_last_byte",
                 "infinity,c1_middle_byte", "infinity,sign"):
        assert g2c[name][1] == 1, name
    for name, half in (("c0=p+s", slice(48, 96)), ("c1=p+s", slice(0, 48))):   # reduced mod p it IS on the curve
        e = bytearray(g2c[name][0])
        v = (int.from_bytes(e[half], "big") & ((1 << 381) - 1)) - P
        assert 0 < v < S.SEARCH_BOUND + 1
        e[half] = v.to_bytes(48, "big")
        e[0] |= 0x80
        assert g2.is_on_curve(g2.decompress(bytes(e)))
    for flag in (0x80, 0x40, 0x20):                                 # only the flag differs from a valid encoding
        e = bytearray(g2c[f"c0|{flag:#04x}"][0])
        e[48] &= 0x1F
        assert bytes(e) == g2c["valid"][0]


def test_no_g1_point_on_the_boundary_of_the_sign_rule():
    """y = (p - 1)/2 and y = (p + 1)/2 would sit on the two sides of `limbs_gt(plain, FP_HALF)`.  Both need
    x^3 = y^2 - 4 = -15/4, which is NOT a cubic residue mod p: the curve has no such point, so no key can probe that
    comparison at equality and the GPU tests feed none."""
    assert P % 3 == 1
    assert not S.g1_half_boundary_abscissa_exists()
    for y in ((P - 1) // 2, (P + 1) // 2):
        assert pow((y * y - 4) % P, (P - 1) // 3, P) != 1


def test_c_abi_compressors_on_crafted_points():
    """pe_g2_compress's `y.c1 == 0 ? y.c0 : y.c1` rule (engine_g1.cpp, pe_g2_compress) and pe_g1_compress on points a
    generic input never offers: ordinates with a zero half, both signs, abscissas 0 and p - 1."""
    from pos_evolution_amd import _abi
    lib = _abi.load()
    u8 = C.POINTER(C.c_uint8)
    pts2 = [q for _, p in S.crafted_points() for q in (p, g2.neg(p), g2.double(p))] + [None]
    pts2 += [g2.decompress(e) for _, e, st in S.g2_boundary_encodings() if st == 0]
    assert sum(1 for p in pts2 if p is not None and p[1][1] == 0) >= 4 and sum(1 for p in pts2 if p is not None and p[1][0] == 0) >= 4
    raw = np.frombuffer(b"".join(g2.to_bytes192(p) for p in pts2), dtype=np.uint8).copy()
    out = np.zeros(96 * len(pts2), dtype=np.uint8)
    assert lib.pe_g2_compress(raw.ctypes.data_as(u8), len(pts2), out.ctypes.data_as(u8)) == 0
    for i, p in enumerate(pts2):
        assert out[96 * i:96 * i + 96].tobytes() == g2.compress(p), i
    pts1 = [g1.decompress(e) for _, e, st in S.g1_boundary_encodings() if st == 0]
    assert len(pts1) >= 7 and None in pts1
    raw = np.frombuffer(b"".join(g1.to_bytes96(p) for p in pts1), dtype=np.uint8).copy()
    out = np.zeros(48 * len(pts1), dtype=np.uint8)
    assert lib.pe_g1_compress(raw.ctypes.data_as(u8), len(pts1), out.ctypes.data_as(u8)) == 0
    for i, p in enumerate(pts1):
        assert out[48 * i:48 * i + 48].tobytes() == g1.compress(p), i
