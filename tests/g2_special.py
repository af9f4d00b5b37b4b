"""Crafted curve points and wire encodings that reach the branches generic points (multiples of a generator) cannot.

A helper module (like tests/fc_scenarios.py), plain Python integers over oracle/g1.py / oracle/g2.py.  Everything here is
deterministic, every search has a fixed bound and raises at it.  tests/test_oracle_g2_special.py checks on the CPU that
each constructor yields what its name says, so that a GPU test built on it cannot pass for lack of reaching its branch.

E'(Fp2): y^2 = x^3 + 4(1 + u).  With x = x0 + x1 u:  Im(x^3 + 4 + 4u) = 3 x0^2 x1 - x1^3 + 4, which vanishes exactly when
x0^2 = (x1^3 - 4) / (3 x1).  Then the right-hand side a = a0 lies in Fp and, -1 being a non-residue (p = 3 mod 4), its
square root in Fp2 is (t, 0) when a0 is a residue and (0, t) with t^2 = -a0 otherwise.
"""
from oracle import g1, g2

P = g1.P
SEARCH_BOUND = 64           # candidates tried per search before it fails (each succeeds with probability >= 1/4)
STATUS_OK, STATUS_MALFORMED, STATUS_OFF_CURVE = 0, 1, 2


def fp_sqrt(v):
    r = pow(v % P, (P + 1) // 4, P)
    return r if r * r % P == v % P else None


def g2_rhs(x):
    """x^3 + 4(1 + u)"""
    return g2.f2_add(g2.f2_mul(g2.f2_sqr(x), x), g2.B2)


# ---------------------------------------------------------------- points whose right-hand side lies in Fp
def rhs_in_fp_points():
    """-> {"real": [P, P'], "imag": [Q, Q']}: curve points with x^3 + 4(1+u) in Fp; "real" have y = (t, 0) (y.c1 == 0),
    "imag" have y = (0, t) (y.c0 == 0).  The first two of each kind over x1 = 1, 2, 3, ..., x0 the smaller root of
    (x1^3 - 4) / (3 x1); y as oracle.g2.f2_sqrt returns it."""
    out = {"real": [], "imag": []}
    for x1 in range(1, SEARCH_BOUND + 1):
        x0 = fp_sqrt((x1 ** 3 - 4) * pow(3 * x1, -1, P))
        if x0 is None:
            continue
        x = (min(x0, P - x0), x1)
        a = g2_rhs(x)
        assert a[1] == 0 and a[0] != 0
        y = g2.f2_sqrt(a)
        kind = "real" if y[1] == 0 else "imag"
        if len(out[kind]) < 2:
            out[kind].append((x, y))
        if len(out["real"]) == 2 and len(out["imag"]) == 2:
            return out
    raise AssertionError(f"rhs_in_fp_points: {SEARCH_BOUND} candidates gave only "
                         f"{len(out['real'])} real and {len(out['imag'])} imaginary roots")


def _walk_on_curve(make_x, count):
    found = []
    for v in range(1, SEARCH_BOUND + 1):
        x = make_x(v)
        y = g2.f2_sqrt(g2_rhs(x))
        if y is not None:
            found.append((x, y))
            if len(found) == count:
                return found
    raise AssertionError(f"_walk_on_curve: {len(found)} of {count} points in {SEARCH_BOUND} candidates")


def shared_half_points():
    """-> {"c0": (P, Q), "c1": (P, Q)}: "c0" two curve points with equal x.c0 (= 1) and different x.c1; "c1" two with
    equal x.c1 (= 3) and different x.c0.  Their x difference is zero in ONE half only; the four points are distinct."""
    return {"c0": tuple(_walk_on_curve(lambda v: (1, v), 2)), "c1": tuple(_walk_on_curve(lambda v: (v, 3), 2))}


def crafted_points():
    """Every crafted G2 point as a flat, named list: [(name, point)]."""
    r, s = rhs_in_fp_points(), shared_half_points()
    return ([(f"real{i}", p) for i, p in enumerate(r["real"])] + [(f"imag{i}", p) for i, p in enumerate(r["imag"])] +
            [(f"same_c0_{i}", p) for i, p in enumerate(s["c0"])] + [(f"same_c1_{i}", p) for i, p in enumerate(s["c1"])])


# ---------------------------------------------------------------- wire-format boundaries
def oracle_status(decompress, enc):
    """The status a decoder must give `enc`, from the ORACLE: it returns -> 0; ValueError "not on the curve" -> 2; any other
    ValueError -> 1 (malformed: no compression flag, malformed infinity, x not canonical)."""
    try:
        decompress(bytes(enc))
    except ValueError as err:
        return STATUS_OFF_CURVE if str(err) == "not on the curve" else STATUS_MALFORMED
    return STATUS_OK


def _be48(v, flags=0):
    b = bytearray(v.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def g1_small_abscissas(count=2):
    """The smallest s >= 0 with s^3 + 4 a square (s = 0 is one: y = 2)."""
    found = []
    for s in range(SEARCH_BOUND):
        if fp_sqrt(s ** 3 + 4) is not None:
            found.append(s)
            if len(found) == count:
                return found
    raise AssertionError("g1_small_abscissas: search bound reached")


def g1_off_curve_abscissa():
    for s in range(SEARCH_BOUND):
        if fp_sqrt(s ** 3 + 4) is None:
            return s
    raise AssertionError("g1_off_curve_abscissa: search bound reached")


def g1_boundary_encodings():
    """-> [(name, 48 bytes, status the oracle gives it)]"""
    s0, s1 = g1_small_abscissas(2)
    gx = g1.G[0]
    cases = [
        ("x=p", _be48(P, 0x80)),                                  # = p + s0: s0 = 0 is on the curve
        ("x=p,sign", _be48(P, 0xA0)),
        ("x=p-1", _be48(P - 1, 0x80)),
        ("x=p-1,sign", _be48(P - 1, 0xA0)),
        ("x=p+s", _be48(P + s1, 0x80)),                            # a decoder that reduced would accept it
        ("x=p+s,sign", _be48(P + s1, 0xA0)),
        ("x=2^381-1", _be48((1 << 381) - 1, 0x80)),
        ("x=0", _be48(s0, 0x80)),
        ("x=0,sign", _be48(s0, 0xA0)),
        ("x=s", _be48(s1, 0x80)),
        ("x=s,sign", _be48(s1, 0xA0)),
        ("x=G", _be48(gx, 0x80)),
        ("x=G,sign", _be48(gx, 0xA0)),
        ("off_curve", _be48(g1_off_curve_abscissa(), 0x80)),
        ("infinity", _be48(0, 0xC0)),
        ("infinity,last_byte", bytes([0xC0]) + bytes(46) + b"\x01"),
        ("infinity,sign", _be48(0, 0xE0)),
        ("infinity,x=G", _be48(gx, 0xC0)),
        ("no_flags,x=G", _be48(gx, 0x00)),
        ("sign_only,x=G", _be48(gx, 0x20)),
        ("infinity_uncompressed", _be48(0, 0x40)),
    ]
    return [(name, enc, oracle_status(g1.decompress, enc)) for name, enc in cases]


def g2_boundary_encodings():
    """-> [(name, 96 bytes x.c1 | x.c0, status the oracle gives it)]; the valid x is that of the shared-half pairs."""
    sh = shared_half_points()
    (v0, v1), _ = sh["c0"][0]                                      # x.c0 = 1, x.c1 = v1: on the curve
    # smallest s with (s, v1) on the curve / (v0, s) on the curve: p + s in that half is what a reducing decoder accepts
    s_c0 = _walk_on_curve(lambda v: (v, v1), 1)[0][0][0]
    s_c1 = _walk_on_curve(lambda v: (v0, v), 1)[0][0][1]

    def enc(c1, c0, flags=0x80, c0_flags=0):
        return _be48(c1, flags) + _be48(c0, c0_flags)

    mid = bytearray(enc(0, 0, 0xC0))
    mid[24] = 0x01
    cases = [
        ("valid", enc(v1, v0)),
        ("valid,sign", enc(v1, v0, 0xA0)),
        ("c1=p", enc(P, v0)),
        ("c0=p", enc(v1, P)),
        ("c1=p-1", enc(P - 1, v0)),
        ("c0=p-1", enc(v1, P - 1)),
        ("c1=p-1,c0=p-1", enc(P - 1, P - 1)),
        ("c0=p+s", enc(v1, P + s_c0)),
        ("c0=p+s,sign", enc(v1, P + s_c0, 0xA0)),
        ("c1=p+s", enc(P + s_c1, v0)),
        ("c1=p,c0=p", enc(P, P)),
        ("c1=2^381-1", enc((1 << 381) - 1, v0)),
        ("c0|0x80", enc(v1, v0, c0_flags=0x80)),                   # the leading byte of x.c0 carries no flags
        ("c0|0x40", enc(v1, v0, c0_flags=0x40)),
        ("c0|0x20", enc(v1, v0, c0_flags=0x20)),
        ("x=0", enc(0, 0)),
        ("infinity", enc(0, 0, 0xC0)),
        ("infinity,sign", enc(0, 0, 0xE0)),
        ("infinity,c0_last_byte", enc(0, 1, 0xC0)),
        ("infinity,c1_middle_byte", bytes(mid)),
        ("infinity,c0|0x80", enc(0, 0, 0xC0, c0_flags=0x80)),
        ("no_flags", enc(v1, v0, 0x00)),
        ("sign_only", enc(v1, v0, 0x20)),
        ("infinity_uncompressed", enc(0, 0, 0x40)),
    ]
    return [(name, e, oracle_status(g2.decompress, e)) for name, e in cases]


# ---------------------------------------------------------------- a G1 point on the boundary of the sign rule
def g1_half_boundary_abscissa_exists():
    """Is there a G1 curve point with y = (p - 1)/2 or y = (p + 1)/2, the two sides of `y > (p - 1)/2`?  Each is the other's
    negative, so they share x with x^3 = y^2 - 4 = 1/4 - 4 = -15/4; p = 1 mod 3, so that is a cube iff its (p-1)/3-th power
    is 1.  It is not (tests/test_oracle_g2_special.py asserts so): no key can sit on that boundary, and no test feeds one."""
    c = (pow(4, -1, P) - 4) % P
    return pow(c, (P - 1) // 3, P) == 1
