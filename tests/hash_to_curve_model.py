"""hash_to_curve for G2, suite BLS12381G2_XMD:SHA-256_SSWU_RO_ (RFC 9380), in plain Python: hashlib and oracle/g2.py's Fp2.
THE SPECIFICATION of pe_hash_to_g2 / pe_map_to_g2 (include/posevo.h): the GPU tests compare byte for byte with this file.

    hash_to_g2(msg, dst) = clear_cofactor(iso3(map_to_curve_g2(u0)) + iso3(map_to_curve_g2(u1))),  (u0, u1) = hash_to_field

Nothing here is copied from a table.  The simplified SWU map lands on E': y^2 = x^3 + A' x + B' (A' = 240 i, B' = 1012 (1 + i));
the 3-isogeny E' -> E2 is DERIVED: its kernel {O, (x0, +-y0)} with x0 = -6 + 6 i (a root of E''s 3-division polynomial), Velu's
formulas, and the scaling by 3 that turns the image curve y^2 = x^3 + 4 (1 + i) 3^6 into E2.  What Velu leaves open -- the sign
of Y -- is fixed by the two known answers of the RFC (tests/golden/hash_to_curve_vectors.json), asserted at import together
with the derivation's own identities; both known answers lie on E2, which a misremembered digit cannot do.
"""
import hashlib
import json
import os

from oracle import g2
from oracle.g1 import P, R_ORDER

ETH2_DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
C_PARAM = -0xD201000000010000            # the curve's parameter (z of the subgroup check)

A_ISO = (0, 240)                         # E'
B_ISO = (1012, 1012)
Z_SWU = (P - 2, P - 1)                   # -(2 + i)
X0 = (P - 6, 6)                          # x of the isogeny's kernel points
F2 = g2


def _f(v):
    return (v % P, 0)


def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = F2.f2_mul(r, a)
        a = F2.f2_sqr(a)
        e >>= 1
    return r


def f2_is_square(a):
    return a == (0, 0) or pow((a[0] * a[0] + a[1] * a[1]) % P, (P - 1) // 2, P) == 1


def sgn0(a):
    return a[0] & 1 if a[0] else a[1] & 1


# ---------------------------------------------------------------- 1. hash_to_field
def expand_message_xmd(msg, dst, n_bytes):
    assert 1 <= len(dst) <= 255 and n_bytes <= 255 * 32
    ell = (n_bytes + 31) // 32
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + n_bytes.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    b = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(b)[:n_bytes]


def hash_to_field(msg, dst):
    """(u0, u1): four 64-byte big-endian integers mod p, (e0, e1), (e2, e3)."""
    uniform = expand_message_xmd(msg, dst, 256)
    e = [int.from_bytes(uniform[64 * k:64 * k + 64], "big") % P for k in range(4)]
    return (e[0], e[1]), (e[2], e[3])


# ---------------------------------------------------------------- 2. simplified SWU onto E'
def g_iso(x):
    return F2.f2_add(F2.f2_add(F2.f2_mul(F2.f2_sqr(x), x), F2.f2_mul(A_ISO, x)), B_ISO)


def swu_takes_x1(u):
    """Whether g(x1) is a square for this u (the branch map_to_curve_g2 takes): for the tests' branch coverage."""
    return f2_is_square(g_iso(_swu_x1(u)))


def _swu_x1(u):
    zu2 = F2.f2_mul(Z_SWU, F2.f2_sqr(u))
    tv1 = F2.f2_add(F2.f2_sqr(zu2), zu2)
    if tv1 == (0, 0):
        return F2.f2_mul(B_ISO, F2.f2_inv(F2.f2_mul(Z_SWU, A_ISO)))
    mba = F2.f2_neg(F2.f2_mul(B_ISO, F2.f2_inv(A_ISO)))
    return F2.f2_mul(mba, F2.f2_add((1, 0), F2.f2_inv(tv1)))


def map_to_curve_g2(u):
    """u in Fp2 -> a point of E' (never the identity)."""
    x1 = _swu_x1(u)
    gx = g_iso(x1)
    x = x1
    if not f2_is_square(gx):
        x = F2.f2_mul(F2.f2_mul(Z_SWU, F2.f2_sqr(u)), x1)
        gx = g_iso(x)
    y = F2.f2_sqrt(gx)
    assert y is not None and F2.f2_sqr(y) == gx
    if sgn0(y) != sgn0(u):
        y = F2.f2_neg(y)
    return (x, y)


# ---------------------------------------------------------------- 3. the 3-isogeny E' -> E2, by Velu
Y0_SQ = g_iso(X0)
V_VELU = F2.f2_add(F2.f2_scalar(F2.f2_sqr(X0), 6), F2.f2_scalar(A_ISO, 2))     # 2 (3 x0^2 + A') for a kernel of order 3
UQ_VELU = F2.f2_scalar(Y0_SQ, 4)
Y_SIGN = -1                                                                      # fixed by the known answers below
INV9, INV27 = pow(9, -1, P), pow(27, -1, P)


def iso3(pt):
    """A point of E' -> the point of E2 (None: the identity; the kernel points go there)."""
    if pt is None:
        return None
    x, y = pt
    d = F2.f2_sub(x, X0)
    if d == (0, 0):
        return None
    di = F2.f2_inv(d)
    di2 = F2.f2_sqr(di)
    X = F2.f2_add(x, F2.f2_add(F2.f2_mul(V_VELU, di), F2.f2_mul(UQ_VELU, di2)))
    Y = F2.f2_mul(y, F2.f2_sub(F2.f2_sub((1, 0), F2.f2_mul(V_VELU, di2)),
                               F2.f2_mul(F2.f2_scalar(UQ_VELU, 2), F2.f2_mul(di2, di))))
    return (F2.f2_scalar(X, INV9), F2.f2_scalar(Y, Y_SIGN * INV27))


# ---------------------------------------------------------------- 4. cofactor clearing
CX = F2.f2_inv(f2_pow((1, 1), (P - 1) // 3))
CY = F2.f2_inv(f2_pow((1, 1), (P - 1) // 2))


def psi(pt):
    if pt is None:
        return None
    (x0, x1), (y0, y1) = pt
    return (F2.f2_mul((x0, -x1 % P), CX), F2.f2_mul((y0, -y1 % P), CY))


def curve_mul(k, pt):
    """[k] pt on E2 for ANY point of the curve (oracle.g2.mul reduces k as if pt had order r)."""
    if k < 0:
        return curve_mul(-k, F2.neg(pt))
    acc, base = F2._to_jac(None), F2._to_jac(pt)
    while k:
        if k & 1:
            acc = F2._jac_add(acc, base)
        base = F2._jac_double(*base)
        k >>= 1
    return F2._from_jac(acc)


def clear_cofactor(pt):
    """[c^2 - c - 1] P + [c - 1] psi(P) + psi^2(2 P), as the sequence the kernel runs."""
    t1 = curve_mul(C_PARAM, pt)
    t2 = psi(pt)
    t3 = F2.add(psi(psi(F2.double(pt))), F2.neg(t2))
    t2 = curve_mul(C_PARAM, F2.add(t1, t2))
    q = F2.add(t3, t2)
    q = F2.add(q, F2.neg(t1))
    return F2.add(q, F2.neg(pt))


def map_to_g2(u0, u1):
    """Steps 2-4: what pe_map_to_g2 computes."""
    q0, q1 = iso3(map_to_curve_g2(u0)), iso3(map_to_curve_g2(u1))
    out = clear_cofactor(F2.add(q0, q1))
    assert F2.is_on_curve(out) and curve_mul(R_ORDER, out) is None
    return out


def hash_to_g2(msg, dst=ETH2_DST):
    return map_to_g2(*hash_to_field(msg, dst))


def u_to_bytes(u0, u1):
    """The 192 bytes pe_map_to_g2 takes per point: u0.c0 | u0.c1 | u1.c0 | u1.c1, 48-byte big-endian each."""
    return b"".join(v.to_bytes(48, "big") for v in (u0[0], u0[1], u1[0], u1[1]))


# ---------------------------------------------------------------- the derivation's identities and the known answers
def _check_derivation():
    a, b, x = A_ISO, B_ISO, X0
    x2 = F2.f2_sqr(x)
    div3 = F2.f2_sub(F2.f2_add(F2.f2_add(F2.f2_scalar(F2.f2_sqr(x2), 3), F2.f2_scalar(F2.f2_mul(a, x2), 6)),
                               F2.f2_scalar(F2.f2_mul(b, x), 12)), F2.f2_sqr(a))
    assert div3 == (0, 0), "x0 is not a root of the 3-division polynomial"
    assert V_VELU == (0, 48) and UQ_VELU == (16, 16)
    assert F2.f2_sub(a, F2.f2_scalar(V_VELU, 5)) == (0, 0)
    w = F2.f2_add(UQ_VELU, F2.f2_mul(x, V_VELU))
    assert F2.f2_sub(b, F2.f2_scalar(w, 7)) == F2.f2_scalar(F2.B2, 3 ** 6)
    assert not f2_is_square(Z_SWU)


def load_vectors():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_to_curve_vectors.json")) as f:
        return json.load(f)


def _check_known_answers():
    v = load_vectors()
    for case in v["expander"]:
        got = expand_message_xmd(case["msg"].encode(), v["expander_dst"].encode(), case["len"])
        assert got.hex() == case["uniform_bytes"], case["msg"]
    for case in v["points"]:
        want = (tuple(int(t, 16) for t in case["x"]), tuple(int(t, 16) for t in case["y"]))
        assert F2.is_on_curve(want), "a known answer off the curve"
        assert hash_to_g2(case["msg"].encode(), v["dst"].encode()) == want, case["msg"]


_check_derivation()
_check_known_answers()
