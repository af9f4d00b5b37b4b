"""The wire rules of the uncompressed point forms the pairing calls take, restated in plain integers (include/posevo.h: "every
point is checked against its curve equation (and for canonical coordinates) on the device"; oracle/g1.py from_bytes96 and
oracle/g2.py from_bytes192 for which bits belong to which element).

  96 bytes  x | y                          G1, y^2 = x^3 + 4
  192 bytes x.c1 | x.c0 | y.c1 | y.c0      G2, y^2 = x^3 + 4 (1 + u)

each element 48 bytes big-endian.  The three top bits of byte 0 are flags; every other element is a plain 384-bit integer.

  bit 6 of byte 0 set            infinity, whatever else the encoding holds
  otherwise bit 7 of byte 0 set  bad (the compressed form is refused here)
  bit 5 of byte 0                not part of the leading coordinate: ignored
  any coordinate >= p            bad (a non-leading element with one of its top three bits set is >= 2^381 > p)
  off the curve                  bad

classify96 / classify192 -> INFINITY, BAD, or the affine point in the oracle's form ((x, y); ((x0, x1), (y0, y1))).
"""
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
INFINITY, BAD = "infinity", "bad"
LEADING_BITS = 381                       # the leading element: 384 bits less the three flags
LEADING_MASK = (1 << LEADING_BITS) - 1


def _elements(b):
    v = [int.from_bytes(b[i:i + 48], "big") for i in range(0, len(b), 48)]
    v[0] &= LEADING_MASK
    return v


def _flags(b):
    """INFINITY, BAD or None from byte 0 alone."""
    if b[0] & 0x40:
        return INFINITY
    if b[0] & 0x80:
        return BAD
    return None


def classify96(b):
    assert len(b) == 96
    f = _flags(b)
    if f is not None:
        return f
    x, y = _elements(b)
    if x >= P or y >= P:
        return BAD
    if (y * y - (x * x * x + 4)) % P:
        return BAD
    return (x, y)


def _f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def classify192(b):
    assert len(b) == 192
    f = _flags(b)
    if f is not None:
        return f
    x1, x0, y1, y0 = _elements(b)
    if max(x1, x0, y1, y0) >= P:
        return BAD
    x, y = (x0, x1), (y0, y1)
    x3 = _f2_mul(_f2_mul(x, x), x)
    y2 = _f2_mul(y, y)
    if (y2[0] - x3[0] - 4) % P or (y2[1] - x3[1] - 4) % P:
        return BAD
    return (x, y)


def classify(b):
    return classify96(b) if len(b) == 96 else classify192(b)
