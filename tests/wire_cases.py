"""The case table of the uncompressed-point decoders: every coordinate position of a G1 and a G2 point at every edge of the wire
rules (tests/wire_model.py), as crafted bytes with the class they must decode to.

The base points are 11 G1 and 5 G2: subgroup points whose LEADING abscissa (x; x.c1) is below 2^381 - p, so that x + p still fits
the 381 bits of the leading element and is a second spelling of the same residue.  Every other element is read as 384 bits:
v + k p fits up to k = 9 (2^384 / p = 9.8).

Per position (G1: x, y; G2: x.c1, x.c0, y.c1, y.c0 -- wire order, element 0 leads):
  plus_p, plus_kp_max   v + p and v + k p for the largest k that fits the element   same residue, not canonical        bad
  bit7, bit6, bit5      one of the top three bits of the element's own first byte
                          leading element: compressed flag | infinity flag | ignored                bad | infinity | same
                          any other element: the value is >= 2^381 > p                                                 bad
  eq_p, eq_p_minus_1    the element replaced by p (not canonical) and by p - 1 (canonical, off the curve)              bad
  plus_1, minus_1       v +- 1 mod p (canonical, off the curve)                                                        bad
Per point:
  canonical             the oracle's own bytes                                                                         same
  inf_canonical, inf_c0, inf_60, inf_40_nonzero
                        0x40 00.., 0xC0 00.., 0x60 00.., 0x40 then 0xFF bytes                                          infinity
  zero_on_curve         the leading element is p, spelt for 0, in a point that is on the curve mod p (G1: (0, 2); G2: x = t + 0 u
                        for the smallest t with a root): ONLY the canonical test refuses it                            bad

`expect` is SAME (decodes to the base point), INFINITY or BAD; `same_residue` says the elements reduce mod p to the base point's,
`on_curve` that the reduced coordinates satisfy the curve equation (tests/test_wire_model.py checks both claims and the class)."""
from collections import namedtuple

from oracle import g1, g2
from tests.wire_model import BAD, INFINITY, LEADING_BITS, P

SAME = "same"
BASE_K = {"g1": 11, "g2": 5}
POSITIONS = {"g1": ("x", "y"), "g2": ("x.c1", "x.c0", "y.c1", "y.c0")}
POSITION_EDGES = ("plus_p", "plus_kp_max", "bit7", "bit6", "bit5", "eq_p", "eq_p_minus_1", "plus_1", "minus_1")
POINT_EDGES = ("canonical", "inf_canonical", "inf_c0", "inf_60", "inf_40_nonzero", "zero_on_curve")

# group "g1" | "g2"; position: a name of POSITIONS or None for a per-point case; element: its index in wire order or None
Case = namedtuple("Case", "name group position element edge enc expect same_residue on_curve")


def base_point(group):
    return g1.mul(BASE_K["g1"], g1.G) if group == "g1" else g2.mul(BASE_K["g2"], g2.G2)


def canonical(group):
    pt = base_point(group)
    return g1.to_bytes96(pt) if group == "g1" else g2.to_bytes192(pt)


def width(element):
    return LEADING_BITS if element == 0 else 384


def _with(enc, element, value=None, or_byte=0):
    out = bytearray(enc)
    if value is not None:
        assert value < 1 << width(element)
        out[48 * element:48 * element + 48] = value.to_bytes(48, "big")
    out[48 * element] |= or_byte
    return bytes(out)


def _zero_on_curve(group):
    if group == "g1":
        return P.to_bytes(48, "big") + (2).to_bytes(48, "big")
    t = 0
    while g2.f2_sqrt(((t * t * t + 4) % P, 4)) is None:     # x = t + 0 u
        t += 1
    y = g2.f2_sqrt(((t * t * t + 4) % P, 4))
    return P.to_bytes(48, "big") + t.to_bytes(48, "big") + y[1].to_bytes(48, "big") + y[0].to_bytes(48, "big")


def _build(group):
    enc = canonical(group)
    out = []

    def add(position, element, edge, data, expect, same_residue, on_curve):
        name = "%s:%s:%s" % (group, position or "point", edge)
        out.append(Case(name, group, position, element, edge, data, expect, same_residue, on_curve))

    for element, position in enumerate(POSITIONS[group]):
        v = int.from_bytes(enc[48 * element:48 * element + 48], "big")
        lead = element == 0
        k_max = ((1 << width(element)) - 1 - v) // P
        assert k_max >= 1, "the base point's leading abscissa leaves no room for + p"
        add(position, element, "plus_p", _with(enc, element, v + P), BAD, True, True)
        add(position, element, "plus_kp_max", _with(enc, element, v + k_max * P), BAD, True, True)
        add(position, element, "bit7", _with(enc, element, or_byte=0x80), BAD, lead, lead)
        add(position, element, "bit6", _with(enc, element, or_byte=0x40), INFINITY if lead else BAD, lead, lead)
        add(position, element, "bit5", _with(enc, element, or_byte=0x20), SAME if lead else BAD, lead, lead)
        add(position, element, "eq_p", _with(enc, element, P), BAD, False, False)
        add(position, element, "eq_p_minus_1", _with(enc, element, P - 1), BAD, False, False)
        add(position, element, "plus_1", _with(enc, element, (v + 1) % P), BAD, False, False)
        add(position, element, "minus_1", _with(enc, element, (v - 1) % P), BAD, False, False)
    n = len(enc)
    add(None, None, "canonical", enc, SAME, True, True)
    add(None, None, "inf_canonical", bytes([0x40]) + bytes(n - 1), INFINITY, False, False)
    add(None, None, "inf_c0", bytes([0xC0]) + bytes(n - 1), INFINITY, False, False)
    add(None, None, "inf_60", bytes([0x60]) + bytes(n - 1), INFINITY, False, False)
    add(None, None, "inf_40_nonzero", bytes([0x40]) + b"\xff" * (n - 1), INFINITY, False, False)
    add(None, None, "zero_on_curve", _zero_on_curve(group), BAD, False, True)
    return out


_TABLE = {}


def cases(group):
    """The cases of "g1" or "g2", built once."""
    if group not in _TABLE:
        _TABLE[group] = _build(group)
    return _TABLE[group]


def case(name):
    return next(c for c in cases(name.split(":")[0]) if c.name == name)
