"""CPU: the case table of tests/wire_cases.py is complete, every crafted encoding has the property its row claims, and
tests/wire_model.py classifies it as the oracle's decoders (from_bytes96 / from_bytes192) plus "< p" and the curve equation do.
tests/test_gpu_wire_points.py feeds the same table to every device decoder."""
import pytest

from oracle import g1, g2
from oracle.g1 import P, R_ORDER
from tests import wire_cases as wc
from tests import wire_model as wm

ORACLE = {"g1": (g1, g1.from_bytes96, g1.G), "g2": (g2, g2.from_bytes192, g2.G2)}
ALL = wc.cases("g1") + wc.cases("g2")


def _flat(group, pt):
    """The elements in wire order."""
    if group == "g1":
        return [pt[0], pt[1]]
    (x0, x1), (y0, y1) = pt
    return [x1, x0, y1, y0]


def _unflat(group, v):
    return (v[0], v[1]) if group == "g1" else ((v[1], v[0]), (v[3], v[2]))


def _oracle_class(group, enc):
    mod, from_bytes, _ = ORACLE[group]
    pt = from_bytes(enc)
    if pt is None:
        return wm.INFINITY
    if enc[0] & 0x80 or max(_flat(group, pt)) >= P or not mod.is_on_curve(pt):
        return wm.BAD
    return pt


def _elements_ignoring_infinity(group, enc):
    """What the coordinates would be were bit 6 clear (the oracle's decoder with that bit taken out)."""
    return _flat(group, ORACLE[group][1](bytes([enc[0] & 0xBF]) + enc[1:]))


def test_wire_model_knows_the_field():
    assert wm.P == P and P.bit_length() == 381 and wm.LEADING_BITS == 381
    assert (1 << 384) // P == 9 and (1 << 381) // P == 1


@pytest.mark.parametrize("group", ("g1", "g2"))
def test_the_base_point_leaves_room_for_x_plus_p(group):
    mod, _, gen = ORACLE[group]
    pt = wc.base_point(group)
    assert pt == mod.mul(wc.BASE_K[group], gen)
    assert mod.is_on_curve(pt) and mod.mul(R_ORDER, pt) is None
    room = (1 << 381) - P
    assert _flat(group, pt)[0] < room
    # the multiples named when the table was planned have the property too; most have not (about 23 % of abscissae)
    for k in {"g1": (2, 11, 12, 13), "g2": (5, 6, 11)}[group]:
        assert _flat(group, mod.mul(k, gen))[0] < room, k
    assert _flat(group, gen)[0] >= room                     # the generator itself has no second spelling of x


@pytest.mark.parametrize("group", ("g1", "g2"))
def test_no_cell_of_the_table_is_empty(group):
    table = wc.cases(group)
    assert len({c.name for c in table}) == len(table)
    for element, position in enumerate(wc.POSITIONS[group]):
        for edge in wc.POSITION_EDGES:
            cell = [c for c in table if c.position == position and c.edge == edge]
            assert len(cell) == 1 and cell[0].element == element, (position, edge)
    for edge in wc.POINT_EDGES:
        assert len([c for c in table if c.position is None and c.edge == edge]) == 1, edge
    assert len(table) == len(wc.POSITIONS[group]) * len(wc.POSITION_EDGES) + len(wc.POINT_EDGES)
    assert {c.expect for c in table} == {wc.SAME, wm.INFINITY, wm.BAD}
    # v + 9 p, the most that 384 bits hold, is reached by an element of each group
    base = _flat(group, wc.base_point(group))
    top = [c for c in table if c.edge == "plus_kp_max"]
    assert 9 * P in [int.from_bytes(c.enc[48 * c.element:48 * c.element + 48], "big") - base[c.element] for c in top]


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_the_crafted_bytes_have_the_claimed_property(c):
    mod = ORACLE[c.group][0]
    base = _flat(c.group, wc.base_point(c.group))
    assert len(c.enc) == 48 * len(base)
    got = _elements_ignoring_infinity(c.group, c.enc)
    assert c.same_residue == ([v % P for v in got] == base)
    assert c.on_curve == mod.is_on_curve(_unflat(c.group, [v % P for v in got]))
    if c.position is None:
        return
    e, v = c.element, base[c.element]
    raw = int.from_bytes(c.enc[48 * e:48 * e + 48], "big")
    others = [i for i in range(len(base)) if i != e]
    assert [got[i] for i in others] == [base[i] for i in others]            # one element crafted, the rest canonical
    if c.edge in ("plus_p", "plus_kp_max"):
        k, rest = divmod(raw - v, P)
        assert rest == 0 and k >= 1 and raw < 1 << wc.width(e)              # fits the element: no flag bit on the leader
        if c.edge == "plus_p":
            assert k == 1
        else:
            assert raw + P >= 1 << wc.width(e) and k in ((1,) if e == 0 else (8, 9))  # 9 for v < 2^384 - 9 p = 0.84 p
    elif c.edge in ("bit7", "bit6", "bit5"):
        bit = {"bit7": 0x80, "bit6": 0x40, "bit5": 0x20}[c.edge]
        assert raw == v | bit << 376 and raw != v
        assert got[e] == (v if e == 0 else raw)                            # the leader's flags are no part of x
        assert e == 0 or raw >= P
    elif c.edge == "eq_p":
        assert raw == P
    elif c.edge == "eq_p_minus_1":
        assert raw == P - 1
    else:
        assert raw == (v + {"plus_1": 1, "minus_1": -1}[c.edge]) % P and raw < P


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_the_model_agrees_with_the_oracle_decoders(c):
    want = _oracle_class(c.group, c.enc)
    assert wm.classify(c.enc) == want
    assert c.expect == (wc.SAME if want == wc.base_point(c.group) else want)
    if c.expect == wm.BAD and c.on_curve:
        # only "< p" or the compression flag stands between this encoding and a second spelling of a curve point
        assert c.enc[0] & 0x80 or max(_elements_ignoring_infinity(c.group, c.enc)) >= P


def test_the_point_cases_spell_what_they_say():
    for group, n in (("g1", 96), ("g2", 192)):
        first = {c.edge: c.enc[0] for c in wc.cases(group) if c.position is None}
        assert (first["inf_canonical"], first["inf_c0"], first["inf_60"], first["inf_40_nonzero"]) == (0x40, 0xC0, 0x60, 0x40)
        for edge in ("inf_canonical", "inf_c0", "inf_60"):
            assert not any(wc.case("%s:point:%s" % (group, edge)).enc[1:])
        assert all(b == 0xFF for b in wc.case("%s:point:inf_40_nonzero" % group).enc[1:])
        assert wc.case("%s:point:canonical" % group).enc == wc.canonical(group)
        assert int.from_bytes(wc.case("%s:point:zero_on_curve" % group).enc[:48], "big") == P
