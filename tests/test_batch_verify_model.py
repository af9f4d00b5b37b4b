"""CPU: tests/batch_verify_model.py, the specification of pe_batch_verify, against the truth by construction -- pk = a G1,
H = b G2, sig = a b G2 is valid, sig = (a b + 1) G2 is not -- on a handful of groups: all valid, one invalid, settled groups of
every kind, the stats tuple, and the forgery that known scalars allow.  The model's two routes (pairings; exponents of
e(G1, G2)) are held to each other on every case."""
import random

import pytest

from oracle import g1, g2
from oracle.g1 import P, R_ORDER
from tests import batch_verify_model as bm

C = 3       # small chunks: two or three of them on a handful of groups


def make(n, seed, invalid=()):
    """n groups by construction; -> (groups, dlogs, truth)."""
    rng = random.Random(seed)
    groups, dlogs = [], []
    for i in range(n):
        a, b = rng.randrange(1, R_ORDER), rng.randrange(1, R_ORDER)
        s = (a * b + (1 if i in invalid else 0)) % R_ORDER
        groups.append((g1.mul(a, g1.G), g2.mul(b, g2.G2), g2.mul(s, g2.G2)))
        dlogs.append((a, b, s))
    return groups, dlogs, [0 if i in invalid else 1 for i in range(n)]


def scalars(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 64) for _ in range(n)]


def outside_g2(seed):
    """A point of the twist outside the r-torsion, as tests/test_oracle_g2_psi.py builds them."""
    rng = random.Random(seed)
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = g2.f2_sqrt(g2.f2_add(g2.f2_mul(g2.f2_sqr(x), x), (4, 4)))
        if y is not None and g2.mul(R_ORDER, (x, y)) is not None:
            return (x, y)


def both_routes(groups, r, dlogs, c=C):
    v1, s1, gt = bm.batch_verify(groups, r, c=c)
    v2, s2, none = bm.batch_verify(groups, r, c=c, dlogs=dlogs)
    assert (v1, s1) == (v2, s2) and none is None and len(gt) == 576
    return v1, s1, gt


ONE = (1).to_bytes(48, "big") + bytes(528)


def test_all_valid():
    groups, dlogs, truth = make(7, 1)
    v, stats, gt = both_routes(groups, scalars(7, 2), dlogs)
    assert v == truth == [1] * 7
    assert stats == (7, 3, 1, 1, 0, 0, C, bm.FAN)      # one top-level exponentiation, no fallback
    assert gt == ONE


@pytest.mark.parametrize("where", (0, 3, 6))
def test_one_invalid(where):
    groups, dlogs, truth = make(7, 3, invalid=(where,))
    v, stats, gt = both_routes(groups, scalars(7, 4), dlogs)
    assert v == truth
    in_chunk = len(range(where // C * C, min(7, where // C * C + C)))
    assert stats == (7, 3, 1, 1, 3, in_chunk, C, bm.FAN)
    assert gt != ONE


def test_settled_groups_of_every_kind():
    groups, dlogs, truth = make(8, 5)
    pk, msg, sig = groups[1]
    groups[1] = ((pk[0], (pk[1] + 1) % P), msg, sig)                               # key off the curve
    groups[2] = (groups[2][0], (msg[0], ((msg[1][0] + 1) % P, msg[1][1])), groups[2][2])   # message point off the curve
    groups[3] = (groups[3][0], groups[3][1], (sig[0], ((sig[1][0] + 1) % P, sig[1][1])))   # signature off the curve
    groups[4] = (groups[4][0], groups[4][1], None)                                 # identity signature
    groups[5] = (None, groups[5][1], groups[5][2])                                 # identity key (an empty index group)
    groups[6] = (groups[6][0], groups[6][1], outside_g2(6))                        # on the curve, outside G2
    for i in range(1, 7):
        dlogs[i] = None
    truth[1:7] = [2, 2, 2, 0, 0, 0]
    v, stats, gt = both_routes(groups, scalars(8, 6), dlogs)
    assert v == truth
    assert stats == (2, 1, 0, 1, 0, 0, C, bm.FAN)      # the neighbours: one chunk, the honest case
    assert gt == ONE
    # a bad point outranks an identity, as in pe_fast_aggregate_verify
    assert bm.settle((None, groups[2][1], groups[0][2])) == 2
    # nothing live at all
    v, stats, gt = bm.batch_verify(groups[1:7], scalars(6, 7), c=C)
    assert v == truth[1:7] and stats == (0, 0, 0, 0, 0, 0, C, bm.FAN) and gt == ONE


def test_stats_of_the_product_tree():
    assert [bm.product_launches(n, 8) for n in (0, 1, 2, 8, 9, 64, 65)] == [0, 0, 1, 1, 2, 2, 3]
    groups, dlogs, _ = make(4, 8)
    r = scalars(4, 9)
    for c, fan, want in ((1, 2, (4, 4, 2)), (1, 4, (4, 4, 1)), (2, 8, (4, 2, 1)), (4, 8, (4, 1, 0)), (5, 8, (4, 1, 0))):
        v, stats, _ = bm.batch_verify(groups, r, c=c, fan=fan, dlogs=dlogs)
        assert v == [1] * 4 and stats == want + (1, 0, 0, c, fan)


@pytest.mark.parametrize("c", (1, 5))       # the two groups in two chunks, and in one
def test_the_forgery_with_known_scalars(c):
    """sig_1' = sig_1 + r_2 D, sig_2' = sig_2 - r_1 D: r_1 sig_1' + r_2 sig_2' = r_1 sig_1 + r_2 sig_2, so the batch says 1, 1
    with the scalars (r_1, r_2) the forger knew -- and 0, 0 with any other pair.  Why the scalars must be secret."""
    groups, dlogs, _ = make(2, 10)
    r1, r2 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F
    d = 0x1234567
    D = g2.mul(d, g2.G2)
    forged = [(groups[0][0], groups[0][1], g2.add(groups[0][2], g2.mul(r2, D))),
              (groups[1][0], groups[1][1], g2.add(groups[1][2], g2.neg(g2.mul(r1, D))))]
    fd = [(dlogs[0][0], dlogs[0][1], (dlogs[0][2] + r2 * d) % R_ORDER), (dlogs[1][0], dlogs[1][1], (dlogs[1][2] - r1 * d) % R_ORDER)]
    if c == 5:
        v, stats, gt = both_routes(forged, [r1, r2], fd, c=c)
        assert gt == ONE
    else:
        v, stats, _ = bm.batch_verify(forged, [r1, r2], c=c, dlogs=fd)
    assert v == [1, 1] and stats[3:6] == (1, 0, 0)     # the top-level product decides, and it is fooled
    for other in ([r1, r2 + 1], [r1 ^ 1, r2], [r2, r1]):
        v, stats, _ = bm.batch_verify(forged, other, c=c, dlogs=fd)
        assert v == [0, 0] and stats[5] == 2
    v, _, _ = bm.batch_verify(forged, [r1 + 2, r2], c=c)          # once through the pairings
    assert v == [0, 0]
