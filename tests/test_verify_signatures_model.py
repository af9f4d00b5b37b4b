"""CPU: tests/verify_signatures_model.py -- its exponent route against the pairing of tests/pairing_model.py on tiny groups, and
the case the feature exists for: a cancelling pair of forged signatures passes with equal weights and fails with unequal ones."""
from oracle import g1, g2
from oracle.g1 import R_ORDER
from tests import pairing_model as pm
from tests import verify_signatures_model as vm

SK = (0x1F2E3D4C5B6A7988, 0x0123456789ABCDEF, 0x7766554433221100, 0x5A5A5A5A)
H = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F)


def _members(sks, h, spoil=()):
    return [(sk, (sk * h + (1 if i in spoil else 0)) % R_ORDER, 0) for i, sk in enumerate(sks)]


def test_exponent_route_is_the_pairing():
    """Three groups of two members (valid, one invalid member, valid with edge weights): the verdict in the exponent equals
    e(sum r pk, H) e(-g1, sum r sig) == 1 computed by the pairing model on the model's own sums."""
    members = _members(SK[:2], H[0]) + _members(SK[1:3], H[1], spoil=(1,)) + _members(SK[2:4], H[0])
    offsets, msgs = [0, 2, 4, 6], [H[0], H[1], H[0]]
    r = [3, 0xAAAAAAAAAAAAAAAA, 5, 7, 1, (1 << 64) - 1]
    verdict, status, group, sums, stats = vm.verify(members, offsets, msgs, r)
    assert verdict == [1, 1, 1, 0, 1, 1] and group == [1, 0, 1] and status == [0] * 6
    assert stats == (0, 1, 2, 2, vm.STRIPE)
    one = pm.gt_bytes(pm.F12_ONE)
    neg_g1 = g1.neg(g1.G)
    for g in range(3):
        pk, sig = g1.mul(sums[g][0], g1.G), g2.mul(sums[g][1], g2.G2)
        value = pm.gt_bytes(pm.pairing_product([(pk, g2.mul(msgs[g], g2.G2)), (neg_g1, sig)]))
        assert (value == one) == (group[g] == 1), g


def test_the_cancelling_pair():
    """sig_a + D and sig_b - D sum to the honest aggregate: equal weights let both pass, unequal ones catch both."""
    d = 0x1234567
    honest = _members(SK[:2], H[0])
    forged = [(honest[0][0], (honest[0][1] + d) % R_ORDER, 0), (honest[1][0], (honest[1][1] - d) % R_ORDER, 0)]
    assert sum(m[1] for m in forged) % R_ORDER == sum(m[1] for m in honest) % R_ORDER     # the plain aggregate is the honest one
    verdict, _, group, _, stats = vm.verify(forged, [0, 2], [H[0]], [77, 77])
    assert verdict == [1, 1] and group == [1] and stats[:4] == (0, 0, 0, 1)
    verdict, _, group, _, stats = vm.verify(forged, [0, 2], [H[0]], [77, 78])
    assert verdict == [0, 0] and group == [0] and stats[:4] == (0, 1, 2, 2)


def test_settled_members_and_group_rules():
    members = _members(SK[:3], H[0])
    members[1] = (members[1][0], None, 3)                       # outside G2: in neither sum, the others stay valid
    verdict, status, group, sums, stats = vm.verify(members + _members(SK[:1], H[1]), [0, 3, 3, 4], [H[0], H[1], 0], [1, 2, 3, 4])
    assert verdict == [1, 0, 1, 0] and status == [0, 3, 0, 0]
    assert group == [0, 1, 0]                                   # a settled member; an empty group; an identity message point
    assert stats[:4] == (1, 0, 0, 1)
    assert sums[0] == ((SK[0] + 3 * SK[2]) % R_ORDER, (SK[0] + 3 * SK[2]) * H[0] % R_ORDER) and sums[1] == (0, 0)
    pk, sig = vm.sum_bytes(sums)
    assert pk[96] == 0x40 and sig[192] == 0x40 and len(pk) == 3 * 96 and len(sig) == 3 * 192
    assert vm.aggregate_bytes(members, [0, 3], verdict) == g2.compress(g2.mul((SK[0] + SK[2]) * H[0] % R_ORDER, g2.G2))


def test_cost_figures():
    assert vm.wave_max_adds(1, 1) == 0.5 and vm.wave_max_adds(16, 1) == 8
    assert 11.5 < vm.wave_max_adds(16, 32) < 12.6 < vm.wave_max_adds(16, 64) + 0.5 < 13.5
    (g2_exec, g2_useful), (g1_exec, g1_useful) = vm.fp_products_per_point(16)
    assert g2_useful == 4 * 15 + 32 * 18 and g1_useful == 4 * 9 + 32 * 10
    assert g2_useful < g2_exec < 64 * (15 + 18) and g1_useful < g1_exec < 64 * (9 + 10)       # under the per-point scale
