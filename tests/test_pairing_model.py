"""CPU: tests/pairing_model.py -- the model that runs the kernels' op tables -- held to the properties that pin a pairing up to
the fixed power c = 3: bilinearity, additivity in each argument, non-degeneracy, infinity.  No second pairing implementation is
trusted.  (About 0.06 s per model pairing; the whole file runs in about 2 s.)"""
import pytest

from tests import pairing_model as pm
from oracle import g1, g2
from oracle.g1 import P, R_ORDER


@pytest.fixture(scope="module")
def e11():
    return pm.pairing(g1.G, g2.G2)


def test_tower_operations(e11):
    f = pm.miller_loop([(g1.mul(9, g1.G), g2.mul(4, g2.G2))])          # a generic Fp12 value
    h = pm.miller_loop([(g1.G, g2.G2)])
    assert pm.f12_mul(f, pm.F12_ONE) == f and pm.f12_mul(f, h) == pm.f12_mul(h, f)
    assert pm.f12_mul(pm.f12_mul(f, h), f) == pm.f12_mul(f, pm.f12_mul(h, f))
    for n in (1, 2, 3):
        assert pm.f12_frob(f, n) == pm.f12_pow(f, P ** n)
    assert pm.f12_conj(f) == pm.f12_pow(f, P ** 6)
    line = ((3, 5), (7, 11), (13, 17))
    dense = [line[0], (0, 0), line[1], line[2], (0, 0), (0, 0)]
    assert pm.f12_mul_line(f, line) == pm.f12_mul(f, dense)
    cyc = pm.f12_pow(f, (P ** 6 - 1) * (P ** 2 + 1))
    assert pm.f12_cyclo_sqr(cyc) == pm.f12_sqr(cyc)
    assert pm.f12_cyclo_sqr(f) != pm.f12_sqr(f)                        # only valid in the cyclotomic subgroup


def test_final_exponentiation_is_the_stated_power():
    f = pm.miller_loop([(g1.mul(6, g1.G), g2.mul(10, g2.G2))])
    assert (P ** 12 - 1) % R_ORDER == 0 and pm.FINAL_POWER_C % R_ORDER != 0
    assert pm.final_exp(f) == pm.f12_pow(f, (P ** 12 - 1) // R_ORDER * pm.FINAL_POWER_C)


def test_non_degenerate(e11):
    assert e11 != pm.F12_ONE
    assert pm.f12_pow(e11, R_ORDER) == pm.F12_ONE


@pytest.mark.parametrize("a,b", [(2, 3), (R_ORDER - 1, 1), (R_ORDER - 1, R_ORDER - 1),
                                 (0x5A3C19E0F1D2B4A6978877665544332211FFEEDDCCBBAA99, 0x1F2E3D4C5B6A79880123456789ABCDEF)])
def test_bilinear(e11, a, b):
    assert pm.pairing(g1.mul(a, g1.G), g2.mul(b, g2.G2)) == pm.f12_pow(e11, a * b % R_ORDER)


def test_additive_in_each_argument():
    p1, p2 = g1.mul(11, g1.G), g1.mul(R_ORDER - 5, g1.G)
    q1, q2 = g2.mul(7, g2.G2), g2.mul(0x123456789ABCDEF, g2.G2)
    assert pm.pairing(g1.add(p1, p2), q1) == pm.f12_mul(pm.pairing(p1, q1), pm.pairing(p2, q1))
    assert pm.pairing(p1, g2.add(q1, q2)) == pm.f12_mul(pm.pairing(p1, q1), pm.pairing(p1, q2))
    # the multi-pairing shares one accumulator: the product of the single pairings
    assert pm.pairing_product([(p1, q1), (p2, q2)]) == pm.f12_mul(pm.pairing(p1, q1), pm.pairing(p2, q2))


def test_infinity_gives_one():
    assert pm.pairing(None, g2.G2) == pm.F12_ONE
    assert pm.pairing(g1.G, None) == pm.F12_ONE
    assert pm.pairing_product([]) == pm.F12_ONE
    assert pm.pairing_product([(g1.G, g2.G2), (None, g2.G2)]) == pm.pairing(g1.G, g2.G2)


def test_verdict_by_construction():
    """What tests/test_gpu_bls_verify.py relies on: prod e(a_i G1, b_i G2) == 1 iff sum a_i b_i == 0 (mod r)."""
    a, b = [3, R_ORDER - 1, 12345], [5, 7, 0]
    b[2] = -(a[0] * b[0] + a[1] * b[1]) * pow(a[2], -1, R_ORDER) % R_ORDER
    pairs = [(g1.mul(x, g1.G), g2.mul(y, g2.G2)) for x, y in zip(a, b)]
    assert pm.pairing_product(pairs) == pm.F12_ONE
    pairs[1] = (pairs[1][0], g2.mul(b[1] + 1, g2.G2))
    assert pm.pairing_product(pairs) != pm.F12_ONE
