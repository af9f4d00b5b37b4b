"""The complement rule and S_c - N on the CPU (tests/committee_sums_model.py): what tests/test_gpu_committee_sums.py expects."""
import numpy as np
import pytest

from oracle import g1
from tests import committee_sums_model as M

INF96 = bytes([0x40]) + bytes(95)


@pytest.mark.parametrize("n", [1, 3, 8, 9, 1025])
def test_threshold_is_a_strict_majority(n):
    for pop in range(0, n + 1):
        assert M.by_complement(n, pop) == (2 * pop > n)
    assert M.by_complement(8, 4) is False and M.by_complement(8, 5) is True
    assert M.by_complement(9, 4) is False and M.by_complement(9, 5) is True


def test_every_condition_is_needed():
    assert M.by_complement(8, 8)
    for off in ("gated", "whole_committee", "sums_valid", "knob"):
        assert not M.by_complement(8, 8, **{off: False})


@pytest.mark.parametrize("name", sorted(M.GROUP_LAW))
def test_group_law_cases_agree_with_the_direct_sum(name):
    scalars, bits = M.GROUP_LAW[name]
    assert M.by_complement(len(scalars), sum(bits))
    direct, cmpl = M.direct_point(scalars, bits), M.complement_point(scalars, bits)
    assert direct == cmpl
    assert g1.to_bytes96(cmpl) == M.expected96(scalars, bits)


def test_the_named_cases_are_what_they_claim():
    s, b = M.GROUP_LAW["cancels"]
    assert M.expected96(s, b) == INF96 and M.complement_point(s, b) is g1.INF
    s, b = M.GROUP_LAW["doubling"]
    s_c = g1.mul(sum(s) % g1.R_ORDER, g1.G)
    minus_n = g1.neg(g1.mul(M.scalar_sum(s, b, want=False), g1.G))
    assert s_c == minus_n and g1.add(s_c, minus_n) == g1.double(s_c)
    s, b = M.GROUP_LAW["same_x"]
    assert g1.add(g1.mul(s[0], g1.G), g1.mul(s[1], g1.G)) == g1.mul(s[2], g1.G)


def test_random_committees_both_routes():
    rng = np.random.Generator(np.random.PCG64(12))
    for n in (1, 2, 5, 16):
        scalars = [int(x) for x in rng.integers(1, 1 << 62, size=n)]
        for density in (0.0, 0.5, 1.0):
            bits = [int(x) for x in (rng.random(n) < density)]
            assert M.direct_point(scalars, bits) == M.complement_point(scalars, bits)
            assert g1.to_bytes96(M.direct_point(scalars, bits)) == M.expected96(scalars, bits)
