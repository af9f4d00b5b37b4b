"""A model of the aggregate pubkeys by complement: which groups go that way, and what comes out.

Keys are s_i * G with known scalars, so a sum of keys is (sum of scalars mod r) * G: the closed form every expectation of
tests/test_gpu_committee_sums.py comes from.  The model adds the points themselves through oracle/g1.py and shows the two
routes -- the attesting members summed directly, the committee's sum minus the absentees -- to be the same point in every
case of the group law."""
from oracle import g1


def by_complement(n_members, popcount, gated=True, whole_committee=True, sums_valid=True, knob=True):
    """The rule k_bits_union applies once per group: all four conditions, else the group is summed directly."""
    return bool(gated and whole_committee and sums_valid and knob and 2 * popcount > n_members)


def scalar_sum(scalars, bits, want=True):
    """Sum of the scalars whose bit equals `want`, mod r."""
    return sum(int(s) for s, b in zip(scalars, bits) if bool(b) == want) % g1.R_ORDER


def expected96(scalars, bits):
    """The 96-byte aggregate pubkey of the members whose bit is set (the closed form); infinity: 0x40 and 95 zero bytes."""
    return g1.to_bytes96(g1.mul(scalar_sum(scalars, bits), g1.G))


def direct_point(scalars, bits):
    """The attesting members' keys added one by one."""
    return g1.sum_points(g1.mul(int(s) % g1.R_ORDER, g1.G) for s, b in zip(scalars, bits) if b)


def complement_point(scalars, bits):
    """S_c + (-N): the whole committee's keys added one by one, minus the absentees' added one by one."""
    s_c = g1.sum_points(g1.mul(int(s) % g1.R_ORDER, g1.G) for s in scalars)
    n = g1.sum_points(g1.mul(int(s) % g1.R_ORDER, g1.G) for s, b in zip(scalars, bits) if not b)
    return g1.add(s_c, g1.neg(n))


# ---- the cases of the group law inside k_g1_finish's subtract-and-add, as (scalars, bits) of one committee
P_, Q_, C_ = 0x1234567, 0x89ABCDE, 0x5555
GROUP_LAW = {
    # {P, -P, Q} with P and -P attesting: S_c = Q, N = Q, S_c - N = infinity
    "cancels": ([P_, g1.R_ORDER - P_, Q_], [1, 1, 0]),
    # a + b + 2c = 0 (mod r), only c absent: S_c = -c G, -N = -c G: the add is a doubling
    "doubling": ([P_, (-P_ - 2 * C_) % g1.R_ORDER, C_], [1, 1, 0]),
    # everyone attests: N at infinity, the output is S_c itself
    "all": ([3, 5, 7, 11, 13], [1, 1, 1, 1, 1]),
    # adjacent scalars, the first three absent in one lane: 1G + 2G = 3G meets 3G (the accumulation's same-x path)
    "same_x": ([1, 2, 3, 1000, 2000, 3000, 4000, 5000], [0, 0, 0, 1, 1, 1, 1, 1]),
}
