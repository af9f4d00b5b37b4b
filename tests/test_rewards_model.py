"""CPU: tests/rewards_model.py -- the specification pe_rewards_and_penalties is held to -- against the cross-check vector
of the pull request that introduced it, tests/golden/rewards_vectors.json, the edges of its rule set, and its own numpy
form."""
import copy
import json

import numpy as np
import pytest

from tests import rewards_model as M

E = M.E32
P = M.ISSUE_PARAMS


def run(reg, current, finalized, p=P, which=M.DO_BOTH, **kw):
    reg = copy.deepcopy(reg)
    return reg, M.run(reg, current, finalized, p, which, **kw)


def test_the_cross_check_vector():
    reg = M.issue_registry()
    total, unslashed, eligible = M.sums(reg, 10, P)
    assert (total, unslashed, len(eligible)) == (207 * 10**9, [96 * 10**9, 80 * 10**9, 48 * 10**9], 6)
    assert M.base_reward_per_increment(total, P) == 140667
    after, st = run(reg, 10, 8)
    assert after.balances == [32001391724, 32001163390, 30998626716, 0, 31997186660, 30000000000, 467530, 32000000000]
    assert after.scores == [0, 0, 8, 88, 0, 50, 0, 9] and st.in_leak == 0
    after, st = run(reg, 10, 3)
    assert after.balances == [32000000005, 32000000000, 30998167515, 0, 31997184912, 30000000000, 0, 32000000000]
    assert after.scores == [0, 0, 24, 104, 11, 50, 2, 9] and st.in_leak == 1
    assert M.base_reward_per_increment(2**20 * E, P) == 349


def test_validator_5_is_eligible_at_epoch_9_and_not_at_10():
    """Slashed, inactive, withdrawable at 10: previous_epoch + 1 < 10 holds at current_epoch 9 only."""
    reg = M.issue_registry()
    after, st = run(reg, 10, 8)
    assert st.n_eligible == 6 and (after.balances[5], after.scores[5]) == (reg.balances[5], reg.scores[5])
    after, st = run(reg, 9, 7)
    assert st.n_eligible == 7 and st.n_slashed_eligible == 1
    assert after.balances[5] < reg.balances[5] and after.scores[5] == 50 + 4 - 16


def test_the_golden_file_is_the_model():
    cases = json.load(open(M.GOLDEN_PATH))
    assert cases == json.loads(json.dumps(M.golden_cases()))
    names = {c["name"] for c in cases}
    assert {"issue_no_leak", "issue_leak", "issue_genesis", "issue_epoch_9_validator_5_eligible"} <= names


def test_the_leak_starts_at_a_delay_of_5():
    assert not M.is_in_inactivity_leak(10, 5, P)   # delay 4
    assert M.is_in_inactivity_leak(10, 4, P)       # delay 5
    reg = M.issue_registry()
    assert run(reg, 10, 5)[1].rewards > 0 and run(reg, 10, 4)[1].rewards == 0
    with pytest.raises(OverflowError):
        M.is_in_inactivity_leak(10, 10, P)         # finalized after the previous epoch: the reference's uint64 underflows


def test_genesis_epoch_is_a_no_op():
    reg = M.issue_registry()
    after, st = run(reg, 0, 0)
    assert after == reg and st.abi() == [0] * 9


def test_epoch_1_clamps_the_previous_epoch_to_0():
    reg = M.issue_registry()
    assert M.get_previous_epoch(1) == 0 == M.get_previous_epoch(0)
    after, st = run(reg, 1, 0)
    assert st.in_leak == 0 and st.n_eligible == 7      # previous_epoch + 1 = 1 < 10: validator 5 counts
    assert after.balances[0] > reg.balances[0]


def test_an_empty_unslashed_set_counts_one_increment():
    reg = M.issue_registry()
    reg.participation = [x & ~4 for x in reg.participation]      # nobody was timely for the head
    _, unslashed, _ = M.sums(reg, 10, P)
    assert unslashed[2] == P.increment
    after, st = run(reg, 10, 8)
    assert st.unslashed_balance[2] == P.increment and after.balances[0] > reg.balances[0]


def test_pairs_are_applied_one_after_the_other_not_netted():
    """Validator 6 (balance 0, flags 6: misses the source, hits target and head): the source penalty meets an empty
    balance and is lost, the target and head rewards then stay.  Netted, the larger penalty would eat all of them."""
    reg = M.issue_registry()
    pairs = []
    after, st = run(reg, 10, 8, pairs_out=pairs)
    v = 6
    rewards, penalties = sum(pr[0][v] for pr in pairs), sum(pr[1][v] for pr in pairs)
    netted = max(0, reg.balances[v] + rewards - penalties)
    assert penalties > 0 and rewards > 0
    assert penalties > rewards and netted == 0
    assert after.balances[v] == 467530 == rewards != netted
    assert st.n_saturated == 2                                                  # validators 3 and 6


def test_bits_3_to_7_of_a_participation_byte_mean_nothing():
    reg = M.issue_registry()
    junk = copy.deepcopy(reg)
    junk.participation = [x | 0xF8 for x in reg.participation]
    for finalized in (8, 3):
        a, sa = run(reg, 10, finalized)
        b, sb = run(junk, 10, finalized)
        assert (a.balances, a.scores, sa) == (b.balances, b.scores, sb)


@pytest.mark.parametrize("which", [M.DO_INACTIVITY, M.DO_DELTAS, M.DO_BOTH])
@pytest.mark.parametrize("current,finalized", [(12, 10), (12, 2), (1, 0), (0, 0)])
@pytest.mark.parametrize("n,seed", [(1, 1), (7, 2), (64, 3), (500, 4), (2000, 5)])
def test_the_numpy_form_equals_the_list_form(n, seed, current, finalized, which):
    a = M.random_registry(n, seed, current)
    reg = M.registry_from_arrays(**a)
    st = M.run(reg, current, finalized, M.Params(), which)
    bal, sc, st_np = M.run_numpy(**a, current_epoch=current, finalized_epoch=finalized, which=which)
    assert [int(x) for x in bal] == reg.balances and [int(x) for x in sc] == reg.scores
    assert st_np == st


def test_the_random_mix_holds_every_class():
    a = M.random_registry(256, 9, 12)
    _, _, st = M.run_numpy(**a, current_epoch=12, finalized_epoch=10)
    assert st.n_saturated and st.n_slashed_eligible and st.n_flag_rewards and st.n_flag_penalties and st.n_inactivity_penalties
    assert len(set(a["sflags"].tolist())) == 8 and len(set((a["participation"] & 7).tolist())) == 8
    assert (a["participation"] & 0xF8).any()
    edge = M.get_previous_epoch(12) + 1
    assert {edge - 1, edge, edge + 1} <= set(a["withdrawable"].tolist())
