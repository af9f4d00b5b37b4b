"""The specification of process_inactivity_updates and process_rewards_and_penalties as the engine runs them
(pe_rewards_and_penalties): the Altair functions, restated here because the reference holds their fields
(state.balances, state.inactivity_scores, Validator.withdrawable_epoch: pe:112, pe:368-369, pe:45), their feeder
(process_attestation, pe:739-749) and the prose that balances "rise and fall with rewards and penalties", but not their
text -- the class DESIGN section 6 calls unpinned, next to get_base_reward, which they extend.

List-based pyspec style over Python integers (``run``), every uint64 overflow of the reference an OverflowError; a
vectorised numpy form for large registries (``run_numpy``), held equal to the list form by tests/test_rewards_model.py.
``python -m tests.rewards_model`` rewrites tests/golden/rewards_vectors.json from ``golden_cases``.
"""
import json
import os
from dataclasses import dataclass, field
from math import isqrt
from typing import List

import numpy as np

UINT64_MAX = 2**64 - 1
FAR_FUTURE_EPOCH = UINT64_MAX
GENESIS_EPOCH = 0
TIMELY_SOURCE_FLAG_INDEX, TIMELY_TARGET_FLAG_INDEX, TIMELY_HEAD_FLAG_INDEX = 0, 1, 2
PARTICIPATION_FLAG_WEIGHTS = [14, 26, 14]
WEIGHT_DENOMINATOR = 64
# the working-state view's flag byte (include/posevo.h)
VAL_ACTIVE, VAL_SLASHED, VAL_ACTIVE_PREV = 0x01, 0x02, 0x08
DO_INACTIVITY, DO_DELTAS = 1, 2  # PE_REWARDS_INACTIVITY, PE_REWARDS_DELTAS
DO_BOTH = DO_INACTIVITY | DO_DELTAS


@dataclass
class Params:
    increment: int = 10**9                       # EFFECTIVE_BALANCE_INCREMENT (pe_config)
    base_reward_factor: int = 64
    inactivity_score_bias: int = 4
    inactivity_score_recovery_rate: int = 16
    inactivity_penalty_quotient: int = 2**24     # Bellatrix; Altair: 3 * 2**24
    min_epochs_to_inactivity_penalty: int = 4


@dataclass
class Registry:
    """What the two functions read of a BeaconState, as the engine holds it."""
    effective_balance: List[int]
    slashed: List[int]
    active_prev: List[int]
    active_cur: List[int]
    participation: List[int]          # previous_epoch_participation bytes
    withdrawable_epoch: List[int]
    balances: List[int]
    scores: List[int]

    def sflags(self):
        return [(VAL_ACTIVE if c else 0) | (VAL_SLASHED if s else 0) | (VAL_ACTIVE_PREV if p else 0)
                for c, s, p in zip(self.active_cur, self.slashed, self.active_prev)]


@dataclass
class Stats:
    total_active_balance: int = 0
    unslashed_balance: List[int] = field(default_factory=lambda: [0, 0, 0])
    n_eligible: int = 0
    in_leak: int = 0
    rewards: int = 0
    penalties: int = 0
    n_saturated: int = 0
    # what the model knows beyond pe_rewards_stats: which classes of validator the inputs held
    n_slashed_eligible: int = 0       # eligible only through slashing
    n_flag_rewards: int = 0           # a flag reward > 0
    n_flag_penalties: int = 0         # a flag penalty > 0
    n_inactivity_penalties: int = 0   # an inactivity penalty > 0

    def abi(self):
        """The nine words of pe_rewards_stats, in order."""
        return [self.total_active_balance, *self.unslashed_balance, self.n_eligible, self.in_leak, self.rewards,
                self.penalties, self.n_saturated]


def u64(x: int, what: str) -> int:
    if not 0 <= x <= UINT64_MAX:
        raise OverflowError(what)
    return x


def get_previous_epoch(current_epoch: int) -> int:
    return max(current_epoch, GENESIS_EPOCH + 1) - 1


def is_in_inactivity_leak(current_epoch: int, finalized_epoch: int, p: Params) -> bool:
    return u64(get_previous_epoch(current_epoch) - finalized_epoch, "finality delay") > p.min_epochs_to_inactivity_penalty


def is_eligible(r: Registry, v: int, previous_epoch: int) -> bool:
    return bool(r.active_prev[v]) or (bool(r.slashed[v]) and previous_epoch + 1 < r.withdrawable_epoch[v])


def in_unslashed(r: Registry, v: int, flag_index: int) -> bool:
    """v in get_unslashed_participating_indices(state, flag_index, previous_epoch).  Bits 3-7 of the byte mean nothing."""
    return bool(r.active_prev[v]) and not r.slashed[v] and bool((r.participation[v] >> flag_index) & 1)


def get_total_balance(r: Registry, indices, p: Params) -> int:
    return max(p.increment, u64(sum(r.effective_balance[v] for v in indices), "total balance"))


def sums(r: Registry, current_epoch: int, p: Params):
    """-> (total_active_balance, [unslashed participating balance of flag 0, 1, 2], eligible indices)."""
    n = len(r.balances)
    previous_epoch = get_previous_epoch(current_epoch)
    total_active = get_total_balance(r, [v for v in range(n) if r.active_cur[v]], p)
    unslashed = [get_total_balance(r, [v for v in range(n) if in_unslashed(r, v, f)], p) for f in range(3)]
    return total_active, unslashed, [v for v in range(n) if is_eligible(r, v, previous_epoch)]


def base_reward_per_increment(total_active: int, p: Params) -> int:
    return u64(p.increment * p.base_reward_factor, "increment * base_reward_factor") // isqrt(total_active)


def check_call_bounds(r: Registry, total_active, unslashed, eligible, in_leak, p: Params, which: int) -> None:
    """The refusals pe_rewards_and_penalties makes before it writes anything (include/posevo.h): conservative bounds from
    the maxima over eligible validators -- they may refuse a call in which no single product would have overflowed."""
    per_increment = base_reward_per_increment(total_active, p)
    u64(total_active // p.increment * WEIGHT_DENOMINATOR, "active increments * WEIGHT_DENOMINATOR")
    max_eff = max((r.effective_balance[v] for v in eligible), default=0)
    max_score = max((r.scores[v] for v in eligible), default=0)
    if which & DO_DELTAS:
        largest_unslashed = 1 if in_leak else max(u // p.increment for u in unslashed)
        u64(max_eff // p.increment * per_increment * max(PARTICIPATION_FLAG_WEIGHTS) * largest_unslashed,
            "base_reward * weight * unslashed increments")
    score_bound = max_score + (p.inactivity_score_bias if which & DO_INACTIVITY else 0)
    u64(score_bound, "inactivity score + bias")
    if which & DO_DELTAS:
        u64(max_eff * score_bound, "effective_balance * inactivity score")


def run(r: Registry, current_epoch: int, finalized_epoch: int, p: Params = None, which: int = DO_BOTH, pairs_out: list = None) -> Stats:
    """process_inactivity_updates (which & DO_INACTIVITY), then process_rewards_and_penalties (which & DO_DELTAS), in
    place on r.scores / r.balances.  Raises OverflowError (and changes nothing) where the engine refuses the call.
    pairs_out: a list that receives the four (rewards, penalties) pairs as they were before any of them was applied."""
    p = p or Params()
    assert which in (DO_INACTIVITY, DO_DELTAS, DO_BOTH)
    inactivity_divisor = u64(p.inactivity_score_bias * p.inactivity_penalty_quotient, "bias * quotient")
    if p.increment == 0 or inactivity_divisor == 0:
        raise OverflowError("increment and bias * quotient must be positive")
    st = Stats()
    if current_epoch == GENESIS_EPOCH:
        return st
    n = len(r.balances)
    previous_epoch = get_previous_epoch(current_epoch)
    in_leak = is_in_inactivity_leak(current_epoch, finalized_epoch, p)
    total_active, unslashed, eligible = sums(r, current_epoch, p)
    check_call_bounds(r, total_active, unslashed, eligible, in_leak, p, which)
    st.total_active_balance, st.unslashed_balance, st.n_eligible, st.in_leak = total_active, unslashed, len(eligible), int(in_leak)
    st.n_slashed_eligible = sum(1 for v in eligible if not r.active_prev[v])

    if which & DO_INACTIVITY:
        for v in eligible:
            if in_unslashed(r, v, TIMELY_TARGET_FLAG_INDEX):
                r.scores[v] -= min(1, r.scores[v])
            else:
                r.scores[v] = u64(r.scores[v] + p.inactivity_score_bias, "score + bias")
            if not in_leak:
                r.scores[v] -= min(p.inactivity_score_recovery_rate, r.scores[v])
    if not which & DO_DELTAS:
        return st

    per_increment = base_reward_per_increment(total_active, p)
    active_increments = total_active // p.increment

    def base_reward(v):
        return u64(r.effective_balance[v] // p.increment * per_increment, "base_reward")

    pairs = []
    for f in range(3):
        rewards, penalties = [0] * n, [0] * n
        unslashed_increments = unslashed[f] // p.increment
        for v in eligible:
            if in_unslashed(r, v, f):
                if not in_leak:
                    numerator = u64(base_reward(v) * PARTICIPATION_FLAG_WEIGHTS[f] * unslashed_increments, "reward numerator")
                    rewards[v] = numerator // (active_increments * WEIGHT_DENOMINATOR)
            elif f != TIMELY_HEAD_FLAG_INDEX:
                penalties[v] = u64(base_reward(v) * PARTICIPATION_FLAG_WEIGHTS[f], "penalty numerator") // WEIGHT_DENOMINATOR
        st.n_flag_rewards += sum(1 for x in rewards if x)
        st.n_flag_penalties += sum(1 for x in penalties if x)
        pairs.append((rewards, penalties))
    rewards, penalties = [0] * n, [0] * n
    for v in eligible:
        if not in_unslashed(r, v, TIMELY_TARGET_FLAG_INDEX):
            penalties[v] = u64(r.effective_balance[v] * r.scores[v], "inactivity numerator") // inactivity_divisor
    st.n_inactivity_penalties = sum(1 for x in penalties if x)
    pairs.append((rewards, penalties))

    if pairs_out is not None:
        pairs_out.extend(pairs)
    saturated = [False] * n
    for rewards, penalties in pairs:                       # one pair after the other: never the netted deltas
        for v in range(n):
            r.balances[v] = (r.balances[v] + rewards[v]) % 2**64   # increase_balance (the engine does not check this sum)
            st.rewards += rewards[v]
            cut = min(penalties[v], r.balances[v])         # decrease_balance
            saturated[v] |= penalties[v] > r.balances[v]
            r.balances[v] -= cut
            st.penalties += cut
    st.rewards %= 2**64
    st.penalties %= 2**64
    st.n_saturated = sum(saturated)
    return st


# ------------------------------------------------------------------------------------------------ numpy form
def run_numpy(eff, sflags, participation, withdrawable, balances, scores, current_epoch: int, finalized_epoch: int,
              p: Params = None, which: int = DO_BOTH):
    """The same rule over numpy uint64 arrays -> (new balances, new scores, Stats).  The call bounds of check_call_bounds
    keep every product inside uint64, so the array arithmetic is exact."""
    p = p or Params()
    U = np.uint64
    eff, balances, scores = (np.asarray(a, dtype=U) for a in (eff, balances, scores))
    withdrawable = np.asarray(withdrawable, dtype=U)
    sflags, participation = np.asarray(sflags, dtype=np.uint8), np.asarray(participation, dtype=np.uint8)
    inactivity_divisor = u64(p.inactivity_score_bias * p.inactivity_penalty_quotient, "bias * quotient")
    st = Stats()
    if current_epoch == GENESIS_EPOCH:
        return balances.copy(), scores.copy(), st
    previous_epoch = get_previous_epoch(current_epoch)
    in_leak = is_in_inactivity_leak(current_epoch, finalized_epoch, p)
    active_prev, slashed = (sflags & VAL_ACTIVE_PREV) != 0, (sflags & VAL_SLASHED) != 0
    eligible = active_prev | (slashed & (U(previous_epoch + 1) < withdrawable))
    unslashed_in = [active_prev & ~slashed & (((participation >> f) & 1) != 0) for f in range(3)]

    def total(mask):
        return max(p.increment, int(eff[mask].sum(dtype=U)))

    total_active = total((sflags & VAL_ACTIVE) != 0)
    unslashed = [total(m) for m in unslashed_in]
    # the call bounds, from the same maxima
    per_increment = base_reward_per_increment(total_active, p)
    u64(total_active // p.increment * WEIGHT_DENOMINATOR, "active increments * WEIGHT_DENOMINATOR")
    max_eff = int(eff[eligible].max()) if eligible.any() else 0
    max_score = int(scores[eligible].max()) if eligible.any() else 0
    if which & DO_DELTAS:
        largest_unslashed = 1 if in_leak else max(u // p.increment for u in unslashed)
        u64(max_eff // p.increment * per_increment * max(PARTICIPATION_FLAG_WEIGHTS) * largest_unslashed, "reward numerator")
    score_bound = u64(max_score + (p.inactivity_score_bias if which & DO_INACTIVITY else 0), "score + bias")
    if which & DO_DELTAS:
        u64(max_eff * score_bound, "inactivity numerator")
    st.total_active_balance, st.unslashed_balance, st.n_eligible, st.in_leak = total_active, unslashed, int(eligible.sum()), int(in_leak)
    st.n_slashed_eligible = int((eligible & ~active_prev).sum())

    scores = scores.copy()
    if which & DO_INACTIVITY:
        hit = eligible & unslashed_in[TIMELY_TARGET_FLAG_INDEX]
        miss = eligible & ~unslashed_in[TIMELY_TARGET_FLAG_INDEX]
        scores[hit] -= np.minimum(U(1), scores[hit])
        scores[miss] += U(p.inactivity_score_bias)
        if not in_leak:
            scores[eligible] -= np.minimum(U(p.inactivity_score_recovery_rate), scores[eligible])
    balances = balances.copy()
    if not which & DO_DELTAS:
        return balances, scores, st

    base = eff // U(p.increment) * U(per_increment)
    zero = np.zeros(eff.size, dtype=U)
    saturated = np.zeros(eff.size, dtype=bool)

    def apply(rewards, penalties):
        nonlocal balances, saturated
        balances = balances + rewards                       # uint64 array arithmetic wraps, as the engine's sum does
        st.rewards += int(rewards.sum(dtype=U))
        saturated |= penalties > balances
        cut = np.minimum(penalties, balances)
        balances = balances - cut
        st.penalties += int(cut.sum(dtype=U))

    for f in range(3):
        w = U(PARTICIPATION_FLAG_WEIGHTS[f])
        got = eligible & unslashed_in[f]
        rewards, penalties = zero.copy(), zero.copy()
        if not in_leak:
            rewards[got] = base[got] * w * U(unslashed[f] // p.increment) // U(total_active // p.increment * WEIGHT_DENOMINATOR)
        if f != TIMELY_HEAD_FLAG_INDEX:
            lost = eligible & ~unslashed_in[f]
            penalties[lost] = base[lost] * w // U(WEIGHT_DENOMINATOR)
        st.n_flag_rewards += int(np.count_nonzero(rewards))
        st.n_flag_penalties += int(np.count_nonzero(penalties))
        apply(rewards, penalties)
    penalties = zero.copy()
    miss = eligible & ~unslashed_in[TIMELY_TARGET_FLAG_INDEX]
    penalties[miss] = eff[miss] * scores[miss] // U(inactivity_divisor)
    st.n_inactivity_penalties = int(np.count_nonzero(penalties))
    apply(zero, penalties)
    st.rewards %= 2**64
    st.penalties %= 2**64
    st.n_saturated = int(saturated.sum())
    return balances, scores, st


def registry_from_arrays(eff, sflags, participation, withdrawable, balances, scores) -> Registry:
    sflags = [int(x) for x in sflags]
    return Registry(effective_balance=[int(x) for x in eff], slashed=[int(bool(f & VAL_SLASHED)) for f in sflags],
                    active_prev=[int(bool(f & VAL_ACTIVE_PREV)) for f in sflags],
                    active_cur=[int(bool(f & VAL_ACTIVE)) for f in sflags], participation=[int(x) for x in participation],
                    withdrawable_epoch=[int(x) for x in withdrawable], balances=[int(x) for x in balances],
                    scores=[int(x) for x in scores])


# ------------------------------------------------------------------------------------------------ random registries
def penalty_edges(p: Params, eff: int = 32 * 10**9, per_increment: int = 349, score: int = 17) -> List[int]:
    """Balances one below, at and one above each penalty a validator of `eff` can meet: the two flag penalties and the
    inactivity penalty of `score`."""
    base = eff // p.increment * per_increment
    pens = [base * 14 // 64, base * 26 // 64, eff * score // (p.inactivity_score_bias * p.inactivity_penalty_quotient)]
    return sorted({max(0, x + d) for x in pens for d in (-1, 0, 1)})


def random_registry(n: int, seed: int, current_epoch: int, p: Params = None):
    """-> dict of numpy arrays (eff, sflags, participation, withdrawable, balances, scores): a mix that holds every
    combination of active-prev / active-cur / slashed, withdrawable before / at / after previous_epoch + 1, all eight flag
    values plus junk high bits, balances in {0, 1, around each penalty, large} and scores in {0, 1, 15, 16, 17, large}."""
    p = p or Params()
    rng = np.random.default_rng(seed)
    edge = get_previous_epoch(current_epoch) + 1
    v = np.arange(n)
    perm = rng.permutation(n)                      # class k of every axis falls on validators of every other class
    sflags = np.array([(VAL_ACTIVE if k & 1 else 0) | (VAL_SLASHED if k & 2 else 0) | (VAL_ACTIVE_PREV if k & 4 else 0)
                       for k in range(8)], dtype=np.uint8)[rng.integers(0, 8, n)]
    if n >= 8:
        sflags[perm[:8]] = [(VAL_ACTIVE if k & 1 else 0) | (VAL_SLASHED if k & 2 else 0) | (VAL_ACTIVE_PREV if k & 4 else 0)
                            for k in range(8)]
    withdrawable = np.array([max(edge - 1, 0), edge, edge + 1, FAR_FUTURE_EPOCH], dtype=np.uint64)[rng.integers(0, 4, n)]
    participation = (rng.integers(0, 8, n) | (rng.integers(0, 32, n) << 3) * (v % 3 == 0)).astype(np.uint8)
    eff = (np.array([32, 32, 32, 31, 16, 1, 0], dtype=np.uint64)[rng.integers(0, 7, n)] * np.uint64(p.increment)).astype(np.uint64)
    edges = penalty_edges(p)
    pool = np.array([0, 1] + edges + [32 * 10**9, 32 * 10**9 + 5, 2**40], dtype=np.uint64)
    balances = pool[rng.integers(0, pool.size, n)]
    scores = np.array([0, 1, 15, 16, 17, 2**20 + 3, 2**27], dtype=np.uint64)[rng.integers(0, 7, n)]
    return dict(eff=eff, sflags=sflags, participation=participation, withdrawable=withdrawable, balances=balances,
                scores=scores)


# ------------------------------------------------------------------------------------------------ the golden file
E32 = 32 * 10**9
ISSUE_PARAMS = Params(inactivity_penalty_quotient=3 * 2**24)


def issue_registry() -> Registry:
    """The cross-check vector of the pull request that added this model: eight validators."""
    far = FAR_FUTURE_EPOCH
    return Registry(effective_balance=[E32, E32, E32, 31 * 10**9, E32, E32, 16 * 10**9, E32],
                    slashed=[0, 0, 0, 0, 1, 1, 0, 0], active_prev=[1, 1, 1, 1, 1, 0, 1, 0], active_cur=[1, 1, 1, 1, 1, 0, 1, 1],
                    participation=[7, 3, 1, 0, 7, 7, 6, 7], withdrawable_epoch=[far, far, far, far, 20, 10, far, far],
                    balances=[E32 + 5, E32, 31 * 10**9, 3000, E32, 30 * 10**9, 0, E32], scores=[0, 1, 20, 100, 7, 50, 3, 9])


def golden_cases():
    """-> list of dicts: name, params, inputs, (current_epoch, finalized_epoch, which) and the model's outputs."""
    import copy
    out = []

    def case(name, reg, current, finalized, params, which=DO_BOTH):
        after = copy.deepcopy(reg)
        st = run(after, current, finalized, params, which)
        out.append(dict(name=name, params=vars(params), current_epoch=current, finalized_epoch=finalized, which=which,
                        registry={k: [int(x) for x in val] for k, val in vars(reg).items()},
                        balances=after.balances, scores=after.scores, stats=st.abi(),
                        classes=[st.n_slashed_eligible, st.n_flag_rewards, st.n_flag_penalties, st.n_inactivity_penalties]))

    reg = issue_registry()
    case("issue_no_leak", reg, 10, 8, ISSUE_PARAMS)
    case("issue_leak", reg, 10, 3, ISSUE_PARAMS)
    case("issue_genesis", reg, 0, 0, ISSUE_PARAMS)
    case("issue_epoch_9_validator_5_eligible", reg, 9, 7, ISSUE_PARAMS)
    case("issue_inactivity_only", reg, 10, 8, ISSUE_PARAMS, DO_INACTIVITY)
    case("issue_deltas_only", reg, 10, 3, ISSUE_PARAMS, DO_DELTAS)
    case("issue_epoch_1", reg, 1, 0, ISSUE_PARAMS)
    case("issue_delay_4_is_no_leak", reg, 10, 5, ISSUE_PARAMS)
    case("issue_delay_5_is_a_leak", reg, 10, 4, ISSUE_PARAMS)
    case("issue_bellatrix_quotient", reg, 10, 3, Params())
    for seed, n, current, finalized in ((1, 40, 12, 10), (2, 40, 12, 2), (3, 67, 5, 4)):
        a = random_registry(n, seed, current)
        case(f"random_{seed}", registry_from_arrays(**a), current, finalized, Params())
    return out


GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rewards_vectors.json")

if __name__ == "__main__":
    with open(GOLDEN_PATH, "w") as fh:
        json.dump(golden_cases(), fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print("wrote", GOLDEN_PATH)
