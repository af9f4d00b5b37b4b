// reward_row.h -- what process_inactivity_updates and process_rewards_and_penalties (the Altair functions, restated in
// tests/rewards_model.py: the reference holds their fields and callers, not their text) do to ONE validator, given the
// registry-wide scalars of the epoch.  One text for k_reward_sums / k_reward_apply (reward_kernels.hip) and for the host
// (engine_epoch.cpp forms the scalars; tests/native/reward_row_host.cpp runs the rule under a plain host compiler and
// tests/test_reward_row_host.py holds it to the model), like att_row.h over pe_hd.h.
//
// All arithmetic is the reference's uint64.  The three divisions are by divisors every validator of a call shares, and
// gfx950 has no 64-bit divide instruction, so a divisor travels as U64Div: a 64-bit multiplier and two shifts after
// Granlund and Montgomery, "Division by invariant integers using multiplication" (1994), figure 4.1 with N = 64.  That form
// is exact for EVERY numerator below 2^64 and every divisor from 1 to 2^64 - 1; it costs one high multiply, one subtraction,
// one addition and two shifts.
#pragma once
#include <stdint.h>

#include "pe_hd.h"

namespace posevo {

// PARTICIPATION_FLAG_WEIGHTS (Appendix A.9) by flag index = bit of a participation byte: TIMELY_SOURCE, TIMELY_TARGET,
// TIMELY_HEAD; WEIGHT_DENOMINATOR.  (The flag passes of att_kernels.hip / fc_kernels.hip spell the same three weights out
// where they add them up for the proposer's numerator.)
constexpr uint32_t REWARD_FLAG_WEIGHT_SOURCE = 14, REWARD_FLAG_WEIGHT_TARGET = 26, REWARD_FLAG_WEIGHT_HEAD = 14;
constexpr uint32_t REWARD_WEIGHT_DENOMINATOR_LOG2 = 6;  // WEIGHT_DENOMINATOR = 64
constexpr uint32_t REWARD_TIMELY_TARGET = 1, REWARD_TIMELY_HEAD = 2;  // flag indices
// the working-state view's flag byte (include/posevo.h: PE_VAL_ACTIVE, PE_VAL_SLASHED, PE_VAL_ACTIVE_PREV)
constexpr uint32_t REWARD_VAL_ACTIVE_CUR = 0x01u, REWARD_VAL_SLASHED = 0x02u, REWARD_VAL_ACTIVE_PREV = 0x08u;
// `which` of pe_rewards_and_penalties (PE_REWARDS_INACTIVITY, PE_REWARDS_DELTAS)
constexpr uint32_t REWARD_DO_INACTIVITY = 1u, REWARD_DO_DELTAS = 2u;

PE_HD uint32_t reward_flag_weight(uint32_t f)
{
    return f == REWARD_TIMELY_TARGET ? REWARD_FLAG_WEIGHT_TARGET : (f == 0 ? REWARD_FLAG_WEIGHT_SOURCE : REWARD_FLAG_WEIGHT_HEAD);
}

// ------------------------------------------------------------------ n / d for a divisor fixed per call
struct U64Div {
    uint64_t m;    // floor(2^64 (2^l - d) / d) + 1 with l = ceil(log2 d): at most 2^64 - 1
    uint32_t sh1;  // min(l, 1)
    uint32_t sh2;  // max(l - 1, 0)
};

PE_HD uint64_t u64_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor(n / d), exact for every n: t = floor(m n / 2^64) <= n, so neither n - t nor t + ((n - t) >> sh1) leaves 64 bits
PE_HD uint64_t u64_div(uint64_t n, const U64Div& d)
{
    const uint64_t t = u64_mulhi(d.m, n);
    return (t + ((n - t) >> d.sh1)) >> d.sh2;
}

// d >= 1 (the caller's check).  Host only (no device attribute): the one 128-bit division per divisor and call.
static inline U64Div u64_div_make(uint64_t d)
{
    const uint32_t l = d <= 1 ? 0u : 64u - (uint32_t)__builtin_clzll(d - 1);  // ceil(log2 d), 0 .. 64
    const uint64_t pow_minus_d = l == 64 ? (uint64_t)0 - d : ((uint64_t)1 << l) - d;
    U64Div r;
    r.m = (uint64_t)((((unsigned __int128)pow_minus_d) << 64) / d) + 1;
    r.sh1 = l ? 1u : 0u;
    r.sh2 = l ? l - 1 : 0u;
    return r;
}

// ------------------------------------------------------------------ the scalars of one call, the same for every validator
struct RewardScalars {
    uint64_t per_increment;       // INCREMENT * base_reward_factor // integer_squareroot(total_active_balance)
    uint64_t unslashed_incr[3];   // max(INCREMENT, sum over unslashed(f)) // INCREMENT, by flag index: never 0
    uint64_t previous_plus_1;     // previous_epoch + 1: a slashed validator is eligible while this is < withdrawable_epoch
    uint64_t score_bias;          // inactivity_score_bias
    uint64_t score_recovery;      // inactivity_score_recovery_rate
    U64Div by_increment;          // / INCREMENT
    U64Div by_active_weight;      // / (total_active_balance // INCREMENT * WEIGHT_DENOMINATOR)
    U64Div by_inactivity;         // / (inactivity_score_bias * inactivity_penalty_quotient)
    uint32_t in_leak;             // is_in_inactivity_leak
    uint32_t which;               // REWARD_DO_*
};

// integer_squareroot: the largest x with x * x <= n (Newton from above; n + 1 is never formed)
static inline uint64_t reward_isqrt(uint64_t n)
{
    if (n < 2) return n;
    uint64_t x = n, y = n / 2 + (n & 1);
    while (y < x) {
        x = y;
        y = (x + n / x) / 2;
    }
    return x;
}

// The host step between the two kernels: the scalar block from what the first pass read back, and every place the
// reference's uint64 would overflow, in 128-bit arithmetic.  The bounds pair maxima that need not meet in one validator:
// they are conservative.  increment >= 1, inactivity_divisor = bias * quotient >= 1, total_active >= increment (the
// caller's checks and get_total_balance's floor).  -> 0, or which product does not fit (REWARD_OVERFLOW_*); *S is complete
// only with 0.
enum {
    REWARD_OVERFLOW_NONE = 0,
    REWARD_OVERFLOW_FACTOR,         // increment * base_reward_factor
    REWARD_OVERFLOW_ACTIVE_WEIGHT,  // total_active / increment * WEIGHT_DENOMINATOR
    REWARD_OVERFLOW_FLAG_REWARD,    // base_reward * 26 * unslashed increments (base_reward * 26 in a leak)
    REWARD_OVERFLOW_SCORE,          // score + bias
    REWARD_OVERFLOW_INACTIVITY,     // effective_balance * score
};
static inline int reward_scalars_make(uint64_t increment, uint64_t base_reward_factor, uint64_t score_bias,
                                      uint64_t score_recovery, uint64_t inactivity_divisor, uint64_t total_active,
                                      const uint64_t unslashed_balance[3], uint64_t max_eff, uint64_t max_score,
                                      uint64_t previous_epoch, bool in_leak, uint32_t which, RewardScalars* S)
{
    typedef unsigned __int128 u128;
    const u128 lim = (u128)UINT64_MAX;
    uint64_t factor_gwei = 0, active_weight = 0;
    if (__builtin_mul_overflow(increment, base_reward_factor, &factor_gwei)) return REWARD_OVERFLOW_FACTOR;
    if (__builtin_mul_overflow(total_active / increment, (uint64_t)1 << REWARD_WEIGHT_DENOMINATOR_LOG2, &active_weight))
        return REWARD_OVERFLOW_ACTIVE_WEIGHT;
    S->per_increment = factor_gwei / reward_isqrt(total_active);
    uint64_t max_unslashed = 1;
    for (int f = 0; f < 3; ++f) {
        S->unslashed_incr[f] = unslashed_balance[f] / increment;
        if (S->unslashed_incr[f] > max_unslashed) max_unslashed = S->unslashed_incr[f];
    }
    if (which & REWARD_DO_DELTAS) {
        u128 bound = (u128)(max_eff / increment) * S->per_increment;  // the largest base reward
        if (bound <= lim) bound *= REWARD_FLAG_WEIGHT_TARGET;         // ... times the largest weight
        if (bound <= lim && !in_leak) bound *= max_unslashed;         // ... times the largest unslashed increments
        if (bound > lim) return REWARD_OVERFLOW_FLAG_REWARD;
    }
    uint64_t score_bound = max_score;
    if ((which & REWARD_DO_INACTIVITY) && __builtin_add_overflow(max_score, score_bias, &score_bound)) return REWARD_OVERFLOW_SCORE;
    if ((which & REWARD_DO_DELTAS) && (u128)max_eff * score_bound > lim) return REWARD_OVERFLOW_INACTIVITY;
    S->previous_plus_1 = previous_epoch + 1;
    S->score_bias = score_bias;
    S->score_recovery = score_recovery;
    S->by_increment = u64_div_make(increment);
    S->by_active_weight = u64_div_make(active_weight);  // total_active >= increment: at least 64
    S->by_inactivity = u64_div_make(inactivity_divisor);
    S->in_leak = in_leak ? 1u : 0u;
    S->which = which;
    return REWARD_OVERFLOW_NONE;
}

// what one validator adds to the call's statistics
struct RewardRowStats {
    uint64_t rewards;     // Gwei credited
    uint64_t penalties;   // Gwei actually debited (after the cut at 0)
    uint32_t saturated;   // 1 where at least one of the four subtractions was cut at 0
};

PE_HD bool reward_active_prev(uint32_t sflags) { return (sflags & REWARD_VAL_ACTIVE_PREV) != 0; }
// get_eligible_validator_indices: active in the previous epoch, or slashed and not yet withdrawable
PE_HD bool reward_eligible(uint32_t sflags, uint64_t withdrawable_epoch, uint64_t previous_plus_1)
{
    return reward_active_prev(sflags) || ((sflags & REWARD_VAL_SLASHED) && previous_plus_1 < withdrawable_epoch);
}
// get_unslashed_participating_indices(state, f, previous_epoch) holds v.  Bits 3-7 of the byte mean nothing.
PE_HD bool reward_unslashed(uint32_t sflags, uint32_t participation, uint32_t f)
{
    return reward_active_prev(sflags) && !(sflags & REWARD_VAL_SLASHED) && ((participation >> f) & 1u);
}

// process_inactivity_updates for one ELIGIBLE validator
PE_HD uint64_t reward_score_update(const RewardScalars& S, uint32_t sflags, uint32_t participation, uint64_t score)
{
    if (reward_unslashed(sflags, participation, REWARD_TIMELY_TARGET))
        score -= score < 1 ? score : 1;
    else
        score += S.score_bias;
    if (!S.in_leak) score -= score < S.score_recovery ? score : S.score_recovery;
    return score;
}

// increase_balance, then decrease_balance with its cut at 0: one (rewards, penalties) pair
PE_HD uint64_t reward_apply_pair(uint64_t balance, uint64_t reward, uint64_t penalty, RewardRowStats* st)
{
    balance += reward;
    st->rewards += reward;
    if (penalty > balance) {
        st->saturated = 1;
        penalty = balance;
    }
    st->penalties += penalty;
    return balance - penalty;
}

// get_flag_index_deltas for one eligible validator and flag f (written out per flag: the scalar block is indexed by
// constants only)
PE_HD uint64_t reward_flag_pair(const RewardScalars& S, uint32_t f, uint64_t unslashed_incr, uint64_t base_reward,
                                uint32_t sflags, uint32_t participation, uint64_t balance, RewardRowStats* st)
{
    const uint64_t weighted = base_reward * reward_flag_weight(f);
    uint64_t reward = 0, penalty = 0;
    if (reward_unslashed(sflags, participation, f)) {
        if (!S.in_leak) reward = u64_div(weighted * unslashed_incr, S.by_active_weight);
    } else if (f != REWARD_TIMELY_HEAD) {
        penalty = weighted >> REWARD_WEIGHT_DENOMINATOR_LOG2;
    }
    return reward_apply_pair(balance, reward, penalty, st);
}

// The whole rule for one validator: the score first (S.which & REWARD_DO_INACTIVITY), then the four pairs in the
// reference's order over the score as it then stands (S.which & REWARD_DO_DELTAS), each pair applied before the next one is
// looked at -- netting the deltas first gives another answer for small balances.  *st must be zero on entry.
PE_HD void reward_row(const RewardScalars& S, uint64_t effective_balance, uint32_t sflags, uint32_t participation,
                      uint64_t withdrawable_epoch, uint64_t* balance, uint64_t* score, RewardRowStats* st)
{
    if (!reward_eligible(sflags, withdrawable_epoch, S.previous_plus_1)) return;
    uint64_t sc = *score;
    if (S.which & REWARD_DO_INACTIVITY) sc = reward_score_update(S, sflags, participation, sc);
    *score = sc;
    if (!(S.which & REWARD_DO_DELTAS)) return;
    const uint64_t base_reward = u64_div(effective_balance, S.by_increment) * S.per_increment;
    uint64_t bal = *balance;
    bal = reward_flag_pair(S, 0, S.unslashed_incr[0], base_reward, sflags, participation, bal, st);
    bal = reward_flag_pair(S, 1, S.unslashed_incr[1], base_reward, sflags, participation, bal, st);
    bal = reward_flag_pair(S, 2, S.unslashed_incr[2], base_reward, sflags, participation, bal, st);
    uint64_t inactivity = 0;
    if (!reward_unslashed(sflags, participation, REWARD_TIMELY_TARGET)) inactivity = u64_div(effective_balance * sc, S.by_inactivity);
    *balance = reward_apply_pair(bal, 0, inactivity, st);
}

}  // namespace posevo
