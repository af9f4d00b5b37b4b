// registry_row.h -- what process_registry_updates and process_slashings (restated in tests/registry_updates_model.py: the
// reference holds their fields, pe:36-45 and pe:359/397, and names get_validator_churn_limit, pe:1261/1270, not their text)
// ask of ONE validator, given the registry-wide scalars of the call.  One text for k_registry_census / k_registry_select /
// k_registry_apply / k_slashings_* (registry_kernels.hip) and for the host (engine_epoch.cpp forms the scalars;
// tests/native/registry_row_host.cpp runs the rules under a plain host compiler and tests/test_registry_row_host.py holds
// them to the model), like reward_row.h.
//
// Every comparison is the reference's unsigned 64-bit; FAR_FUTURE_EPOCH = 2^64 - 1 is an ordinary value.  The divisions are
// by divisors every validator of a call shares and travel as U64Div (reward_row.h).
#pragma once
#include <stdint.h>

#include "pe_hd.h"
#include "reward_row.h"

namespace posevo {

constexpr uint64_t REGISTRY_FAR_FUTURE_EPOCH = ~(uint64_t)0;

// ------------------------------------------------------------------ process_registry_updates
// The scalars of one call, the same for every validator (the host step of pe_registry_updates forms them)
struct RegistryScalars {
    uint64_t current_epoch;
    uint64_t finalized_epoch;
    uint64_t max_effective_balance;
    uint64_t ejection_balance;
    uint64_t eligibility_mark;   // current_epoch + 1: what the mark writes
    uint64_t exit_base;          // the exit queue's closed form: the k-th fresh ejection in index order leaves at
    uint64_t exit_fill;          //   exit_base + (exit_fill + k) / churn_limit
    U64Div by_churn_limit;
    uint64_t withdrawability_delay;
    uint64_t activation_epoch;   // compute_activation_exit_epoch(current_epoch) = current_epoch + 1 + MAX_SEED_LOOKAHEAD
    uint64_t threshold;          // T: queued validators below it are all activated ...
    uint64_t threshold_take;     // r: ... and the first r in index order of those at it
    uint32_t take_all;           // the whole queue fits the activation churn limit: T and r are not read
    uint32_t pad;
};

// is_active_validator: the predicate of k_active_compact
PE_HD bool registry_active(uint64_t activation_epoch, uint64_t exit_epoch, uint64_t epoch)
{
    return activation_epoch <= epoch && epoch < exit_epoch;
}
// is_eligible_for_activation_queue (Altair): never marked, and a full effective balance
PE_HD bool registry_mark(uint64_t eligibility_epoch, uint64_t effective_balance, uint64_t max_effective_balance)
{
    return eligibility_epoch == REGISTRY_FAR_FUTURE_EPOCH && effective_balance == max_effective_balance;
}
// active with an effective balance at or below EJECTION_BALANCE: initiate_validator_exit is called ...
PE_HD bool registry_eject(uint64_t activation_epoch, uint64_t exit_epoch, uint64_t effective_balance, uint64_t current_epoch,
                          uint64_t ejection_balance)
{
    return registry_active(activation_epoch, exit_epoch, current_epoch) && effective_balance <= ejection_balance;
}
// ... and does something only where no exit is set yet: these alone advance k
PE_HD bool registry_eject_fresh(uint64_t activation_epoch, uint64_t exit_epoch, uint64_t effective_balance,
                                uint64_t current_epoch, uint64_t ejection_balance)
{
    return exit_epoch == REGISTRY_FAR_FUTURE_EPOCH &&
           registry_eject(activation_epoch, exit_epoch, effective_balance, current_epoch, ejection_balance);
}
// the exit epoch of the k-th fresh ejection in index order (k from 0)
PE_HD uint64_t registry_exit_epoch(uint64_t base, uint64_t fill, uint64_t k, const U64Div& by_churn_limit)
{
    return base + u64_div(fill + k, by_churn_limit);
}
// is_eligible_for_activation: in the activation queue (finalized eligibility, not yet activated)
PE_HD bool registry_queued(uint64_t eligibility_epoch, uint64_t activation_epoch, uint64_t finalized_epoch)
{
    return eligibility_epoch <= finalized_epoch && activation_epoch == REGISTRY_FAR_FUTURE_EPOCH;
}
// a queued validator among the first activation_churn_limit by (eligibility epoch, index); tie_rank = its rank in index
// order among the queued validators whose eligibility epoch is the threshold (read only there)
PE_HD bool registry_activated(const RegistryScalars& S, uint64_t eligibility_epoch, uint64_t tie_rank)
{
    if (S.take_all) return true;
    return eligibility_epoch < S.threshold || (eligibility_epoch == S.threshold && tie_rank < S.threshold_take);
}

// The exit queue's start from what the census read back: E0 = max(largest exit epoch set, activation_exit_epoch), c0 = the
// validators that hold E0 (0 where E0 is the look-ahead epoch and nobody leaves then).  A full epoch is skipped.
static inline void registry_exit_start(uint64_t max_exit, uint64_t n_at_max, bool any_exit, uint64_t activation_exit_epoch,
                                       uint64_t churn_limit, uint64_t* base, uint64_t* fill)
{
    uint64_t e0 = activation_exit_epoch, c0 = 0;
    if (any_exit && max_exit >= activation_exit_epoch) {
        e0 = max_exit;
        c0 = n_at_max;
    }
    if (c0 >= churn_limit) {
        *base = e0 + 1;
        *fill = 0;
    } else {
        *base = e0;
        *fill = c0;
    }
}

// get_validator_churn_limit and (Deneb) get_validator_activation_churn_limit; cap 0 = no cap.  quotient >= 1.
static inline uint64_t registry_churn_limit(uint64_t n_active, uint64_t min_per_epoch, uint64_t quotient)
{
    const uint64_t q = n_active / quotient;
    return q > min_per_epoch ? q : min_per_epoch;
}
static inline uint64_t registry_activation_churn_limit(uint64_t churn_limit, uint64_t cap)
{
    return cap && cap < churn_limit ? cap : churn_limit;
}

// (largest exit epoch set, how many hold it): on equal maxima the counts add, otherwise the larger maximum wins.  count 0 =
// the empty pair (epoch is then not read).
struct RegistryExitMax {
    uint64_t epoch;
    uint64_t count;
};
PE_HD RegistryExitMax registry_exit_max_join(const RegistryExitMax& a, const RegistryExitMax& b)
{
    if (a.count == 0) return b;
    if (b.count == 0) return a;
    if (a.epoch == b.epoch) return RegistryExitMax{a.epoch, a.count + b.count};
    return a.epoch > b.epoch ? a : b;
}

// ------------------------------------------------------------------ process_slashings
struct SlashingScalars {
    uint64_t target_epoch;    // current_epoch + EPOCHS_PER_SLASHINGS_VECTOR / 2: the withdrawable epoch the penalty falls on
    uint64_t adjusted;        // min(sum(slashings) * PROPORTIONAL_SLASHING_MULTIPLIER, total_active_balance)
    uint64_t increment;
    U64Div by_increment;
    U64Div by_total;          // / total_active_balance (never below the increment)
};

PE_HD bool slashing_applies(uint32_t sflags, uint64_t withdrawable_epoch, uint64_t target_epoch)
{
    return (sflags & REWARD_VAL_SLASHED) && withdrawable_epoch == target_epoch;
}
// effective_balance // INCREMENT * adjusted // total * INCREMENT (the host step has refused a product beyond 64 bits)
PE_HD uint64_t slashing_penalty(const SlashingScalars& S, uint64_t effective_balance)
{
    return u64_div(u64_div(effective_balance, S.by_increment) * S.adjusted, S.by_total) * S.increment;
}

}  // namespace posevo
