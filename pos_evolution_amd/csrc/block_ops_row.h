// block_ops_row.h -- what process_proposer_slashing, process_attester_slashing and process_voluntary_exit (restated in
// tests/block_ops_model.py: the reference holds the Validator fields, pe:36-45, `slashings`, pe:359/397, and
// is_slashable_attestation_data, pe:1134-1143, not slash_validator, initiate_validator_exit or the three functions' text) ask
// of ONE validator and ONE candidate, given the scalars of the call.  One text for the k_block_ops_* kernels
// (block_ops_kernels.hip), for the host step (engine_block_ops.cpp) and for a plain host compiler
// (tests/native/block_ops_row_host.cpp, held to the model by tests/test_block_ops_row_host.py), like registry_row.h, whose
// registry_active, registry_exit_start and registry_exit_epoch the exit queue goes through here too.
//
// A CANDIDATE is one (operation, validator) pair in operation order: every member of an attester slashing's intersection in
// ascending index order, a proposer slashing's proposer, an exit's validator.  Its position is its SLOT.  A candidate is
// POTENT if everything that does not depend on earlier operations of the call holds for it: the operation's own checks (the
// data, the headers, the lists, the verdict, exit.epoch) and the resident row (slashable / active, no exit set, old enough).
// Within one call a validator's row changes in two ways only -- it is slashed (never slashable again) or it gets an exit epoch
// beyond current_epoch (still active, still slashable, never exits again) -- so the sequential loop reduces to two minima per
// validator: the first potent candidate of any kind (first_potent) and the first potent slashing candidate (first_slash).
//   a slashing candidate slashes      iff it is potent and its slot is first_slash
//   an exit candidate takes effect    iff it is potent and its slot is first_potent
//   a fresh exit epoch is assigned    at first_potent, iff no exit epoch was set before the call
// Every comparison is the reference's unsigned 64-bit; FAR_FUTURE_EPOCH = 2^64 - 1 is an ordinary value.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pe_hd.h"
#include "registry_row.h"
#include "reward_row.h"

namespace posevo {

// pe_block_op.kind and the per-operation statuses (include/posevo.h: PE_OP_*; engine_block_ops.cpp asserts the equality)
constexpr uint32_t BLOCK_OP_PROPOSER_SLASHING = 1, BLOCK_OP_ATTESTER_SLASHING = 2, BLOCK_OP_VOLUNTARY_EXIT = 3;
constexpr uint32_t BLOCK_OP_OK = 0, BLOCK_OP_NOT_SLASHABLE_DATA = 64, BLOCK_OP_BAD_INDICES = 65, BLOCK_OP_BAD_SIGNATURE = 66,
                   BLOCK_OP_NOBODY_SLASHABLE = 67, BLOCK_OP_HEADER_MISMATCH = 68, BLOCK_OP_PROPOSER_NOT_SLASHABLE = 69,
                   BLOCK_OP_NOT_ACTIVE = 70, BLOCK_OP_ALREADY_EXITING = 71, BLOCK_OP_EXIT_EPOCH_FUTURE = 72,
                   BLOCK_OP_TOO_YOUNG = 73;
constexpr uint32_t BLOCK_OPS_NONE = 0xFFFFFFFFu;  // no validator in a slot | no slot in a table

// What the host decides of an operation before any kernel runs.  PRE_OK: every check that reads neither the registry nor
// the index lists passed.  An operation whose status the host alone decides takes no slots.
constexpr uint32_t BLOCK_OP_PRE_OK = 1u, BLOCK_OP_PRE_BAD_SIGNATURE = 2u, BLOCK_OP_PRE_EPOCH_FUTURE = 4u;

// One operation as the kernels read it: attester slashing: the two ranges of the flat index array, len1 + len2 slots (the
// first list's elements, then the second's, which are only checked); the others: `index`, one slot.
struct BlockOpDev {
    uint32_t kind, pre;
    uint32_t off1, len1, off2, len2;
    uint32_t index, pad;
};

// what k_block_ops_resolve leaves per slot for k_block_ops_apply
constexpr uint32_t BLOCK_EV_FRESH_EXIT = 1u;   // this candidate's validator gets the next exit epoch of the queue
constexpr uint32_t BLOCK_EV_SLASH = 2u;        // this candidate slashes its validator
constexpr uint32_t BLOCK_EV_EXIT_WAS_SET = 4u; // ... whose exit epoch was set before the call: the slash lane writes withdrawable

// The scalars of one call, the same for every candidate (the host step of pe_process_block_operations forms them)
struct BlockOpsScalars {
    uint64_t current_epoch;
    uint64_t shard_committee_period;
    uint64_t exit_base, exit_fill;    // the k-th fresh exit in operation order leaves at registry_exit_epoch(base, fill, k)
    U64Div by_churn_limit;
    uint64_t withdrawability_delay;
    uint64_t slashed_withdrawable;    // current_epoch + EPOCHS_PER_SLASHINGS_VECTOR
    U64Div by_penalty_quotient;       // / MIN_SLASHING_PENALTY_QUOTIENT
    U64Div by_reward_quotient;        // / WHISTLEBLOWER_REWARD_QUOTIENT
    uint64_t total_rewards;           // every slashing's reward: all go to the proposer
    uint32_t proposer_index;
    uint32_t n_slots;
};

// is_slashable_validator
PE_HD bool block_ops_slashable(uint32_t sflags, uint64_t activation_epoch, uint64_t withdrawable_epoch, uint64_t epoch)
{
    return !(sflags & REWARD_VAL_SLASHED) && activation_epoch <= epoch && epoch < withdrawable_epoch;
}

// process_voluntary_exit's asserts in their order.  already_exiting: an earlier candidate of this call took effect on the
// validator.  activation_epoch <= current_epoch where the age is read, so the subtraction is the comparison without a wrap.
PE_HD uint32_t block_ops_exit_status(uint64_t activation_epoch, uint64_t exit_epoch, uint64_t current_epoch,
                                     uint64_t shard_committee_period, bool already_exiting, uint32_t pre)
{
    if (!registry_active(activation_epoch, exit_epoch, current_epoch)) return BLOCK_OP_NOT_ACTIVE;
    if (exit_epoch != REGISTRY_FAR_FUTURE_EPOCH || already_exiting) return BLOCK_OP_ALREADY_EXITING;
    if (pre & BLOCK_OP_PRE_EPOCH_FUTURE) return BLOCK_OP_EXIT_EPOCH_FUTURE;
    if (current_epoch - activation_epoch < shard_committee_period) return BLOCK_OP_TOO_YOUNG;
    if (pre & BLOCK_OP_PRE_BAD_SIGNATURE) return BLOCK_OP_BAD_SIGNATURE;
    return BLOCK_OP_OK;
}
// process_proposer_slashing behind the header checks (the host's)
PE_HD uint32_t block_ops_proposer_status(bool slashable, bool slashed_earlier, uint32_t pre)
{
    if (!slashable || slashed_earlier) return BLOCK_OP_PROPOSER_NOT_SLASHABLE;
    if (pre & BLOCK_OP_PRE_BAD_SIGNATURE) return BLOCK_OP_BAD_SIGNATURE;
    return BLOCK_OP_OK;
}

// A candidate's potency from its operation and the resident row.  lists_bad: the attester slashing's lists failed.
PE_HD bool block_ops_potent(uint32_t kind, uint32_t pre, bool lists_bad, uint32_t sflags, uint64_t activation_epoch,
                            uint64_t exit_epoch, uint64_t withdrawable_epoch, uint64_t current_epoch,
                            uint64_t shard_committee_period)
{
    if (kind == BLOCK_OP_VOLUNTARY_EXIT)
        return block_ops_exit_status(activation_epoch, exit_epoch, current_epoch, shard_committee_period, false, pre) == BLOCK_OP_OK;
    return (pre & BLOCK_OP_PRE_OK) && !lists_bad && block_ops_slashable(sflags, activation_epoch, withdrawable_epoch, current_epoch);
}

// what a candidate does, from the two tables' entries of its validator (BLOCK_EV_*)
PE_HD uint32_t block_ops_events(uint32_t kind, bool potent, uint32_t slot, uint32_t first_potent, uint32_t first_slash,
                                uint64_t exit_epoch)
{
    if (!potent) return 0;
    uint32_t ev = 0;
    if (kind != BLOCK_OP_VOLUNTARY_EXIT && slot == first_slash)
        ev |= BLOCK_EV_SLASH | (exit_epoch != REGISTRY_FAR_FUTURE_EPOCH ? BLOCK_EV_EXIT_WAS_SET : 0u);
    if (slot == first_potent && exit_epoch == REGISTRY_FAR_FUTURE_EPOCH) ev |= BLOCK_EV_FRESH_EXIT;
    return ev;
}

// slash_validator's withdrawable epoch
PE_HD uint64_t block_ops_slashed_withdrawable(uint64_t withdrawable_epoch, uint64_t slashed_withdrawable)
{
    return withdrawable_epoch > slashed_withdrawable ? withdrawable_epoch : slashed_withdrawable;
}

// slash_validator on the balance of the slashed validator: decrease_balance's cut at 0, and -- where it is the proposer, the
// j-th slashing of the call -- the closed form of the sequential loop: the rewards of the slashings before it have arrived
// when the penalty falls, the others (its own included) come afterwards.  rewards_before = total_rewards = 0 for anyone else.
// The host step has refused a call whose sums could leave 64 bits.
struct BlockOpsDebit {
    uint64_t balance, debited;
    uint32_t saturated;
};
PE_HD BlockOpsDebit block_ops_slash_balance(uint64_t balance, uint64_t penalty, uint64_t rewards_before, uint64_t total_rewards)
{
    BlockOpsDebit r;
    const uint64_t at_slash = balance + rewards_before;
    r.saturated = penalty > at_slash ? 1u : 0u;
    r.debited = r.saturated ? at_slash : penalty;
    r.balance = at_slash - r.debited + (total_rewards - rewards_before);
    return r;
}

// is_slashable_attestation_data over two AttestationData as they travel (the leading 128 bytes of a pe_attestation: slot,
// index, beacon_block_root, source epoch at byte 48 and root, target epoch at byte 88 and root), as pe_on_attester_slashing
// reads it: a double vote or a surround vote.  Host only.
static inline bool block_ops_slashable_data(const uint8_t d1[128], const uint8_t d2[128])
{
    uint64_t s1, t1, s2, t2;
    memcpy(&s1, d1 + 48, 8);
    memcpy(&t1, d1 + 88, 8);
    memcpy(&s2, d2 + 48, 8);
    memcpy(&t2, d2 + 88, 8);
    const bool double_vote = memcmp(d1, d2, 128) != 0 && t1 == t2;
    const bool surround = s1 < s2 && t2 < t1;
    return double_vote || surround;
}

// ------------------------------------------------------------------ the host's two steps (no device attribute)
// pe_block_op of include/posevo.h, field for field (engine_block_ops.cpp asserts size and offsets)
struct BlockOpHost {
    uint32_t kind, flags;
    uint8_t data_1[128], data_2[128];
    uint64_t indices_1_offset, indices_1_length, indices_2_offset, indices_2_length;
    uint64_t header_1_slot, header_1_proposer_index;
    uint8_t header_1_root[32];
    uint64_t header_2_slot, header_2_proposer_index;
    uint8_t header_2_root[32];
    uint64_t validator_index, exit_epoch;
};
constexpr uint32_t BLOCK_OP_FLAG_SIGNATURE_VALID = 1u;
constexpr uint64_t BLOCK_OPS_MAX_SLOTS = (uint64_t)1 << 31;  // slots and indices of one call stay below this

// Before any kernel: what an operation's own fields decide.  -> 0, or 1: unknown kind, 2: a range runs past n_indices (or
// beyond BLOCK_OPS_MAX_SLOTS).  *status: the status the host alone decides (the operation then takes no slots), else
// BLOCK_OP_OK -- to be settled by the kernels.
static inline int block_ops_prepare(const BlockOpHost& op, uint64_t n_val, uint64_t n_indices, uint64_t current_epoch,
                                    BlockOpDev* out, uint32_t* status)
{
    BlockOpDev d;
    memset(&d, 0, sizeof d);
    d.kind = op.kind;
    *status = BLOCK_OP_OK;
    const bool sig = op.flags & BLOCK_OP_FLAG_SIGNATURE_VALID;
    if (op.kind == BLOCK_OP_ATTESTER_SLASHING) {
        if (op.indices_1_offset > n_indices || op.indices_1_length > n_indices - op.indices_1_offset ||
            op.indices_2_offset > n_indices || op.indices_2_length > n_indices - op.indices_2_offset || n_indices >= BLOCK_OPS_MAX_SLOTS)
            return 2;
        if (!block_ops_slashable_data(op.data_1, op.data_2)) *status = BLOCK_OP_NOT_SLASHABLE_DATA;
        else if (op.indices_1_length == 0 || op.indices_2_length == 0) *status = BLOCK_OP_BAD_INDICES;
        d.pre = sig ? BLOCK_OP_PRE_OK : BLOCK_OP_PRE_BAD_SIGNATURE;
        if (*status == BLOCK_OP_OK) {
            d.off1 = (uint32_t)op.indices_1_offset;
            d.len1 = (uint32_t)op.indices_1_length;
            d.off2 = (uint32_t)op.indices_2_offset;
            d.len2 = (uint32_t)op.indices_2_length;
        }
    } else if (op.kind == BLOCK_OP_PROPOSER_SLASHING) {
        if (op.header_1_slot != op.header_2_slot || op.header_1_proposer_index != op.header_2_proposer_index ||
            memcmp(op.header_1_root, op.header_2_root, 32) == 0)
            *status = BLOCK_OP_HEADER_MISMATCH;
        else if (op.header_1_proposer_index >= n_val) *status = BLOCK_OP_BAD_INDICES;
        d.pre = sig ? BLOCK_OP_PRE_OK : BLOCK_OP_PRE_BAD_SIGNATURE;
        d.index = (uint32_t)op.header_1_proposer_index;
    } else if (op.kind == BLOCK_OP_VOLUNTARY_EXIT) {
        if (op.validator_index >= n_val) *status = BLOCK_OP_BAD_INDICES;
        d.pre = (sig ? 0u : BLOCK_OP_PRE_BAD_SIGNATURE) | (current_epoch >= op.exit_epoch ? 0u : BLOCK_OP_PRE_EPOCH_FUTURE);
        if (d.pre == 0) d.pre = BLOCK_OP_PRE_OK;
        d.index = (uint32_t)op.validator_index;
    } else {
        return 1;
    }
    *out = d;
    return 0;
}
// the slots an operation takes
static inline uint64_t block_ops_slots(const BlockOpDev& d, uint32_t host_status)
{
    if (host_status != BLOCK_OP_OK) return 0;
    return d.kind == BLOCK_OP_ATTESTER_SLASHING ? (uint64_t)d.len1 + d.len2 : 1;
}

// what the read-only passes found, summed over the call's candidates
struct BlockOpsTotals {
    unsigned long long n_fresh, n_slashed;     // fresh exit epochs to assign | validators slashed
    unsigned long long rewards, slashed_balance, max_eff_slashed;
    unsigned long long proposer_balance;       // balance[proposer_index] before the call
};
// the constants of the call (pe_block_ops_params, in its order)
struct BlockOpsParams {
    uint64_t min_slashing_penalty_quotient, whistleblower_reward_quotient, epochs_per_slashings_vector, shard_committee_period,
        min_validator_withdrawability_delay, max_seed_lookahead, min_per_epoch_churn_limit, churn_limit_quotient;
};
// -> 0, or what pe_process_block_operations refuses with PE_ERR_INVALID_ARG before any kernel runs:
// 1 a quotient is 0, 2 current_epoch + epochs_per_slashings_vector wraps or reaches FAR, 3 the look-ahead epoch reaches FAR
static inline int block_ops_check_params(const BlockOpsParams& p, uint64_t current_epoch)
{
    typedef unsigned __int128 u128;
    const u128 far = (u128)REGISTRY_FAR_FUTURE_EPOCH;
    if (p.min_slashing_penalty_quotient == 0 || p.whistleblower_reward_quotient == 0 || p.churn_limit_quotient == 0) return 1;
    if ((u128)current_epoch + p.epochs_per_slashings_vector >= far) return 2;
    if ((u128)current_epoch + 1 + p.max_seed_lookahead >= far) return 3;
    return 0;
}
// The host step between the read-only passes and the writing one: the churn limit, the exit queue's start (registry_row.h),
// the scalars, and the refusals -- 4 the churn limit is 0, 5 the last exit epoch + the delay wraps or reaches FAR, 6 the sums
// could leave 64 bits (n_slashed * the largest slashed effective balance + the proposer's balance: every reward, every sum
// of rewards and the slashed balance lie below that).
static inline int block_ops_scalars_make(const BlockOpsParams& p, uint64_t current_epoch, uint32_t proposer_index, uint32_t n_slots,
                                         uint64_t n_active, uint64_t max_exit, uint64_t n_at_max, const BlockOpsTotals& t,
                                         BlockOpsScalars* S, uint64_t* churn_limit, uint64_t* last_exit_epoch)
{
    typedef unsigned __int128 u128;
    const u128 far = (u128)REGISTRY_FAR_FUTURE_EPOCH;
    memset(S, 0, sizeof *S);
    *last_exit_epoch = 0;
    *churn_limit = registry_churn_limit(n_active, p.min_per_epoch_churn_limit, p.churn_limit_quotient);
    if (*churn_limit == 0) return 4;
    registry_exit_start(max_exit, n_at_max, n_at_max != 0, current_epoch + 1 + p.max_seed_lookahead, *churn_limit, &S->exit_base,
                        &S->exit_fill);
    if (t.n_fresh) {
        const u128 last = (u128)S->exit_base + ((u128)S->exit_fill + (t.n_fresh - 1)) / *churn_limit;
        if (last + p.min_validator_withdrawability_delay >= far) return 5;
        *last_exit_epoch = (uint64_t)last;
    }
    if ((u128)t.n_slashed * t.max_eff_slashed + t.proposer_balance > (u128)UINT64_MAX) return 6;
    S->current_epoch = current_epoch;
    S->shard_committee_period = p.shard_committee_period;
    S->by_churn_limit = u64_div_make(*churn_limit);
    S->withdrawability_delay = p.min_validator_withdrawability_delay;
    S->slashed_withdrawable = current_epoch + p.epochs_per_slashings_vector;
    S->by_penalty_quotient = u64_div_make(p.min_slashing_penalty_quotient);
    S->by_reward_quotient = u64_div_make(p.whistleblower_reward_quotient);
    S->total_rewards = t.rewards;
    S->proposer_index = proposer_index;
    S->n_slots = n_slots;
    return 0;
}

// the operation whose slots hold `slot`: slot_off[op] <= slot < slot_off[op + 1] (operations without slots are passed over)
PE_HD uint32_t block_ops_op_of_slot(const uint32_t* slot_off, uint32_t n_ops, uint32_t slot)
{
    uint32_t lo = 0, hi = n_ops;  // the first op in (lo, hi] with slot_off > slot, minus one
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (slot_off[mid] <= slot) lo = mid; else hi = mid;
    }
    return lo;
}
// is x in the ascending list[0 .. len)?
PE_HD bool block_ops_in_list(const uint32_t* list, uint32_t len, uint32_t x)
{
    uint32_t lo = 0, hi = len;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (list[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < len && list[lo] == x;
}

// One slot of an operation: the validator it names (BLOCK_OPS_NONE: none) and whether it shows the operation's lists to be
// bad (not strictly ascending at this element, or an index outside the registry).
struct BlockOpsSlot {
    uint32_t validator;
    uint32_t bad;
};
PE_HD BlockOpsSlot block_ops_slot(const BlockOpDev& op, uint32_t i, const uint32_t* indices, uint64_t n_val)
{
    BlockOpsSlot r;
    r.validator = BLOCK_OPS_NONE;
    r.bad = 0;
    if (op.kind != BLOCK_OP_ATTESTER_SLASHING) {
        r.validator = op.index;
        return r;
    }
    const bool first = i < op.len1;
    const uint32_t* list = indices + (first ? op.off1 : op.off2);
    const uint32_t j = first ? i : i - op.len1;
    const uint32_t x = list[j];
    if (x >= n_val || (j > 0 && list[j - 1] >= x)) r.bad = 1;
    else if (first && block_ops_in_list(indices + op.off2, op.len2, x)) r.validator = x;
    return r;
}

}  // namespace posevo
