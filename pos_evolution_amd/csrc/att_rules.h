// att_rules.h -- which pe_att_status an attestation row gets: the first failing assert, in the spec's order.  One text for
// the host routes (engine_attest.cpp), the device bodies (att_bodies.inc, att_kernels.hip) and a plain-compiler test
// (tests/native/att_rules_host.cpp, which drives the whole boundary matrix through it against tests/att_rules_model.py):
//   fork-choice side   validate_on_attestation (A.4), then the committee (A.6), then is_valid_indexed_attestation (A.7)
//   state side         pe:724-726, the committee with pe:727 and pe:730, is_matching_source and the flag indices (A.9), A.7
// The rules ask for the store, the state and the row through small adapters that hold no rule: how a root is found, how an
// ancestor is walked and how a block root of the state's chain is compared is data access and stays with the caller.
// Over att_row.h and pe_hd.h, nothing but <stdint.h>: compiles under hipcc and under a plain host compiler.
#pragma once
#include <stdint.h>

#include "att_row.h"

namespace posevo {

// pe_att_status, PE_ATT_FLAG_* and the participation flag bits (A.9); engine_internal.h pins them to include/posevo.h
PE_HD_CONST int32_t ST_OK = 0, ST_EPOCH_TIME = 1, ST_EPOCH_SLOT = 2, ST_UNKNOWN_TARGET = 3, ST_UNKNOWN_BLOCK = 4,
                    ST_BLOCK_AFTER_SLOT = 5, ST_TARGET_NOT_ANCESTOR = 6, ST_SLOT_NOT_PAST = 7, ST_NO_TABLE = 8,
                    ST_INDEX_RANGE = 9, ST_BITS_LENGTH = 10, ST_EMPTY = 11, ST_BAD_SIGNATURE = 12, ST_INCLUSION = 13,
                    ST_SOURCE = 14;
PE_HD_CONST uint32_t FLAG_SIG_VALID = 0x1u, FLAG_FROM_BLOCK = 0x2u, FLAG_OVERLAPPING = 0x4u;
PE_HD_CONST uint32_t TIMELY_SOURCE = 0x1u, TIMELY_TARGET = 0x2u, TIMELY_HEAD = 0x4u;
PE_HD_CONST uint32_t ATT_NO_BLOCK = 0xFFFFFFFFu;  // "no such root" of a store adapter

// ------------------------------------------------------------------ validate_on_attestation (A.4)
// `store` answers in block indices: find(root) -> index or ATT_NO_BLOCK, slot_of(index), and get_ancestor (A.2) as
// ancestor(index, slot) -> the store's own handle of that block, which handle(index) gives for any block (the device table
// walks pre-order positions, the host block indices).  The look-ups are lazy: the walk needs a found block.
struct FcVerdict {
    int32_t status;
    uint32_t block;  // index of beacon_block_root, where the ladder came as far as finding it
};
template <class Store, class RootT>
PE_HD FcVerdict att_fork_choice_status(const Store& store, bool from_block, uint64_t slot, uint64_t target_epoch,
                                       const RootT& target_root, const RootT& block_root, uint64_t cur_slot,
                                       uint64_t cur_epoch, uint64_t prev_epoch, uint64_t slots_per_epoch)
{
    FcVerdict v;
    v.block = ATT_NO_BLOCK;
    v.status = ST_OK;
    // validate_target_epoch_against_current_time (skipped for attestations from blocks, pe:1423)
    if (!from_block && target_epoch != cur_epoch && target_epoch != prev_epoch) v.status = ST_EPOCH_TIME;
    else if (target_epoch != slot / slots_per_epoch) v.status = ST_EPOCH_SLOT;
    else {
        const uint32_t tgt = store.find(target_root);
        if (tgt == ATT_NO_BLOCK) v.status = ST_UNKNOWN_TARGET;
        else if ((v.block = store.find(block_root)) == ATT_NO_BLOCK) v.status = ST_UNKNOWN_BLOCK;
        else if (store.slot_of(v.block) > slot) v.status = ST_BLOCK_AFTER_SLOT;
        // get_ancestor(store, beacon_block_root, compute_start_slot_at_epoch(target.epoch)): the block's slot is <= data.slot
        // and the epoch is data.slot's, so the walk is at most SLOTS_PER_EPOCH parent steps
        else if (!(store.ancestor(v.block, target_epoch * slots_per_epoch) == store.handle(tgt))) v.status = ST_TARGET_NOT_ANCESTOR;
        else if (cur_slot < slot + 1) v.status = ST_SLOT_NOT_PAST;
    }
    return v;
}

// ------------------------------------------------------------------ the committee a row names (A.6, pe:727, pe:730)
// Three readings of one ladder.  get_indexed_attestation reads bits[i] for every committee position and asserts nothing
// about data.index: over bits in host memory surplus bits are ignored; resident bits are the union of exactly the committee's
// length.  process_attestation asserts both the index (pe:727) and the length (pe:730).
enum AttCommitteeReading { ATT_FC_HOST_BITS, ATT_FC_RESIDENT_BITS, ATT_STATE };
// the state's reading from the fork choice's exact one (the device plans the latter per group, k_att_plan): pe:727 sits
// behind "no table" and in front of the rest
PE_HD int32_t att_committee_state_status(int32_t resident_status, bool index_over)
{
    if (resident_status == ST_NO_TABLE) return ST_NO_TABLE;
    if (index_over) return ST_INDEX_RANGE;
    return resident_status;
}
// `size`: the committee's length where cp.exists
PE_HD int32_t att_committee_status(bool table_loaded, const CommitteePos& cp, uint32_t n_bits, uint32_t size,
                                   AttCommitteeReading reading)
{
    int32_t st = ST_OK;
    if (!table_loaded) st = ST_NO_TABLE;
    else if (!cp.exists) st = ST_INDEX_RANGE;
    else if (reading == ATT_FC_HOST_BITS ? n_bits < size : n_bits != size) st = ST_BITS_LENGTH;
    return reading == ATT_STATE ? att_committee_state_status(st, cp.index_over) : st;
}

// ------------------------------------------------------------------ is_valid_indexed_attestation (A.7)
// The signature verdict, then what the OR-ed bits say: members that overlap never verify (A.8), no bit is the empty list.
PE_HD int32_t att_indexed_status(bool sig_valid, bool overlap, uint32_t count)
{
    if (!sig_valid) return ST_BAD_SIGNATURE;
    if (overlap) return ST_BAD_SIGNATURE;
    if (count == 0) return ST_EMPTY;
    return ST_OK;
}

// ------------------------------------------------------------------ process_attestation (pe:724-730) + flag indices (A.9)
struct StateClock {  // what the asserts read of the state and the configuration
    uint64_t slot, cur_epoch, prev_epoch, slots_per_epoch, min_inclusion_delay, sqrt_spe;
};
PE_HD int32_t att_state_time_status(uint64_t slot, uint64_t target_epoch, const StateClock& c)
{
    if (target_epoch != c.prev_epoch && target_epoch != c.cur_epoch) return ST_EPOCH_TIME;                 // pe:724
    if (target_epoch != slot / c.slots_per_epoch) return ST_EPOCH_SLOT;                                     // pe:725
    if (!(slot + c.min_inclusion_delay <= c.slot && c.slot <= slot + c.slots_per_epoch)) return ST_INCLUSION;  // pe:726
    return ST_OK;
}
// which participation array the flags go to (pe:739-742): 0 current, 1 previous -- and whose justified checkpoint the source is
PE_HD uint32_t att_which(uint64_t target_epoch, uint64_t cur_epoch) { return target_epoch == cur_epoch ? 0u : 1u; }
PE_HD uint32_t att_flag_mask(uint64_t delay, uint64_t sqrt_spe, uint64_t slots_per_epoch, uint64_t min_inclusion_delay,
                             bool matching_target, bool matching_head)
{
    uint32_t mask = 0;
    if (delay <= sqrt_spe) mask |= TIMELY_SOURCE;
    if (matching_target && delay <= slots_per_epoch) mask |= TIMELY_TARGET;
    if (matching_head && delay == min_inclusion_delay) mask |= TIMELY_HEAD;
    return mask;
}
// `row` answers, each at most once and only when the ladder has come that far: committee_status() (the ATT_FC_RESIDENT_BITS
// reading) and index_over() of its committee, source_matches() (is_matching_source against the justified checkpoint of its
// epoch), matching_target() and matching_head() (get_block_root / get_block_root_at_slot of the state's chain).
struct StateVerdict {
    int32_t status;      // before A.7, which the caller asks next
    uint32_t flag_mask;
};
template <class RowView>
PE_HD StateVerdict att_state_status(const RowView& row, uint64_t slot, uint64_t target_epoch, const StateClock& c)
{
    StateVerdict v;
    v.flag_mask = 0;
    v.status = att_state_time_status(slot, target_epoch, c);
    if (v.status != ST_OK) return v;
    const int32_t resident_status = row.committee_status();
    v.status = att_committee_state_status(resident_status, row.index_over());
    if (v.status != ST_OK) return v;
    if (!row.source_matches()) { v.status = ST_SOURCE; return v; }  // assert is_matching_source
    const bool matching_target = row.matching_target();
    const bool matching_head = matching_target && row.matching_head();
    v.flag_mask = att_flag_mask(c.slot - slot, c.sqrt_spe, c.slots_per_epoch, c.min_inclusion_delay, matching_target, matching_head);
    return v;
}

}  // namespace posevo
