// att_row.h -- where an attestation row's bits and committee lie: do the bits lie inside the arena, and which committee of the
// target epoch's table does (slot, index) name.  One text for the host paths (engine_attest.cpp, engine_slash.cpp, through
// engine_internal.h) and the device bodies (att_bodies.inc), so that the routes tests/test_gpu_att_rules.py compares cannot
// disagree here.  What a missing committee or an index beyond committees_per_slot means for the row's status, and in which
// order, is att_rules.h, over this header (the slasher keeps a ladder of its own).  Like the field headers it compiles under
// hipcc and under a plain host compiler (pe_hd.h).
#pragma once
#include <stdint.h>

#include "pe_hd.h"

namespace posevo {

// aggregation_bits of n_bits bits at byte bits_offset of an arena of arena_len bytes (n_bits beyond 2^31 - 1 are refused:
// word and byte counts of a row stay inside 32 bits everywhere behind this check)
PE_HD bool att_bits_in_arena(uint32_t bits_offset, uint32_t n_bits, uint64_t arena_len)
{
    return n_bits <= 0x7FFFFFFFu && (uint64_t)bits_offset + ((uint64_t)n_bits + 7) / 8 <= arena_len;
}

// get_beacon_committee's position (A.6) in a table of n_committees = committees_per_slot * SLOTS_PER_EPOCH committees:
// compute_committee(index = (slot % SLOTS_PER_EPOCH) * committees_per_slot + data.index, count = n_committees).
// on_attestation's get_beacon_committee asserts nothing about data.index itself -- only the position has to exist; pe:727
// (process_attestation) and pe_aggregate require data.index < committees_per_slot: index_over.  An index of 2^32 - 1 or
// more names no committee (n_committees is 32 bits wide) and is kept out of the sum, which would wrap.
struct CommitteePos {
    uint32_t pos;     // the position, where it exists
    bool exists;      // position < n_committees
    bool index_over;  // data.index >= committees_per_slot
};
PE_HD CommitteePos att_committee_pos(uint32_t n_committees, uint64_t slots_per_epoch, uint64_t slot, uint64_t index)
{
    const uint64_t cps = n_committees / slots_per_epoch;
    const uint64_t flat = index < 0xFFFFFFFFull ? (slot % slots_per_epoch) * cps + index : ~0ull;
    CommitteePos r;
    r.pos = (uint32_t)flat;
    r.exists = flat < n_committees;
    r.index_over = index >= cps;
    return r;
}

}  // namespace posevo
