// The status rules of pos_evolution_amd/csrc/att_rules.h compiled for the HOST by a plain C++ compiler, from the very header
// the engine's host routes and the gfx950 validators include: tests/test_att_rules_host.py drives the boundary matrix of
// tests/att_rules_cases.py through them and holds every row to tests/att_rules_model.py.  The store is three plain arrays
// (parent index, slot, root id); a root is a 64-bit id here.  Nothing below decides a status: the adapters look things up,
// the two entry points ask the rules in the order the engine's routes ask them.
#include "../../pos_evolution_amd/csrc/att_rules.h"

using namespace posevo;

namespace {

struct ArrayStore {
    uint32_t n;
    const uint32_t* parent;  // ATT_NO_BLOCK for the first block
    const uint64_t* slot;
    const uint64_t* root;
    uint32_t find(const uint64_t& r) const
    {
        for (uint32_t i = 0; i < n; ++i)
            if (root[i] == r) return i;
        return ATT_NO_BLOCK;
    }
    uint32_t handle(uint32_t idx) const { return idx; }
    uint64_t slot_of(uint32_t idx) const { return slot[idx]; }
    uint32_t ancestor(uint32_t idx, uint64_t s) const  // get_ancestor (A.2)
    {
        while (slot[idx] > s && parent[idx] != ATT_NO_BLOCK) idx = parent[idx];
        return idx;
    }
};

// one committee table of n_committees committees of `size` members each, loaded or not
struct Committees {
    int loaded;
    uint32_t n_committees, size;
    uint64_t slots_per_epoch;
    int32_t status(uint64_t slot, uint64_t index, uint32_t n_bits, AttCommitteeReading reading, bool* index_over) const
    {
        const CommitteePos cp = loaded ? att_committee_pos(n_committees, slots_per_epoch, slot, index) : CommitteePos{0, false, false};
        *index_over = cp.index_over;
        return att_committee_status(loaded != 0, cp, n_bits, size, reading);
    }
};

struct StateRow {
    const ArrayStore& store;
    const Committees& com;
    uint32_t tip;
    uint64_t slot, index, target_epoch, target_root, block_root;
    uint32_t n_bits;
    bool source_ok;
    mutable bool over;
    int32_t committee_status() const { return com.status(slot, index, n_bits, ATT_FC_RESIDENT_BITS, &over); }
    bool index_over() const { return over; }
    bool source_matches() const { return source_ok; }
    bool matching_target() const { return store.root[store.ancestor(tip, target_epoch * com.slots_per_epoch)] == target_root; }
    bool matching_head() const { return store.root[store.ancestor(tip, slot)] == block_root; }
};

}  // namespace

extern "C" {

// row = {slot, index, target_epoch, target_root, block_root, n_bits, from_block, sig_valid, overlap, count}
// clock = {cur_slot, cur_epoch, prev_epoch, slots_per_epoch}; table = {loaded, n_committees, size}; reading: 0 host bits, 1 resident
int32_t arl_fork_choice(uint32_t n_blocks, const uint32_t* parent, const uint64_t* slot, const uint64_t* root, const uint64_t row[10],
                        const uint64_t clock[4], const uint32_t table[3], int reading, uint32_t* block_out)
{
    const ArrayStore store{n_blocks, parent, slot, root};
    const FcVerdict v = att_fork_choice_status(store, row[6] != 0, row[0], row[2], row[3], row[4], clock[0], clock[1], clock[2], clock[3]);
    *block_out = v.block;
    int32_t st = v.status;
    bool over;
    const Committees com{(int)table[0], table[1], table[2], clock[3]};
    if (st == ST_OK) st = com.status(row[0], row[1], (uint32_t)row[5], reading ? ATT_FC_RESIDENT_BITS : ATT_FC_HOST_BITS, &over);
    if (st == ST_OK) st = att_indexed_status(row[7] != 0, row[8] != 0, (uint32_t)row[9]);
    return st;
}

// clock = {state.slot, cur_epoch, prev_epoch, slots_per_epoch, min_inclusion_delay, sqrt(slots_per_epoch)}
// out = {status of the ladder before A.7, status, flag mask, which}
void arl_state(uint32_t n_blocks, const uint32_t* parent, const uint64_t* slot, const uint64_t* root, uint32_t tip, const uint64_t row[10],
               int source_matches, const uint64_t clock[6], const uint32_t table[3], int32_t out[4])
{
    const ArrayStore store{n_blocks, parent, slot, root};
    const Committees com{(int)table[0], table[1], table[2], clock[3]};
    const StateClock c{clock[0], clock[1], clock[2], clock[3], clock[4], clock[5]};
    const StateRow view{store, com, tip, row[0], row[1], row[2], row[3], row[4], (uint32_t)row[5], source_matches != 0, false};
    const StateVerdict v = att_state_status(view, row[0], row[2], c);
    out[0] = v.status;
    out[1] = v.status == ST_OK ? att_indexed_status(row[7] != 0, row[8] != 0, (uint32_t)row[9]) : v.status;
    out[2] = (int32_t)v.flag_mask;
    out[3] = (int32_t)att_which(row[2], clock[1]);
}

int32_t arl_indexed_status(int sig_valid, int overlap, uint32_t count) { return att_indexed_status(sig_valid != 0, overlap != 0, count); }

uint32_t arl_flag_mask(uint64_t delay, uint64_t sqrt_spe, uint64_t slots_per_epoch, uint64_t min_delay, int matching_target, int matching_head)
{
    return att_flag_mask(delay, sqrt_spe, slots_per_epoch, min_delay, matching_target != 0, matching_head != 0);
}

// the constants, in the order of include/posevo.h's pe_att_status
void arl_status_values(int32_t out[15])
{
    const int32_t v[15] = {ST_OK, ST_EPOCH_TIME, ST_EPOCH_SLOT, ST_UNKNOWN_TARGET, ST_UNKNOWN_BLOCK, ST_BLOCK_AFTER_SLOT,
                           ST_TARGET_NOT_ANCESTOR, ST_SLOT_NOT_PAST, ST_NO_TABLE, ST_INDEX_RANGE, ST_BITS_LENGTH, ST_EMPTY,
                           ST_BAD_SIGNATURE, ST_INCLUSION, ST_SOURCE};
    for (int i = 0; i < 15; ++i) out[i] = v[i];
}

}  // extern "C"
