// The row rules of pos_evolution_amd/csrc/att_row.h compiled for the HOST by a plain C++ compiler, from the very header the
// engine's host paths and the gfx950 bodies include: tests/test_att_row_host.py holds them against Python integers.
#include "../../pos_evolution_amd/csrc/att_row.h"

using namespace posevo;

extern "C" {

int arh_bits_in_arena(uint32_t bits_offset, uint32_t n_bits, uint64_t arena_len)
{
    return att_bits_in_arena(bits_offset, n_bits, arena_len) ? 1 : 0;
}

// out = {position (meaningful where it exists), exists, index >= committees per slot}
void arh_committee_pos(uint32_t n_committees, uint64_t slots_per_epoch, uint64_t slot, uint64_t index, uint32_t out[3])
{
    const CommitteePos cp = att_committee_pos(n_committees, slots_per_epoch, slot, index);
    out[0] = cp.pos;
    out[1] = cp.exists ? 1 : 0;
    out[2] = cp.index_over ? 1 : 0;
}

}  // extern "C"
