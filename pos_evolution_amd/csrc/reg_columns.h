// reg_columns.h -- the registry's per-validator device arrays ("columns"): which there are, how wide a row is, which rows a
// validator nobody has written yet takes, and how much memory a column of n validators asks for.
//
// ONE table, REG_COLUMNS: a new per-validator array is one row of it, and with that row it is sized by its setter, grown by
// registry_grow, filled where fresh rows are filled and released with the handle (engine_internal.h: reg_ensure, reg_fill,
// reg_release walk the table; nothing else sizes a column).  A column belongs to a group: the columns one call sets together
// and, for the three that a handle may not hold at all, the unit that is held or not (engine_internal.h: reg_held).
//
// Pure arithmetic, no HIP: tests/test_reg_columns.py compiles this header with the host compiler alone.
#pragma once
#include <stdint.h>
#include <cstddef>

namespace posevo {

// Rows of a column of n validators: some kernels read four entries at a time (kernels.h: RemapArgs), so a column ends on a
// multiple of four rows and its fresh rows are filled through that multiple.
constexpr uint64_t reg_rows(uint64_t n) { return (n + 3) & ~uint64_t(3); }

// The allocation a column of n validators asks for: its padded rows, never less than one block of four rows nor than 64 bytes
// (an empty registry still has arrays a kernel may be handed).
constexpr uint64_t reg_column_bytes(uint64_t elem, uint64_t n)
{
    const uint64_t rows = reg_rows(n) < 4 ? 4 : reg_rows(n), bytes = elem * rows;
    return bytes < 64 ? 64 : bytes;
}

// registry_grow's capacity, in validators: what the columns were last grown to (never less than the registry they hold), doubled
// where the new size does not fit, so that 16 deposits per block do not reallocate per block; a multiple of four rows, and no
// more than the 2^32 rows a 32-bit validator index can name.
constexpr uint64_t reg_grown_capacity(uint64_t capacity, uint64_t n_old, uint64_t n_new)
{
    uint64_t cap = capacity > n_old ? capacity : n_old;
    if (n_new > capacity) cap = n_new > 2 * cap ? n_new : 2 * cap;
    cap = reg_rows(cap);
    return cap < 0x100000000ull ? cap : 0x100000000ull;
}

enum RegGroup : uint32_t {
    REG_JUSTIFIED = 1u << 0,      // pe_set_validators / pe_set_balances: what get_head weighs
    REG_VOTES = 1u << 1,          // the latest messages
    REG_VOTE_SLOT = 1u << 2,      // ... their slots: the vote-expiry variant only
    REG_PARTICIPATION = 1u << 3,  // current / previous_epoch_participation
    REG_VIEW = 1u << 4,           // the working-state view
    REG_EPOCHS = 1u << 5,         // pe_registry_set_epochs
    REG_BALANCES = 1u << 6,       // pe_state_set_balances
    REG_STATIC = 1u << 7,         // pe_registry_set_static
    REG_POINTS = 1u << 8,         // the pubkey table: where keys are loaded
    REG_POINTS30 = 1u << 9,       // ... in the accumulation's field form: where build_points30 has run
};
constexpr uint32_t REG_ALL_GROUPS = (1u << 10) - 1;
constexpr uint32_t REG_POINT_BYTES = 128;  // a row of the pubkey table (kernels.h: 4 * G1_ROW_WORDS)

// X(member of pe_engine, bytes per row, group, fill): fill = the byte every fresh row takes (a validator without balance,
// score, participation or latest message), -1 = the caller writes the rows (k_deposit_apply, the setters).
#define REG_COLUMNS(X)                                    \
    X(d_balance, 8, REG_JUSTIFIED, 0)                     \
    X(d_flags, 1, REG_JUSTIFIED, 0)                       \
    X(d_vote_key, 8, REG_VOTES, 0)                        \
    X(d_vote_block, 4, REG_VOTES, 0xFF)                   \
    X(d_vote_slot, 4, REG_VOTE_SLOT, 0)                   \
    X(d_part_cur, 1, REG_PARTICIPATION, 0)                \
    X(d_part_prev, 1, REG_PARTICIPATION, 0)               \
    X(d_sbalance, 8, REG_VIEW, -1)                        \
    X(d_sflags, 1, REG_VIEW, -1)                          \
    X(d_incr, 2, REG_VIEW, -1)                            \
    X(d_activation_epoch, 8, REG_EPOCHS, -1)              \
    X(d_exit_epoch, 8, REG_EPOCHS, -1)                    \
    X(d_rbalance, 8, REG_BALANCES, 0)                     \
    X(d_inactivity, 8, REG_BALANCES, 0)                   \
    X(d_withdrawable, 8, REG_BALANCES, -1)                \
    X(d_pubkey_leaf, 32, REG_STATIC, -1)                  \
    X(d_withdrawal_credentials, 32, REG_STATIC, -1)       \
    X(d_activation_eligibility, 8, REG_STATIC, -1)        \
    X(d_points, REG_POINT_BYTES, REG_POINTS, -1)          \
    X(d_points30, REG_POINT_BYTES, REG_POINTS30, -1)

struct RegColumn { const char* name; uint32_t elem; RegGroup group; int fill; };
#define REG_COLUMN_ROW(member, elem, group, fill) {#member, elem, group, fill},
constexpr RegColumn REG_COLUMN[] = {REG_COLUMNS(REG_COLUMN_ROW)};
#undef REG_COLUMN_ROW
constexpr size_t REG_N_COLUMNS = sizeof(REG_COLUMN) / sizeof(REG_COLUMN[0]);

}  // namespace posevo
