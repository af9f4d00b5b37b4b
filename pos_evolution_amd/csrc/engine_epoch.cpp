// engine_epoch.cpp -- the working-state view and the epoch boundary over the resident registry: the registry-wide functions
// of the reference that sit there and whose callers' text it holds.
//   pe_state_set_validators / _get  the view itself: effective balances and flags of the state being processed
//   pe_participation_set / _get / _rotate   current / previous_epoch_participation (pe:739-742), rotated at the boundary
//   pe_ffg_balances                 total active / previous-target / current-target balance (k_ffg_balances)
//   pe_registry_set_epochs / _get   Validator.activation_epoch / exit_epoch (pe:43-44), two u64 arrays in device memory
//   pe_active_set                   get_active_validator_indices(state, epoch) with its length (pe:467, pe:1234, pe:1267) and
//                                   get_total_active_balance (pe:1268): k_active_compact (shuffle_kernels.hip)
//   pe_state_refresh_activity       PE_VAL_ACTIVE / PE_VAL_ACTIVE_PREV of the working-state view from those epochs
//   pe_compute_proposers            compute_proposer_index (pe:604-618), once per seed: k_proposer_sample (shuffle_kernels.hip)
//   pe_effective_balance_updates    process_effective_balance_updates (pe:122-133): k_effective_balance_update (fc_kernels.hip)
// All read and write the working-state view (d_sbalance / d_sflags / d_incr) and leave the justified-checkpoint data get_head
// weighs (d_balance / d_flags) alone.  All are synchronous, single-GPU calls; inputs travel through the arena's pinned
// staging block, results through its pinned output block.
#include "engine_internal.h"

using namespace posevo;

namespace posevo {

void registry_epochs_drop(pe_engine* h)
{
    h->epochs_set = false;
    h->active_valid = false;  // the buffer stays: a shuffle in flight may still read it, and nothing rewrites it here
}

int materialise_state_view(pe_engine* h)
{
    if (h->state_view_set) return PE_OK;
    const uint64_t n = h->n_val;
    const size_t n4 = (n + 3) & ~size_t(3);
    HIP_TRY(h, h->d_sbalance.ensure(std::max<size_t>(64, n4 * 8)));
    HIP_TRY(h, h->d_sflags.ensure(std::max<size_t>(64, n4)));
    if (n) {
        HIP_TRY(h, hipMemcpyAsync(h->d_sbalance.p, h->d_balance.p, 8 * n, hipMemcpyDeviceToDevice, h->stream));
        launch_state_view_from_registry(h->stream, h->d_flags.as<uint8_t>(), h->d_balance.as<uint64_t>(),
                                        h->cfg.effective_balance_increment, n, h->d_sflags.as<uint8_t>(),
                                        h->d_incr.as<uint16_t>());
        HIP_TRY(h, hipGetLastError());
    }
    h->state_view_set = true;
    return PE_OK;
}

}  // namespace posevo

extern "C" {

int pe_participation_set(pe_engine* h, int which, const uint8_t* flags, uint64_t n)
{
    if (!h || !flags || n != h->n_val || (which != 0 && which != 1)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    DevBuf& b = which ? h->d_part_prev : h->d_part_cur;
    HIP_TRY(h, hipMemcpyAsync(b.p, flags, n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PE_OK;
}
int pe_participation_get(pe_engine* h, int which, uint8_t* out_flags, uint64_t n)
{
    if (!h || !out_flags || n != h->n_val || (which != 0 && which != 1)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    DevBuf& b = which ? h->d_part_prev : h->d_part_cur;
    HIP_TRY(h, hipMemcpyAsync(out_flags, b.p, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PE_OK;
}
int pe_participation_rotate(pe_engine* h)
{
    if (!h) return PE_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    std::swap(h->d_part_cur, h->d_part_prev);  // previous = current
    // on the state stream, behind the flag passes that still write the old arrays (and off the fork-choice stream)
    // The array that becomes "current" was "previous": its last readers and writers are the flag passes of earlier steps, on
    // this stream; synchronous readers on the engine's stream (pe_participation_get, pe_ffg_balances) complete before they
    // return.  So the memset needs no ordering against the engine's stream -- unless a flag pass had to be placed there
    // (state_stream_begin's fall-back when its fork event could not be recorded): then this rotation forks behind it.
    hipStream_t ss;
    if (h->state_work_on_main) {
        h->state_work_on_main = false;
        ss = state_stream_begin(h);
    } else {
        ss = state_stream_unordered(h);
    }
    if (h->n_val) HIP_TRY(h, hipMemsetAsync(h->d_part_cur.p, 0, (h->n_val + 3) & ~uint64_t(3), ss));  // current = 0
    return PE_OK;
}

int pe_state_set_validators(pe_engine* h, uint64_t n, const uint64_t* effective_balance, const uint8_t* flags)
{
    if (!h || (n && (!effective_balance || !flags))) return PE_ERR_INVALID_ARG;
    if (n != h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_state_set_validators: n differs from the registry size");
    PE_TRY(enter(h));
    std::vector<uint16_t> incr(n);
    const uint64_t inc = h->cfg.effective_balance_increment;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t q = effective_balance[i] / inc;
        if (q > 0xFFFF) return fail(h, PE_ERR_INVALID_ARG, "effective_balance / increment exceeds 65535");
        incr[i] = (uint16_t)q;
    }
    const size_t n4 = (n + 3) & ~size_t(3);
    HIP_TRY(h, h->d_sbalance.ensure(std::max<size_t>(64, n4 * 8)));
    HIP_TRY(h, h->d_sflags.ensure(std::max<size_t>(64, n4)));
    HIP_TRY(h, hipMemcpyAsync(h->d_sbalance.p, effective_balance, n * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_sflags.p, flags, n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_incr.p, incr.data(), n * 2, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->state_view_set = true;
    return PE_OK;
}

// Read-back of the working-state view (checkpoint / resume): *out_is_set = 0 while the view still mirrors the registry.
int pe_state_get_validators(pe_engine* h, uint64_t n, uint64_t* out_effective_balance, uint8_t* out_flags, int* out_is_set)
{
    if (!h || !out_is_set || (n && (!out_effective_balance || !out_flags))) return PE_ERR_INVALID_ARG;
    if (n != h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_state_get_validators: n differs from the registry size");
    PE_TRY(enter(h));
    *out_is_set = h->state_view_set ? 1 : 0;
    if (n && h->d_sbalance.p && h->d_sflags.p) {
        HIP_TRY(h, hipMemcpyAsync(out_effective_balance, h->d_sbalance.p, n * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(out_flags, h->d_sflags.p, n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return PE_OK;
}

int pe_ffg_balances(pe_engine* h, uint64_t out[3])
{
    if (!h || !out) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    OutBlock ob(h);
    const size_t off = ob.alloc(8ull * 3 * 256);
    PE_TRY(ob.ensure());
    uint32_t blocks = 0;
    if (h->n_val) {
        blocks = launch_ffg_balances(h->stream, h->d_sbalance.as<uint64_t>(), h->d_sflags.as<uint8_t>(),
                                     h->d_part_cur.as<uint8_t>(), h->d_part_prev.as<uint8_t>(), h->n_val,
                                     ob.dev<uint64_t>(off));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, ob.download());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    uint64_t s[3] = {0, 0, 0};
    const uint64_t* p = ob.host<uint64_t>(off);
    for (uint32_t b = 0; b < blocks; ++b)
        for (int k = 0; k < 3; ++k) s[k] += p[3 * b + k];
    for (int k = 0; k < 3; ++k) out[k] = std::max<uint64_t>(h->cfg.effective_balance_increment, s[k]);  // get_total_balance
    return PE_OK;
}

int pe_registry_set_epochs(pe_engine* h, uint64_t n, const uint64_t* activation_epoch, const uint64_t* exit_epoch)
{
    if (!h || (n && (!activation_epoch || !exit_epoch))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (n != h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_registry_set_epochs: n differs from the registry size");
    HIP_TRY(h, h->d_activation_epoch.ensure(std::max<size_t>(64, 8 * n)));
    HIP_TRY(h, h->d_exit_epoch.ensure(std::max<size_t>(64, 8 * n)));
    if (n) {
        HIP_TRY(h, hipMemcpyAsync(h->d_activation_epoch.p, activation_epoch, 8 * n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_exit_epoch.p, exit_epoch, 8 * n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->epochs_set = true;
    h->active_valid = false;  // a list compacted from the previous epochs is not a list of these
    return PE_OK;
}

int pe_registry_get_epochs(pe_engine* h, uint64_t n, uint64_t* out_activation_epoch, uint64_t* out_exit_epoch, int* out_is_set)
{
    if (!h || !out_is_set || (n && (!out_activation_epoch || !out_exit_epoch))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (n != h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_registry_get_epochs: n differs from the registry size");
    *out_is_set = h->epochs_set ? 1 : 0;
    if (n && h->epochs_set) {
        HIP_TRY(h, hipMemcpyAsync(out_activation_epoch, h->d_activation_epoch.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(out_exit_epoch, h->d_exit_epoch.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return PE_OK;
}

int pe_active_set(pe_engine* h, uint64_t epoch, uint32_t* out_n_active, uint64_t* out_total_balance, uint32_t* out_indices)
{
    if (!h || !out_n_active || !out_total_balance) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready())
        return fail(h, PE_ERR_STATE, "pe_active_set: the handle exchanges with other ranks (pe_dist_init); "
                                     "a sharded registry is not supported");
    if (!h->epochs_set) return fail(h, PE_ERR_STATE, "pe_active_set: no registry epochs (pe_registry_set_epochs first)");
    const uint64_t n = h->n_val;
    const uint64_t inc = h->cfg.effective_balance_increment;
    if (n && h->d_sbalance.cap < 8 * n)
        return fail(h, PE_ERR_STATE, "pe_active_set: the working-state view does not cover the registry");
    if (n == 0) {
        h->active_valid = true;
        h->active_epoch = epoch;
        h->active_n = 0;
        *out_n_active = 0;
        *out_total_balance = inc;
        return PE_OK;
    }
    const size_t list_bytes = std::max<size_t>(64, 4 * n), wg_bytes = std::max<size_t>(64, active_scratch_bytes(n));
    if (h->active_read_pending && (list_bytes > h->d_active.cap || wg_bytes > h->d_active_wg.cap)) {
        HIP_TRY(h, hipEventSynchronize(h->ev_active_read));  // the list is about to be freed, not merely rewritten
        h->active_read_pending = false;
    }
    HIP_TRY(h, h->d_active.ensure(list_bytes));
    HIP_TRY(h, h->d_active_wg.ensure(wg_bytes));
    OutBlock ob(h);
    const size_t off_tot = ob.alloc(sizeof(ActiveTotals));
    const size_t off_idx = out_indices ? ob.alloc(4 * n) : 0;
    PE_TRY(ob.ensure());
    h->active_valid = false;
    if (h->active_read_pending) {  // a shuffle in flight still reads the list: the rewrite queues behind it on the device
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_active_read, 0));
        h->active_read_pending = false;
    }
    launch_active_compact(h->stream, h->d_activation_epoch.as<uint64_t>(), h->d_exit_epoch.as<uint64_t>(), epoch,
                          h->d_sbalance.as<uint64_t>(), n, h->d_active_wg.p, h->d_active.as<uint32_t>(),
                          ob.dev<ActiveTotals>(off_tot));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, ob.download(off_tot, sizeof(ActiveTotals)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const ActiveTotals tot = *ob.host<ActiveTotals>(off_tot);
    if (tot.n_active > n) return fail(h, PE_ERR_NO_DEVICE, "k_active_scan returned more active validators than the registry holds");
    if (out_indices && tot.n_active) {  // straight into the pinned block, and only the list's own length
        HIP_TRY(h, hipMemcpyAsync(ob.host<uint32_t>(off_idx), h->d_active.p, 4ull * tot.n_active, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        memcpy(out_indices, ob.host<uint32_t>(off_idx), 4ull * tot.n_active);
    }
    h->active_valid = true;
    h->active_epoch = epoch;
    h->active_n = tot.n_active;
    *out_n_active = tot.n_active;
    *out_total_balance = std::max<uint64_t>(inc, tot.balance);  // get_total_balance's floor (Appendix A.1), as pe_ffg_balances
    return PE_OK;
}

int pe_state_refresh_activity(pe_engine* h, uint64_t current_epoch)
{
    if (!h) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready())
        return fail(h, PE_ERR_STATE, "pe_state_refresh_activity: the handle exchanges with other ranks (pe_dist_init); "
                                     "a sharded registry is not supported");
    if (!h->epochs_set) return fail(h, PE_ERR_STATE, "pe_state_refresh_activity: no registry epochs (pe_registry_set_epochs first)");
    PE_TRY(materialise_state_view(h));
    const uint64_t previous_epoch = std::max<uint64_t>(current_epoch, 1) - 1;  // get_previous_epoch's clamp at GENESIS_EPOCH
    launch_activity_flags(h->stream, h->d_activation_epoch.as<uint64_t>(), h->d_exit_epoch.as<uint64_t>(), current_epoch,
                          previous_epoch, h->n_val, h->d_sflags.as<uint8_t>());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return PE_OK;
}

int pe_compute_proposers(pe_engine* h, const uint8_t* seeds32, uint32_t n_seeds, const uint32_t* active_indices,
                         uint32_t n_active, uint32_t shuffle_round_count, uint64_t max_effective_balance,
                         uint32_t max_tries, uint32_t* out_proposers, uint32_t* out_tries)
{
    if (!h || (n_seeds && (!seeds32 || !out_proposers))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready())
        return fail(h, PE_ERR_STATE, "pe_compute_proposers: the handle exchanges with other ranks (pe_dist_init); "
                                     "sampling over a sharded registry is not supported");
    if (shuffle_round_count > 255) return fail(h, PE_ERR_INVALID_ARG, "shuffle_round_count is a uint8 in the spec");
    PE_TRY(validate_active_set(h, active_indices, n_active));
    if (n_active == 0) return fail(h, PE_ERR_INVALID_ARG, "pe_compute_proposers: the active set is empty (pe:608)");
    if (max_tries == 0) max_tries = 4096;
    if (n_seeds == 0) return PE_OK;
    const bool staged = active_indices != nullptr && active_indices != PE_ACTIVE_RESIDENT;  // a host list: copied and uploaded
    Stage st(h);
    PE_TRY(st.reserve(32ull * n_seeds + (staged ? 4ull * n_active : 0) + 1024));
    const size_t off_seed = st.alloc(32ull * n_seeds);
    const size_t off_idx = st.alloc(staged ? 4ull * n_active + 4 : 4);
    uint32_t* sw = st.host<uint32_t>(off_seed);
    for (uint64_t i = 0; i < 8ull * n_seeds; ++i) {  // the kernels take a seed as 8 big-endian words
        const uint8_t* b = seeds32 + 4 * i;
        sw[i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
    }
    if (staged) memcpy(st.host<uint32_t>(off_idx), active_indices, 4ull * n_active);
    OutBlock ob(h);
    const size_t off_prop = ob.alloc(4ull * n_seeds);
    const size_t off_tries = ob.alloc(4ull * n_seeds);
    PE_TRY(ob.ensure());
    HIP_TRY(h, st.upload());
    launch_proposer_sample(h->stream, st.dev<uint32_t>(off_seed), n_seeds, n_active, shuffle_round_count,
                           active_list_dev(h, active_indices, st.dev<uint32_t>(off_idx)), h->d_sbalance.as<uint64_t>(),
                           max_effective_balance, max_tries, ob.dev<uint32_t>(off_prop), ob.dev<uint32_t>(off_tries));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, ob.download());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    memcpy(out_proposers, ob.host<uint32_t>(off_prop), 4ull * n_seeds);
    if (out_tries) memcpy(out_tries, ob.host<uint32_t>(off_tries), 4ull * n_seeds);
    return PE_OK;
}

int pe_effective_balance_updates(pe_engine* h, uint64_t n, const uint64_t* balances, uint64_t max_effective_balance,
                                 uint64_t hysteresis_quotient, uint64_t downward_multiplier, uint64_t upward_multiplier,
                                 uint64_t* out_n_changed, uint64_t* out_effective_balance)
{
    if (!h || !out_n_changed || (n && !balances)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready())
        return fail(h, PE_ERR_STATE, "pe_effective_balance_updates: the handle exchanges with other ranks (pe_dist_init); "
                                     "a sharded registry is not supported");
    if (n != h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_effective_balance_updates: n differs from the registry size");
    const uint64_t inc = h->cfg.effective_balance_increment;
    if (inc == 0 || hysteresis_quotient == 0)
        return fail(h, PE_ERR_INVALID_ARG, "pe_effective_balance_updates: increment and hysteresis quotient must be positive");
    if (max_effective_balance / inc > 0xFFFF) return fail(h, PE_ERR_INVALID_ARG, "max_effective_balance / increment exceeds 65535");
    const uint64_t step = inc / hysteresis_quotient;  // HYSTERESIS_INCREMENT (pe:126)
    uint64_t down = 0, up = 0;
    if (__builtin_mul_overflow(step, downward_multiplier, &down) || __builtin_mul_overflow(step, upward_multiplier, &up))
        return fail(h, PE_ERR_INVALID_ARG, "pe_effective_balance_updates: a hysteresis threshold exceeds 64 bits");
    *out_n_changed = 0;
    if (n == 0) return PE_OK;
    Stage st(h);
    PE_TRY(st.reserve(8ull * n + 1024));
    const size_t off_bal = st.alloc(8ull * n);
    memcpy(st.host<uint64_t>(off_bal), balances, 8ull * n);
    OutBlock ob(h);
    const size_t off_cnt = ob.alloc(8);
    const size_t off_eff = out_effective_balance ? ob.alloc(8ull * n) : 0;
    PE_TRY(ob.ensure());
    PE_TRY(materialise_state_view(h));  // the view still mirrors the registry: a view of its own first, flags included
    HIP_TRY(h, st.upload());
    HIP_TRY(h, hipMemsetAsync(ob.dev<uint64_t>(off_cnt), 0, 8, h->stream));
    launch_effective_balance_update(h->stream, st.dev<uint64_t>(off_bal), h->d_sbalance.as<uint64_t>(),
                                    h->d_incr.as<uint16_t>(), n, inc, down, up, max_effective_balance,
                                    ob.dev<uint64_t>(off_cnt));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, ob.download(off_cnt, 8));
    if (out_effective_balance)  // straight into the pinned block: a pageable read-back of 8 MB is staged in small pieces
        HIP_TRY(h, hipMemcpyAsync(ob.host<uint64_t>(off_eff), h->d_sbalance.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *out_n_changed = *ob.host<uint64_t>(off_cnt);
    if (out_effective_balance) memcpy(out_effective_balance, ob.host<uint64_t>(off_eff), 8ull * n);
    return PE_OK;
}

}  // extern "C"
