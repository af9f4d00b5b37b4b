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
//   pe_state_set_balances / _get    state.balances, state.inactivity_scores (pe:112, pe:368-369) and Validator.withdrawable_epoch
//                                   (pe:45): three u64 arrays in device memory
//   pe_rewards_params_default       the constants of the two functions below
//   pe_rewards_and_penalties        process_inactivity_updates and process_rewards_and_penalties (Altair; restated in
//                                   tests/rewards_model.py) over those arrays: k_reward_sums, a host step, k_reward_apply
//                                   (reward_kernels.hip; the rule per validator is reward_row.h)
//   pe_registry_params_default      the constants of the function below
//   pe_registry_updates             process_registry_updates (restated in tests/registry_updates_model.py) over the resident
//                                   epochs: k_registry_census, a host step, the selection of the activation queue's head
//                                   (k_registry_select, k_registry_ties), k_registry_apply (registry_kernels.hip; the rule
//                                   per validator is registry_row.h)
//   pe_process_slashings            process_slashings over the resident balances: k_ffg_balances' total, k_slashings_census,
//                                   a host step, k_slashings_apply
//   pe_effective_balance_updates    process_effective_balance_updates (pe:122-133): k_effective_balance_update (fc_kernels.hip),
//                                   over the caller's balances or the resident ones (PE_BALANCES_RESIDENT)
// All read and write the working-state view (d_sbalance / d_sflags / d_incr) and leave the justified-checkpoint data get_head
// weighs (d_balance / d_flags) alone.  All are synchronous, single-GPU calls; inputs travel through the arena's pinned
// staging block, results through its pinned output block.
#include "engine_internal.h"
#include "registry_row.h"
#include "reward_row.h"

using namespace posevo;

namespace posevo {

void registry_epochs_drop(pe_engine* h)
{
    h->epochs_set = false;
    h->active_valid = false;  // the buffer stays: a shuffle in flight may still read it, and nothing rewrites it here
}

void resident_balances_drop(pe_engine* h) { h->balances_set = false; }

int materialise_state_view(pe_engine* h)
{
    if (h->state_view_set) return PE_OK;
    const uint64_t n = h->n_val;
    HIP_TRY(h, reg_ensure(h, REG_VIEW, n, /*keep=*/false));  // overwritten below
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
    std::vector<uint16_t> incr;
    PE_TRY(balance_increments(h, effective_balance, n, incr));
    HIP_TRY(h, reg_ensure(h, REG_VIEW, n, /*keep=*/false));  // overwritten below
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
    HIP_TRY(h, reg_ensure(h, REG_EPOCHS, n, /*keep=*/false));
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
    for (uint32_t i = 0; i < n_seeds; ++i) be32_words(seeds32 + 32ull * i, sw + 8ull * i);
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

int pe_state_set_balances(pe_engine* h, uint64_t n, const uint64_t* balances, const uint64_t* inactivity_scores,
                          const uint64_t* withdrawable_epoch)
{
    if (!h || (n && !balances)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (n != h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_state_set_balances: n differs from the registry size");
    HIP_TRY(h, reg_ensure(h, REG_BALANCES, n, /*keep=*/false, &h->balances_set));
    if (n) {
        HIP_TRY(h, hipMemcpyAsync(h->d_rbalance.p, balances, 8 * n, hipMemcpyHostToDevice, h->stream));
        if (inactivity_scores)
            HIP_TRY(h, hipMemcpyAsync(h->d_inactivity.p, inactivity_scores, 8 * n, hipMemcpyHostToDevice, h->stream));
        else
            HIP_TRY(h, hipMemsetAsync(h->d_inactivity.p, 0, 8 * n, h->stream));
        if (withdrawable_epoch)
            HIP_TRY(h, hipMemcpyAsync(h->d_withdrawable.p, withdrawable_epoch, 8 * n, hipMemcpyHostToDevice, h->stream));
        else
            HIP_TRY(h, hipMemsetAsync(h->d_withdrawable.p, 0xFF, 8 * n, h->stream));  // FAR_FUTURE_EPOCH = 2^64 - 1
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->balances_set = true;
    return PE_OK;
}

int pe_state_get_balances(pe_engine* h, uint64_t n, uint64_t* out_balances, uint64_t* out_inactivity_scores,
                          uint64_t* out_withdrawable_epoch, int* out_is_set)
{
    if (!h) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (n != h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_state_get_balances: n differs from the registry size");
    if (out_is_set) *out_is_set = h->balances_set ? 1 : 0;
    if (n && h->balances_set) {
        if (out_balances) HIP_TRY(h, hipMemcpyAsync(out_balances, h->d_rbalance.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
        if (out_inactivity_scores)
            HIP_TRY(h, hipMemcpyAsync(out_inactivity_scores, h->d_inactivity.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
        if (out_withdrawable_epoch)
            HIP_TRY(h, hipMemcpyAsync(out_withdrawable_epoch, h->d_withdrawable.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return PE_OK;
}

void pe_rewards_params_default(pe_rewards_params* out)
{
    if (!out) return;
    out->base_reward_factor = 64;
    out->inactivity_score_bias = 4;
    out->inactivity_score_recovery_rate = 16;
    out->inactivity_penalty_quotient = 1ull << 24;  // INACTIVITY_PENALTY_QUOTIENT_BELLATRIX; Altair's own is 3 * 2^24
    out->min_epochs_to_inactivity_penalty = 4;
}

int pe_rewards_and_penalties(pe_engine* h, uint64_t current_epoch, uint64_t finalized_epoch, const pe_rewards_params* params,
                             uint32_t which, pe_rewards_stats* out_stats)
{
    if (!h || !params) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready())
        return fail(h, PE_ERR_STATE, "pe_rewards_and_penalties: the handle exchanges with other ranks (pe_dist_init); "
                                     "a sharded registry is not supported");
    if (which == 0 || (which & ~(uint32_t)(PE_REWARDS_INACTIVITY | PE_REWARDS_DELTAS)))
        return fail(h, PE_ERR_INVALID_ARG, "pe_rewards_and_penalties: which must be PE_REWARDS_INACTIVITY, PE_REWARDS_DELTAS or both");
    if (!h->balances_set)
        return fail(h, PE_ERR_STATE, "pe_rewards_and_penalties: no resident balances (pe_state_set_balances first)");
    const uint64_t inc = h->cfg.effective_balance_increment;
    const uint64_t bias = params->inactivity_score_bias;
    uint64_t inactivity_divisor = 0;
    if (inc == 0 || __builtin_mul_overflow(bias, params->inactivity_penalty_quotient, &inactivity_divisor) || inactivity_divisor == 0)
        return fail(h, PE_ERR_INVALID_ARG, "pe_rewards_and_penalties: increment and inactivity_score_bias * "
                                           "inactivity_penalty_quotient must be positive and fit 64 bits");
    pe_rewards_stats stats;
    memset(&stats, 0, sizeof stats);
    if (current_epoch == 0) {  // both functions return at GENESIS_EPOCH
        if (out_stats) *out_stats = stats;
        return PE_OK;
    }
    const uint64_t previous_epoch = current_epoch - 1;  // get_previous_epoch: current_epoch >= 1 here
    if (finalized_epoch > previous_epoch)
        return fail(h, PE_ERR_INVALID_ARG, "pe_rewards_and_penalties: finalized_epoch lies after the previous epoch");
    const bool in_leak = previous_epoch - finalized_epoch > params->min_epochs_to_inactivity_penalty;
    const uint64_t n = h->n_val;
    OutBlock ob(h);
    const size_t off_sums = ob.alloc(8ull * REWARD_SUMS_Q * REWARD_SUMS_MAX_WG);
    const size_t off_apply = ob.alloc(8ull * REWARD_APPLY_Q * REWARD_APPLY_MAX_WG);
    PE_TRY(ob.ensure());
    PE_TRY(materialise_state_view(h));  // the view still mirrors the registry: a view of its own first, as the balance update does

    // ---- first pass: what the rule divides by, and the maxima its products are bounded with
    uint64_t sums[REWARD_SUMS_Q] = {0, 0, 0, 0, 0, 0, 0};
    if (n) {
        const uint32_t blocks = launch_reward_sums(h->stream, h->d_sbalance.as<uint64_t>(), h->d_sflags.as<uint8_t>(),
                                                   h->d_part_prev.as<uint8_t>(), h->d_inactivity.as<uint64_t>(),
                                                   h->d_withdrawable.as<uint64_t>(), n, previous_epoch + 1,
                                                   ob.dev<uint64_t>(off_sums));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, ob.download(off_sums, 8ull * REWARD_SUMS_Q * blocks));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const uint64_t* p = ob.host<uint64_t>(off_sums);
        for (uint32_t b = 0; b < blocks; ++b)
            for (int q = 0; q < REWARD_SUMS_Q; ++q) {
                const uint64_t x = p[(size_t)REWARD_SUMS_Q * b + q];
                sums[q] = q < 5 ? sums[q] + x : std::max(sums[q], x);
            }
    }
    const uint64_t total_active = std::max(inc, sums[0]);  // get_total_balance's floor (Appendix A.1), as pe_ffg_balances
    const uint64_t max_eff = sums[5], max_score = sums[6];
    stats.total_active_balance = total_active;
    for (int f = 0; f < 3; ++f) stats.unslashed_balance[f] = std::max(inc, sums[1 + f]);
    stats.n_eligible = sums[4];
    stats.in_leak = in_leak ? 1 : 0;

    // ---- host step (reward_row.h): the scalars, and every place the reference's uint64 would overflow -- before anything is written
    RewardScalars S;
    memset(&S, 0, sizeof S);
    static const char* const overflow_of[] = {"", "increment * base_reward_factor", "active increments * WEIGHT_DENOMINATOR",
                                              "base_reward * weight * unslashed increments", "inactivity score + bias",
                                              "effective_balance * inactivity score"};
    const int over = reward_scalars_make(inc, params->base_reward_factor, bias, params->inactivity_score_recovery_rate,
                                         inactivity_divisor, total_active, stats.unslashed_balance, max_eff, max_score,
                                         previous_epoch, in_leak, which, &S);
    if (over)
        return fail(h, PE_ERR_INVALID_ARG, std::string("pe_rewards_and_penalties: ") + overflow_of[over] + " can exceed 64 bits");

    // ---- second pass: the rule per validator
    if (n) {
        const uint32_t blocks = launch_reward_apply(h->stream, S, h->d_sbalance.as<uint64_t>(), h->d_sflags.as<uint8_t>(),
                                                    h->d_part_prev.as<uint8_t>(), h->d_withdrawable.as<uint64_t>(), n,
                                                    h->d_rbalance.as<uint64_t>(), h->d_inactivity.as<uint64_t>(),
                                                    ob.dev<uint64_t>(off_apply));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, ob.download(off_apply, 8ull * REWARD_APPLY_Q * blocks));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const uint64_t* p = ob.host<uint64_t>(off_apply);
        for (uint32_t b = 0; b < blocks; ++b) {
            stats.rewards += p[(size_t)REWARD_APPLY_Q * b + 0];
            stats.penalties += p[(size_t)REWARD_APPLY_Q * b + 1];
            stats.n_saturated += p[(size_t)REWARD_APPLY_Q * b + 2];
        }
    }
    if (out_stats) *out_stats = stats;
    return PE_OK;
}

void pe_registry_params_default(pe_registry_params* out)
{
    if (!out) return;
    out->max_effective_balance = 32000000000ull;
    out->ejection_balance = 16000000000ull;
    out->max_seed_lookahead = 4;
    out->min_validator_withdrawability_delay = 256;
    out->min_per_epoch_churn_limit = 4;
    out->churn_limit_quotient = 65536;
    out->max_per_epoch_activation_churn_limit = 0;  // none: the limit of the forks before Deneb (Deneb: 8)
}

int pe_registry_updates(pe_engine* h, uint64_t current_epoch, uint64_t finalized_epoch, const pe_registry_params* params,
                        pe_registry_stats* out_stats)
{
    if (!h || !params) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready())
        return fail(h, PE_ERR_STATE, "pe_registry_updates: the handle exchanges with other ranks (pe_dist_init); "
                                     "a sharded registry is not supported");
    if (!h->epochs_set) return fail(h, PE_ERR_STATE, "pe_registry_updates: no registry epochs (pe_registry_set_epochs first)");
    if (!h->balances_set)
        return fail(h, PE_ERR_STATE, "pe_registry_updates: no resident withdrawable epochs (pe_state_set_balances first)");
    if (!h->static_set)
        return fail(h, PE_ERR_STATE, "pe_registry_updates: no resident eligibility epochs (pe_registry_set_static first)");
    const uint64_t n = h->n_val;
    if (n && h->d_sbalance.cap < 8 * n)
        return fail(h, PE_ERR_STATE, "pe_registry_updates: the working-state view does not cover the registry");
    typedef unsigned __int128 u128;
    const u128 far = (u128)REGISTRY_FAR_FUTURE_EPOCH;
    if (params->churn_limit_quotient == 0) return fail(h, PE_ERR_INVALID_ARG, "pe_registry_updates: churn_limit_quotient is 0");
    const u128 activation_wide = (u128)current_epoch + 1 + params->max_seed_lookahead;
    if (activation_wide >= far)
        return fail(h, PE_ERR_INVALID_ARG, "pe_registry_updates: current_epoch + 1 + max_seed_lookahead reaches FAR_FUTURE_EPOCH");
    const uint64_t activation_exit_epoch = (uint64_t)activation_wide;

    const uint32_t n_wg = (uint32_t)((n + REGISTRY_WG - 1) / REGISTRY_WG);
    HIP_TRY(h, h->d_registry_wg.ensure(std::max<size_t>(64, registry_scratch_bytes(n))));
    OutBlock ob(h);
    const size_t off_census = ob.alloc(sizeof(RegistryTotals));
    const size_t off_ties = ob.alloc(sizeof(RegistryTotals));
    const size_t off_hist = ob.alloc(8 * 256 * sizeof(uint32_t));  // one histogram per byte of an epoch
    const size_t off_activated = ob.alloc(std::max<size_t>(4, 4ull * n_wg));
    PE_TRY(ob.ensure());
    uint64_t* const d_elig = h->d_activation_eligibility.as<uint64_t>();
    uint64_t* const d_act = h->d_activation_epoch.as<uint64_t>();
    uint64_t* const d_exit = h->d_exit_epoch.as<uint64_t>();

    // ---- census (read-only): the counts, the exit queue's end, the ejected validators' offsets
    RegistryTotals tot;
    memset(&tot, 0, sizeof tot);
    if (n) {
        launch_registry_census(h->stream, d_elig, d_act, d_exit, h->d_sbalance.as<uint64_t>(), n, current_epoch, finalized_epoch,
                               params->max_effective_balance, params->ejection_balance, h->d_registry_wg.p,
                               ob.dev<RegistryTotals>(off_census));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, ob.download(off_census, sizeof(RegistryTotals)));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        tot = *ob.host<RegistryTotals>(off_census);
        if (tot.n_active > n || tot.n_marked > n || tot.n_queue > n || tot.n_counted > n || tot.n_at_max > n)
            return fail(h, PE_ERR_NO_DEVICE, "k_registry_scan returned more validators than the registry holds");
    }

    // ---- host step: the limits, the exit queue's closed form, every refusal -- before anything is written
    pe_registry_stats stats;
    memset(&stats, 0, sizeof stats);
    stats.n_active = tot.n_active;
    stats.churn_limit = registry_churn_limit(tot.n_active, params->min_per_epoch_churn_limit, params->churn_limit_quotient);
    if (stats.churn_limit == 0)
        return fail(h, PE_ERR_INVALID_ARG, "pe_registry_updates: the churn limit is 0 (min_per_epoch_churn_limit)");
    stats.activation_churn_limit = registry_activation_churn_limit(stats.churn_limit, params->max_per_epoch_activation_churn_limit);
    stats.n_marked_eligible = tot.n_marked;
    stats.n_ejected = tot.n_counted;
    stats.queue_len = tot.n_queue;
    stats.activation_epoch = activation_exit_epoch;
    RegistryScalars S;
    memset(&S, 0, sizeof S);
    registry_exit_start(tot.max_exit, tot.n_at_max, tot.n_at_max != 0, activation_exit_epoch, stats.churn_limit, &S.exit_base,
                        &S.exit_fill);
    if (stats.n_ejected) {
        const u128 last = (u128)S.exit_base + (S.exit_fill + (stats.n_ejected - 1)) / stats.churn_limit;
        if (last + params->min_validator_withdrawability_delay >= far)
            return fail(h, PE_ERR_INVALID_ARG, "pe_registry_updates: the last exit epoch + min_validator_withdrawability_delay "
                                               "reaches FAR_FUTURE_EPOCH");
        stats.first_exit_epoch = S.exit_base;
        stats.last_exit_epoch = (uint64_t)last;
    }
    S.current_epoch = current_epoch;
    S.finalized_epoch = finalized_epoch;
    S.max_effective_balance = params->max_effective_balance;
    S.ejection_balance = params->ejection_balance;
    S.eligibility_mark = current_epoch + 1;
    S.by_churn_limit = u64_div_make(stats.churn_limit);
    S.withdrawability_delay = params->min_validator_withdrawability_delay;
    S.activation_epoch = activation_exit_epoch;
    const uint64_t want = std::min(stats.activation_churn_limit, stats.queue_len);
    S.take_all = stats.queue_len <= stats.activation_churn_limit ? 1u : 0u;

    // ---- the head of the queue by (eligibility epoch, index): the threshold epoch byte by byte from the top (read-only).
    // Every queued epoch is <= finalized_epoch, so the bytes above its highest one are 0 in all of them.
    if (!S.take_all) {
        uint32_t top = 0;
        while (top < 7 && (finalized_epoch >> (8 * (top + 1)))) ++top;
        HIP_TRY(h, hipMemsetAsync(ob.dev<uint32_t>(off_hist), 0, 8 * 256 * sizeof(uint32_t), h->stream));
        uint64_t prefix = 0, need = want;  // the need-th smallest epoch among the queued that agree with prefix
        for (int byte = (int)top; byte >= 0; --byte) {
            const size_t off = off_hist + (size_t)byte * 256 * sizeof(uint32_t);
            launch_registry_select(h->stream, d_elig, d_act, n, finalized_epoch, (uint32_t)byte, prefix, ob.dev<uint32_t>(off));
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, ob.download(off, 256 * sizeof(uint32_t)));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            const uint32_t* hist = ob.host<uint32_t>(off);
            uint64_t below = 0;
            uint32_t b = 0;
            while (b < 256 && below + hist[b] < need) below += hist[b++];
            if (b == 256) return fail(h, PE_ERR_NO_DEVICE, "k_registry_select counted fewer queued validators than the census");
            need -= below;
            prefix = (prefix << 8) | b;
        }
        S.threshold = prefix;
        S.threshold_take = need;
        launch_registry_ties(h->stream, d_elig, d_act, n, finalized_epoch, S.threshold, h->d_registry_wg.p,
                             ob.dev<RegistryTotals>(off_ties));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, ob.download(off_ties, sizeof(RegistryTotals)));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (ob.host<RegistryTotals>(off_ties)->n_counted < need)
            return fail(h, PE_ERR_NO_DEVICE, "k_registry_ties counted fewer validators at the threshold than the selection");
    }

    // ---- the writes
    if (stats.n_marked_eligible || stats.n_ejected || want) {
        uint32_t rows = 0;
        const uint32_t* d_activated = launch_registry_apply(h->stream, S, h->d_sbalance.as<uint64_t>(), n, h->d_registry_wg.p, d_elig,
                                                            d_act, d_exit, h->d_withdrawable.as<uint64_t>(), &rows);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(ob.host<uint32_t>(off_activated), d_activated, 4ull * rows, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const uint32_t* p = ob.host<uint32_t>(off_activated);
        for (uint32_t b = 0; b < rows; ++b) stats.n_activated += p[b];
        if (stats.n_ejected || stats.n_activated) h->active_valid = false;  // compacted from the previous epochs
    }
    if (out_stats) *out_stats = stats;
    return PE_OK;
}

int pe_process_slashings(pe_engine* h, uint64_t current_epoch, uint64_t sum_slashings, uint64_t proportional_slashing_multiplier,
                         uint64_t epochs_per_slashings_vector, pe_slashings_stats* out_stats)
{
    if (!h) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready())
        return fail(h, PE_ERR_STATE, "pe_process_slashings: the handle exchanges with other ranks (pe_dist_init); "
                                     "a sharded registry is not supported");
    if (!h->balances_set) return fail(h, PE_ERR_STATE, "pe_process_slashings: no resident balances (pe_state_set_balances first)");
    const uint64_t n = h->n_val;
    if (n && (h->d_sbalance.cap < 8 * n || h->d_sflags.cap < n))
        return fail(h, PE_ERR_STATE, "pe_process_slashings: the working-state view does not cover the registry");
    const uint64_t inc = h->cfg.effective_balance_increment;
    uint64_t scaled = 0, target_epoch = 0;
    if (inc == 0) return fail(h, PE_ERR_INVALID_ARG, "pe_process_slashings: the increment must be positive");
    if (__builtin_mul_overflow(sum_slashings, proportional_slashing_multiplier, &scaled))
        return fail(h, PE_ERR_INVALID_ARG, "pe_process_slashings: sum_slashings * proportional_slashing_multiplier exceeds 64 bits");
    if (__builtin_add_overflow(current_epoch, epochs_per_slashings_vector / 2, &target_epoch))
        return fail(h, PE_ERR_INVALID_ARG, "pe_process_slashings: current_epoch + epochs_per_slashings_vector / 2 exceeds 64 bits");
    OutBlock ob(h);
    const size_t off_ffg = ob.alloc(8ull * 3 * 256);
    const size_t off_census = ob.alloc(8ull * SLASHINGS_CENSUS_Q * SLASHINGS_CENSUS_MAX_WG);
    const size_t off_apply = ob.alloc(8ull * SLASHINGS_APPLY_Q * SLASHINGS_APPLY_MAX_WG);
    PE_TRY(ob.ensure());

    // ---- read-only: get_total_active_balance (pe_ffg_balances' reduction), who is penalised and the largest of them
    uint64_t total = 0, n_penalised = 0, max_eff = 0;
    if (n) {
        const uint32_t ffg_blocks = launch_ffg_balances(h->stream, h->d_sbalance.as<uint64_t>(), h->d_sflags.as<uint8_t>(),
                                                        h->d_part_cur.as<uint8_t>(), h->d_part_prev.as<uint8_t>(), n,
                                                        ob.dev<uint64_t>(off_ffg));
        HIP_TRY(h, hipGetLastError());
        const uint32_t blocks = launch_slashings_census(h->stream, h->d_sbalance.as<uint64_t>(), h->d_sflags.as<uint8_t>(),
                                                        h->d_withdrawable.as<uint64_t>(), n, target_epoch,
                                                        ob.dev<uint64_t>(off_census));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, ob.download(off_ffg, 8ull * 3 * ffg_blocks));
        HIP_TRY(h, ob.download(off_census, 8ull * SLASHINGS_CENSUS_Q * blocks));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const uint64_t* f = ob.host<uint64_t>(off_ffg);
        for (uint32_t b = 0; b < ffg_blocks; ++b) total += f[3 * b];
        const uint64_t* p = ob.host<uint64_t>(off_census);
        for (uint32_t b = 0; b < blocks; ++b) {
            n_penalised += p[(size_t)SLASHINGS_CENSUS_Q * b];
            max_eff = std::max(max_eff, p[(size_t)SLASHINGS_CENSUS_Q * b + 1]);
        }
    }
    total = std::max(inc, total);  // get_total_balance's floor (Appendix A.1), as pe_ffg_balances

    // ---- host step
    pe_slashings_stats stats;
    memset(&stats, 0, sizeof stats);
    stats.total_active_balance = total;
    stats.adjusted_total_slashing_balance = std::min(scaled, total);
    stats.n_penalised = n_penalised;
    if ((unsigned __int128)(max_eff / inc) * stats.adjusted_total_slashing_balance > (unsigned __int128)UINT64_MAX)
        return fail(h, PE_ERR_INVALID_ARG, "pe_process_slashings: effective_balance / increment * the adjusted slashing balance "
                                           "can exceed 64 bits");
    SlashingScalars S;
    memset(&S, 0, sizeof S);
    S.target_epoch = target_epoch;
    S.adjusted = stats.adjusted_total_slashing_balance;
    S.increment = inc;
    S.by_increment = u64_div_make(inc);
    S.by_total = u64_div_make(total);

    // ---- the one writing pass
    if (n_penalised) {
        const uint32_t blocks = launch_slashings_apply(h->stream, S, h->d_sbalance.as<uint64_t>(), h->d_sflags.as<uint8_t>(),
                                                       h->d_withdrawable.as<uint64_t>(), n, h->d_rbalance.as<uint64_t>(),
                                                       ob.dev<uint64_t>(off_apply));
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, ob.download(off_apply, 8ull * SLASHINGS_APPLY_Q * blocks));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const uint64_t* p = ob.host<uint64_t>(off_apply);
        uint64_t seen = 0;
        for (uint32_t b = 0; b < blocks; ++b) {
            seen += p[(size_t)SLASHINGS_APPLY_Q * b + 0];
            stats.penalties += p[(size_t)SLASHINGS_APPLY_Q * b + 1];
            stats.n_saturated += p[(size_t)SLASHINGS_APPLY_Q * b + 2];
        }
        stats.n_penalised = seen;
    }
    if (out_stats) *out_stats = stats;
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
    const bool resident = balances == PE_BALANCES_RESIDENT;  // read where pe_state_set_balances / pe_rewards_and_penalties left them
    if (resident && !h->balances_set)
        return fail(h, PE_ERR_STATE, "PE_BALANCES_RESIDENT: the handle holds no resident balances (pe_state_set_balances first)");
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
    size_t off_bal = 0;
    if (!resident) {
        PE_TRY(st.reserve(8ull * n + 1024));
        off_bal = st.alloc(8ull * n);
        memcpy(st.host<uint64_t>(off_bal), balances, 8ull * n);
    }
    OutBlock ob(h);
    const size_t off_cnt = ob.alloc(8);
    const size_t off_eff = out_effective_balance ? ob.alloc(8ull * n) : 0;
    PE_TRY(ob.ensure());
    PE_TRY(materialise_state_view(h));  // the view still mirrors the registry: a view of its own first, flags included
    HIP_TRY(h, st.upload());
    HIP_TRY(h, hipMemsetAsync(ob.dev<uint64_t>(off_cnt), 0, 8, h->stream));
    launch_effective_balance_update(h->stream, resident ? h->d_rbalance.as<uint64_t>() : st.dev<uint64_t>(off_bal), h->d_sbalance.as<uint64_t>(),
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
