// engine_epoch.cpp -- the epoch boundary over the resident registry: the two registry-wide functions of the reference that
// sit there and whose full text it holds.
//   pe_compute_proposers            compute_proposer_index (pe:604-618), once per seed: k_proposer_sample (shuffle_kernels.hip)
//   pe_effective_balance_updates    process_effective_balance_updates (pe:122-133): k_effective_balance_update (fc_kernels.hip)
// Both read and write the working-state view (d_sbalance / d_incr) and leave the justified-checkpoint data get_head weighs
// (d_balance / d_flags) alone.  Both are synchronous, single-GPU calls; inputs travel through the arena's pinned staging
// block, results through its pinned output block.
#include "engine_internal.h"

using namespace posevo;

extern "C" {

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
    if (n_active == 0) return fail(h, PE_ERR_INVALID_ARG, "pe_compute_proposers: the active set is empty (pe:608)");
    PE_TRY(validate_active_set(h, active_indices, n_active));
    if (max_tries == 0) max_tries = 4096;
    if (n_seeds == 0) return PE_OK;
    const bool identity = active_indices == nullptr;
    Stage st(h);
    PE_TRY(st.reserve(32ull * n_seeds + (identity ? 0 : 4ull * n_active) + 1024));
    const size_t off_seed = st.alloc(32ull * n_seeds);
    const size_t off_idx = st.alloc(identity ? 4 : 4ull * n_active + 4);
    uint32_t* sw = st.host<uint32_t>(off_seed);
    for (uint64_t i = 0; i < 8ull * n_seeds; ++i) {  // the kernels take a seed as 8 big-endian words
        const uint8_t* b = seeds32 + 4 * i;
        sw[i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
    }
    if (!identity) memcpy(st.host<uint32_t>(off_idx), active_indices, 4ull * n_active);
    OutBlock ob(h);
    const size_t off_prop = ob.alloc(4ull * n_seeds);
    const size_t off_tries = ob.alloc(4ull * n_seeds);
    PE_TRY(ob.ensure());
    HIP_TRY(h, st.upload());
    launch_proposer_sample(h->stream, st.dev<uint32_t>(off_seed), n_seeds, n_active, shuffle_round_count,
                           identity ? nullptr : st.dev<uint32_t>(off_idx), h->d_sbalance.as<uint64_t>(),
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
    if (!h->state_view_set) {  // the view still mirrors the registry: make it a view of its own first, flags included
        const size_t n4 = (n + 3) & ~size_t(3);
        HIP_TRY(h, h->d_sbalance.ensure(std::max<size_t>(64, n4 * 8)));
        HIP_TRY(h, h->d_sflags.ensure(std::max<size_t>(64, n4)));
        HIP_TRY(h, hipMemcpyAsync(h->d_sbalance.p, h->d_balance.p, 8 * n, hipMemcpyDeviceToDevice, h->stream));
        launch_state_view_from_registry(h->stream, h->d_flags.as<uint8_t>(), h->d_balance.as<uint64_t>(), inc, n,
                                        h->d_sflags.as<uint8_t>(), h->d_incr.as<uint16_t>());
        HIP_TRY(h, hipGetLastError());
        h->state_view_set = true;
    }
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
