// The per-validator predicates, the exit queue's closed form, the (largest exit epoch, holders) pair and the slashing penalty
// of pos_evolution_amd/csrc/registry_row.h compiled for the HOST by a plain C++ compiler, from the very header
// engine_epoch.cpp and the gfx950 kernels include: tests/test_registry_row_host.py holds them against
// tests/registry_updates_model.py.  With -DRGH_MAIN the file is a stand-alone program (its own main) that holds the closed
// form to the sequential exit loop on small registries, for a run under -fsanitize=address,undefined.
#include <algorithm>
#include <vector>

#include "../../pos_evolution_amd/csrc/registry_row.h"

using namespace posevo;

extern "C" {

// A whole call the way pe_registry_updates makes it: census, host step, selection, apply, over host arrays.
// params = the seven words of pe_registry_params; out_stats = the ten words of pe_registry_stats.
// -> 0, or 1 quotient 0, 2 look-ahead epoch reaches FAR, 3 churn limit 0, 4 withdrawable epoch reaches FAR (nothing written).
int rgh_registry_updates(uint64_t n, uint64_t* elig, uint64_t* act, uint64_t* ext, uint64_t* wdr, const uint64_t* eff,
                         const uint64_t params[7], uint64_t cur, uint64_t fin, uint64_t out_stats[10])
{
    typedef unsigned __int128 u128;
    const uint64_t max_eff = params[0], ejection = params[1], lookahead = params[2], delay = params[3], min_churn = params[4],
                   quotient = params[5], cap = params[6];
    if (quotient == 0) return 1;
    const u128 target_wide = (u128)cur + 1 + lookahead;
    if (target_wide >= (u128)REGISTRY_FAR_FUTURE_EPOCH) return 2;
    const uint64_t target = (uint64_t)target_wide;
    uint64_t n_active = 0, n_marked = 0, n_eject = 0;
    RegistryExitMax pair = {0, 0};
    std::vector<uint64_t> queue;  // eligibility epochs of the queued
    for (uint64_t v = 0; v < n; ++v) {
        n_active += registry_active(act[v], ext[v], cur);
        n_marked += registry_mark(elig[v], eff[v], max_eff);
        n_eject += registry_eject_fresh(act[v], ext[v], eff[v], cur, ejection);
        if (registry_queued(elig[v], act[v], fin)) queue.push_back(elig[v]);
        const RegistryExitMax one = {ext[v], ext[v] != REGISTRY_FAR_FUTURE_EPOCH ? 1u : 0u};
        pair = v & 1 ? registry_exit_max_join(pair, one) : registry_exit_max_join(one, pair);  // either order
    }
    const uint64_t limit = registry_churn_limit(n_active, min_churn, quotient);
    if (limit == 0) return 3;
    const uint64_t activation_limit = registry_activation_churn_limit(limit, cap);
    RegistryScalars S = RegistryScalars();
    registry_exit_start(pair.epoch, pair.count, pair.count != 0, target, limit, &S.exit_base, &S.exit_fill);
    uint64_t first = 0, last = 0;
    if (n_eject) {
        const u128 last_wide = (u128)S.exit_base + (S.exit_fill + (n_eject - 1)) / limit;
        if (last_wide + delay >= (u128)REGISTRY_FAR_FUTURE_EPOCH) return 4;
        first = S.exit_base;
        last = (uint64_t)last_wide;
    }
    S.current_epoch = cur;
    S.finalized_epoch = fin;
    S.max_effective_balance = max_eff;
    S.ejection_balance = ejection;
    S.eligibility_mark = cur + 1;
    S.by_churn_limit = u64_div_make(limit);
    S.withdrawability_delay = delay;
    S.activation_epoch = target;
    S.take_all = queue.size() <= activation_limit;
    if (!S.take_all) {  // the activation_limit-th smallest epoch, and how many of its holders are taken
        std::vector<uint64_t> sorted(queue);
        std::sort(sorted.begin(), sorted.end());
        S.threshold = sorted[activation_limit - 1];
        S.threshold_take = activation_limit - (uint64_t)(std::lower_bound(sorted.begin(), sorted.end(), S.threshold) - sorted.begin());
    }
    uint64_t k = 0, tie_rank = 0, n_activated = 0;
    for (uint64_t v = 0; v < n; ++v) {
        const uint64_t el = elig[v];
        const bool marked = registry_mark(el, eff[v], max_eff);
        const bool fresh = registry_eject_fresh(act[v], ext[v], eff[v], cur, ejection);
        const bool queued = registry_queued(el, act[v], fin);
        const bool tie = !S.take_all && queued && el == S.threshold;
        if (marked) elig[v] = S.eligibility_mark;
        if (fresh) {
            ext[v] = registry_exit_epoch(S.exit_base, S.exit_fill, k++, S.by_churn_limit);
            wdr[v] = ext[v] + delay;
        }
        if (queued && registry_activated(S, el, tie_rank)) {
            act[v] = S.activation_epoch;
            ++n_activated;
        }
        tie_rank += tie;
    }
    const uint64_t stats[10] = {n_active, limit, activation_limit, n_marked, n_eject, first, last, (uint64_t)queue.size(),
                                n_activated, target};
    for (int i = 0; i < 10; ++i) out_stats[i] = stats[i];
    return 0;
}

// pe_process_slashings over host arrays.  -> 0, or 1 sum * multiplier, 2 the target epoch, 3 the penalty's product exceeds
// 64 bits (nothing written).  out_stats = the five words of pe_slashings_stats.
int rgh_slashings(uint64_t n, const uint64_t* eff, const uint8_t* sflags, const uint64_t* wdr, uint64_t* bal, uint64_t inc,
                  uint64_t cur, uint64_t sum_slashings, uint64_t multiplier, uint64_t vector, uint64_t out_stats[5])
{
    uint64_t scaled = 0, target = 0, total = 0, max_eff = 0;
    if (__builtin_mul_overflow(sum_slashings, multiplier, &scaled)) return 1;
    if (__builtin_add_overflow(cur, vector / 2, &target)) return 2;
    for (uint64_t v = 0; v < n; ++v) {
        if (sflags[v] & REWARD_VAL_ACTIVE_CUR) total += eff[v];
        if (slashing_applies(sflags[v], wdr[v], target) && eff[v] > max_eff) max_eff = eff[v];
    }
    if (total < inc) total = inc;
    SlashingScalars S = SlashingScalars();
    S.target_epoch = target;
    S.adjusted = scaled < total ? scaled : total;
    S.increment = inc;
    S.by_increment = u64_div_make(inc);
    S.by_total = u64_div_make(total);
    if ((unsigned __int128)(max_eff / inc) * S.adjusted > (unsigned __int128)UINT64_MAX) return 3;
    uint64_t count = 0, penalties = 0, saturated = 0;
    for (uint64_t v = 0; v < n; ++v) {
        if (!slashing_applies(sflags[v], wdr[v], target)) continue;
        uint64_t penalty = slashing_penalty(S, eff[v]);
        if (penalty > bal[v]) {
            penalty = bal[v];
            ++saturated;
        }
        bal[v] -= penalty;
        ++count;
        penalties += penalty;
    }
    const uint64_t stats[5] = {total, S.adjusted, count, penalties, saturated};
    for (int i = 0; i < 5; ++i) out_stats[i] = stats[i];
    return 0;
}

}  // extern "C"

#ifdef RGH_MAIN
#include <stdio.h>
// small registries with exits already set at and around the look-ahead epoch, every churn limit from 1 to 5: the closed form
// against initiate_validator_exit called validator by validator
int main()
{
    const uint64_t FAR = REGISTRY_FAR_FUTURE_EPOCH;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&state]() {
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return state;
    };
    long checked = 0;
    for (int round = 0; round < 400; ++round) {
        const uint64_t n = 1 + next() % 40, cur = 10, limit = 1 + next() % 5, target = cur + 1 + 4;
        std::vector<uint64_t> elig(n, 0), act(n, 0), ext(n), wdr(n, FAR), eff(n);
        for (uint64_t v = 0; v < n; ++v) {
            const uint64_t r = next() % 8;
            ext[v] = r < 5 ? FAR : target - 1 + next() % 4;
            eff[v] = next() % 2 ? 16000000000ull : 32000000000ull;
        }
        std::vector<uint64_t> want(ext);
        for (uint64_t v = 0; v < n; ++v) {
            if (!(act[v] <= cur && cur < want[v] && eff[v] <= 16000000000ull) || want[v] != FAR) continue;
            uint64_t q = target, holders = 0;
            for (uint64_t e : want)
                if (e != FAR && e > q) q = e;
            for (uint64_t e : want) holders += e == q;
            if (holders >= limit) ++q;
            want[v] = q;
        }
        const uint64_t params[7] = {32000000000ull, 16000000000ull, 4, 256, limit, 1ull << 40, 0};
        uint64_t stats[10];
        if (rgh_registry_updates(n, elig.data(), act.data(), ext.data(), wdr.data(), eff.data(), params, cur, 5, stats)) return 2;
        for (uint64_t v = 0; v < n; ++v) {
            if (ext[v] != want[v] || (want[v] != FAR && wdr[v] != FAR && wdr[v] != want[v] + 256)) {
                printf("round %d validator %llu: %llu, sequential %llu\n", round, (unsigned long long)v,
                       (unsigned long long)ext[v], (unsigned long long)want[v]);
                return 1;
            }
            ++checked;
        }
    }
    printf("registry_row_host: %ld exit epochs, closed form exact\n", checked);
    return 0;
}
#endif
