// The per-validator rule, the invariant division and the host step of pos_evolution_amd/csrc/reward_row.h compiled for the
// HOST by a plain C++ compiler, from the very header engine_epoch.cpp and the gfx950 kernels include:
// tests/test_reward_row_host.py holds them against tests/rewards_model.py and Python integers.  With -DRRH_MAIN the file is
// a stand-alone program (its own main) that sweeps the division's edges, for a run under -fsanitize=address,undefined.
#include "../../pos_evolution_amd/csrc/reward_row.h"

using namespace posevo;

extern "C" {

uint64_t rrh_div(uint64_t n, uint64_t d) { return u64_div(n, u64_div_make(d)); }
uint64_t rrh_isqrt(uint64_t n) { return reward_isqrt(n); }

// A whole call the way pe_rewards_and_penalties makes it: first pass, host step, second pass, over host arrays.
// params = {increment, base_reward_factor, bias, recovery, quotient}; out_stats = the nine words of pe_rewards_stats.
// -> 0, or the REWARD_OVERFLOW_* code of the refusal (nothing written).
int rrh_run(uint64_t n, const uint64_t* eff, const uint8_t* sflags, const uint8_t* part, const uint64_t* withdrawable,
            uint64_t* balances, uint64_t* scores, const uint64_t params[5], uint64_t previous_epoch, int in_leak,
            uint32_t which, uint64_t out_stats[9])
{
    const uint64_t inc = params[0];
    uint64_t tot = 0, u[3] = {0, 0, 0}, n_el = 0, max_eff = 0, max_score = 0;
    for (uint64_t v = 0; v < n; ++v) {
        if (sflags[v] & REWARD_VAL_ACTIVE_CUR) tot += eff[v];
        for (uint32_t f = 0; f < 3; ++f)
            if (reward_unslashed(sflags[v], part[v], f)) u[f] += eff[v];
        if (reward_eligible(sflags[v], withdrawable[v], previous_epoch + 1)) {
            ++n_el;
            if (eff[v] > max_eff) max_eff = eff[v];
            if (scores[v] > max_score) max_score = scores[v];
        }
    }
    if (tot < inc) tot = inc;
    for (int f = 0; f < 3; ++f)
        if (u[f] < inc) u[f] = inc;
    RewardScalars S = RewardScalars();
    const int over = reward_scalars_make(inc, params[1], params[2], params[3], params[2] * params[4], tot, u, max_eff, max_score,
                                         previous_epoch, in_leak != 0, which, &S);
    if (over) return over;
    uint64_t rewards = 0, penalties = 0, saturated = 0;
    for (uint64_t v = 0; v < n; ++v) {
        RewardRowStats st = {0, 0, 0};
        reward_row(S, eff[v], sflags[v], part[v], withdrawable[v], &balances[v], &scores[v], &st);
        rewards += st.rewards;
        penalties += st.penalties;
        saturated += st.saturated;
    }
    const uint64_t stats[9] = {tot, u[0], u[1], u[2], n_el, (uint64_t)(in_leak != 0), rewards, penalties, saturated};
    for (int i = 0; i < 9; ++i) out_stats[i] = stats[i];
    return 0;
}

}  // extern "C"

#ifdef RRH_MAIN
#include <stdio.h>
// numerators at both ends and around every multiple boundary of d that 64 bits hold near the top, for divisors at the
// powers of two, beside them and at the engine's own
int main()
{
    typedef unsigned __int128 u128;
    uint64_t divisors[400];
    int nd = 0;
    for (int k = 0; k < 64; ++k)
        for (int64_t delta = -1; delta <= 1; ++delta) {
            const uint64_t d = ((uint64_t)1 << k) + (uint64_t)delta;
            if (d) divisors[nd++] = d;
        }
    const uint64_t more[] = {3, 64, 1000000000ull, 64ull << 27, 3ull * 4 * (1ull << 24), 4ull << 24, UINT64_MAX, UINT64_MAX - 1,
                             0x8000000000000001ull, 207 * 64};
    for (uint64_t d : more) divisors[nd++] = d;
    long checked = 0;
    for (int i = 0; i < nd; ++i) {
        const uint64_t d = divisors[i];
        const U64Div dv = u64_div_make(d);
        const uint64_t top_q = UINT64_MAX / d;
        const uint64_t qs[] = {0, 1, 2, top_q / 2, top_q - 1, top_q};
        for (uint64_t q : qs)
            for (int64_t delta = -2; delta <= 2; ++delta) {
                const u128 wide = (u128)q * d + (u128)(__int128)delta;
                if (wide > (u128)UINT64_MAX) continue;  // also the wrapped negatives
                const uint64_t nn = (uint64_t)wide;
                if (u64_div(nn, dv) != nn / d) {
                    printf("u64_div(%llu, %llu) wrong\n", (unsigned long long)nn, (unsigned long long)d);
                    return 1;
                }
                ++checked;
            }
        const uint64_t ends[] = {UINT64_MAX, UINT64_MAX - 1, UINT64_MAX - d + 1, 0x8000000000000000ull};
        for (uint64_t nn : ends) {
            if (u64_div(nn, dv) != nn / d) return 1;
            ++checked;
        }
    }
    printf("reward_row_host: %ld divisions exact\n", checked);
    return 0;
}
#endif
