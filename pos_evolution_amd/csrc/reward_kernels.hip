// reward_kernels.hip -- process_inactivity_updates and process_rewards_and_penalties over the resident registry, for gfx950.
// Two streaming passes with a host step between them (engine_epoch.cpp, pe_rewards_and_penalties):
//   k_reward_sums    the registry-wide quantities the per-validator rule divides by, and the two maxima the host bounds the
//                    rule's products with: per-workgroup partials, added on the host (no global atomics: the result does
//                    not depend on the order workgroups retire in)
//   k_reward_apply   the per-validator rule of reward_row.h, one lane per validator: score, then the four (rewards,
//                    penalties) pairs in order, each cut at 0 on its own; balance and score are written where they changed
// Both read every array once, coalesced (8-byte and 1-byte lanes in index order).  Bytes per validator: 26 read by the first
// (effective balance 8, flags 1, previous participation 1, score 8, withdrawable epoch 8), 34 read (those and the balance)
// and up to 16 written by the second.  No LDS beyond the 4-wave reduction, no scratch, wave priority not raised: these run
// at the epoch boundary, not beside a head.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "reward_row.h"
#include "wave64.h"

namespace posevo {

namespace {

// the four waves of a workgroup meet in LDS: Q quantities each, slot q of the result in lanes 0 .. Q - 1
template <int Q, typename Combine>
__device__ __forceinline__ unsigned long long wg_combine(unsigned long long (&lds)[4][Q], const unsigned long long (&mine)[Q],
                                                         Combine combine)
{
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) lds[wave][q] = mine[q];
    }
    __syncthreads();
    unsigned long long r = 0;
    if (threadIdx.x < Q) {
        r = lds[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < 4; ++w) r = combine(threadIdx.x, r, lds[w][threadIdx.x]);
    }
    return r;
}

}  // namespace

// partials[workgroup][REWARD_SUMS_Q] = {total active balance, unslashed balance of flag 0, 1, 2, eligible validators,
//                                       largest effective balance among the eligible, largest score among the eligible}
__global__ void __launch_bounds__(256)
k_reward_sums(const unsigned long long* __restrict__ eff_balance, const uint8_t* __restrict__ sflags,
              const uint8_t* __restrict__ part_prev, const unsigned long long* __restrict__ scores,
              const unsigned long long* __restrict__ withdrawable, uint64_t n_val, uint64_t previous_plus_1,
              unsigned long long* __restrict__ partials)
{
    unsigned long long tot = 0, u0 = 0, u1 = 0, u2 = 0, n_el = 0, max_eff = 0, max_score = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_val; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t f = sflags[v], p = part_prev[v];
        const unsigned long long b = eff_balance[v], sc = scores[v], w = withdrawable[v];
        if (f & REWARD_VAL_ACTIVE_CUR) tot += b;
        if (reward_unslashed(f, p, 0)) u0 += b;
        if (reward_unslashed(f, p, 1)) u1 += b;
        if (reward_unslashed(f, p, 2)) u2 += b;
        if (reward_eligible(f, w, previous_plus_1)) {
            n_el += 1;
            max_eff = max(max_eff, b);
            max_score = max(max_score, sc);
        }
    }
    __shared__ unsigned long long lds[4][REWARD_SUMS_Q];
    const unsigned long long mine[REWARD_SUMS_Q] = {wave_sum(tot), wave_sum(u0), wave_sum(u1), wave_sum(u2), wave_sum(n_el),
                                                    wave_max(max_eff), wave_max(max_score)};
    const unsigned long long r = wg_combine<REWARD_SUMS_Q>(lds, mine, [](uint32_t q, unsigned long long a, unsigned long long b) {
        return q < 5 ? a + b : max(a, b);
    });
    if (threadIdx.x < REWARD_SUMS_Q) partials[(uint64_t)blockIdx.x * REWARD_SUMS_Q + threadIdx.x] = r;
}

uint32_t launch_reward_sums(hipStream_t s, const uint64_t* eff_balance, const uint8_t* sflags, const uint8_t* part_prev,
                            const uint64_t* scores, const uint64_t* withdrawable, uint64_t n_val, uint64_t previous_plus_1,
                            uint64_t* partials)
{
    if (n_val == 0) return 0;
    uint64_t blocks = (n_val + 256 * 16 - 1) / (256 * 16);  // launch_ffg_balances' sizing and cap
    if (blocks > REWARD_SUMS_MAX_WG) blocks = REWARD_SUMS_MAX_WG;
    hipLaunchKernelGGL(k_reward_sums, dim3((unsigned)blocks), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(eff_balance), sflags, part_prev,
                       reinterpret_cast<const unsigned long long*>(scores),
                       reinterpret_cast<const unsigned long long*>(withdrawable), n_val, previous_plus_1,
                       reinterpret_cast<unsigned long long*>(partials));
    return (uint32_t)blocks;
}

// partials[workgroup][REWARD_APPLY_Q] = {rewards credited, penalties debited, validators with a subtraction cut at 0}
__global__ void __launch_bounds__(256)
k_reward_apply(const RewardScalars S, const unsigned long long* __restrict__ eff_balance, const uint8_t* __restrict__ sflags,
               const uint8_t* __restrict__ part_prev, const unsigned long long* __restrict__ withdrawable, uint64_t n_val,
               unsigned long long* __restrict__ balances, unsigned long long* __restrict__ scores,
               unsigned long long* __restrict__ partials)
{
    unsigned long long rewards = 0, penalties = 0, saturated = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_val; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t balance = balances[v], score = scores[v];
        uint64_t new_balance = balance, new_score = score;
        RewardRowStats st = {0, 0, 0};
        reward_row(S, eff_balance[v], sflags[v], part_prev[v], withdrawable[v], &new_balance, &new_score, &st);
        if (new_balance != balance) balances[v] = new_balance;
        if (new_score != score) scores[v] = new_score;
        rewards += st.rewards;
        penalties += st.penalties;
        saturated += st.saturated;
    }
    __shared__ unsigned long long lds[4][REWARD_APPLY_Q];
    const unsigned long long mine[REWARD_APPLY_Q] = {wave_sum(rewards), wave_sum(penalties), wave_sum(saturated)};
    const unsigned long long r = wg_combine<REWARD_APPLY_Q>(lds, mine, [](uint32_t, unsigned long long a, unsigned long long b) {
        return a + b;
    });
    if (threadIdx.x < REWARD_APPLY_Q) partials[(uint64_t)blockIdx.x * REWARD_APPLY_Q + threadIdx.x] = r;
}

uint32_t launch_reward_apply(hipStream_t s, const RewardScalars& S, const uint64_t* eff_balance, const uint8_t* sflags,
                             const uint8_t* part_prev, const uint64_t* withdrawable, uint64_t n_val, uint64_t* balances,
                             uint64_t* scores, uint64_t* partials)
{
    if (n_val == 0) return 0;
    uint64_t blocks = (n_val + 255) / 256;  // one lane per validator, until the registry outgrows eight workgroups per CU
    if (blocks > REWARD_APPLY_MAX_WG) blocks = REWARD_APPLY_MAX_WG;
    hipLaunchKernelGGL(k_reward_apply, dim3((unsigned)blocks), dim3(256), 0, s, S,
                       reinterpret_cast<const unsigned long long*>(eff_balance), sflags, part_prev,
                       reinterpret_cast<const unsigned long long*>(withdrawable), n_val,
                       reinterpret_cast<unsigned long long*>(balances), reinterpret_cast<unsigned long long*>(scores),
                       reinterpret_cast<unsigned long long*>(partials));
    return (uint32_t)blocks;
}

}  // namespace posevo
