// block_ops_kernels.hip -- proposer slashings, attester slashings and voluntary exits over the resident registry, for gfx950.
// The per-candidate and per-validator rules are block_ops_row.h; the host steps are engine_block_ops.cpp
// (pe_process_block_operations).
//
// One lane per SLOT, BLOCK_OPS_WG of them per workgroup.  The slots of a call are its candidates' positions in (operation,
// index) order: an attester slashing takes one per element of its first list and one per element of its second (checked
// only), a proposer slashing or an exit takes one.  A list is as long as the call's total allows: a lane finds its operation
// by a search over the operations' slot offsets and its list's other side by a search in that list, no list is held in a
// wave or a workgroup.  The slot order IS the candidate order, so the ordered compaction of the intersection is the ordered
// scan over the event flags below; slots that hold no candidate count 0.
//   k_block_ops_lists    read-only: the validator of every slot (an element of the first list that the second holds; the
//                        proposer; the exiting validator), and per operation whether a list is not strictly ascending or
//                        leaves the registry (an OR of flags: the same whatever the order)
//   k_block_ops_claim    read-only: potent candidates take their validator's entry of two tables by a MINIMUM over slots --
//                        the first potent candidate and the first potent slashing candidate: a function of the slots alone,
//                        not of which lane arrives first
//   k_block_ops_resolve  read-only: what every candidate does (BLOCK_EV_*), the single operations' statuses, per operation
//                        whether an attester slashing slashed anyone, per workgroup the fresh exits, the slashed, their
//                        rewards and effective balances
//   k_block_ops_scan     ONE workgroup walks the partials (k_registry_scan's form): exclusive offsets of the fresh exits and
//                        of the rewards per workgroup, the totals, the proposer's balance
//   k_block_ops_apply    the only writing pass: rank and reward prefix = the workgroup's offset + the waves before + the
//                        lanes before.  The lane of a fresh exit writes exit_epoch and withdrawable_epoch; the lane of a slash
//                        writes the flag, the balance and -- where the exit was set before the call -- withdrawable_epoch;
//                        rewards reach the proposer's balance through the lane that slashes it or, where nobody does,
//                        through the call's last lane.  One writer per validator and column, no atomic on a balance.
// No order comes from an atomic, no workgroup waits for another (plain launches on one stream), no scratch.
#include <hip/hip_runtime.h>

#include "block_ops_row.h"
#include "kernels.h"
#include "wave64.h"

namespace posevo {

namespace {

constexpr int BLOCK_OPS_WAVES = BLOCK_OPS_WG / 64;
static_assert(BLOCK_OPS_WG % 64 == 0, "whole waves");

__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// the resident row of one validator as the rules read it
struct Row {
    uint64_t act, ext, wdr;
    uint32_t sflags;
};
__device__ __forceinline__ Row load_row(const BlockOpsRegistry& R, uint32_t v)
{
    Row r;
    r.act = R.activation_epoch[v];
    r.ext = R.exit_epoch[v];
    r.wdr = R.withdrawable[v];
    r.sflags = R.sflags[v];
    return r;
}
__device__ __forceinline__ bool potent(const BlockOpDev& op, bool lists_bad, const Row& r, uint64_t cur, uint64_t period)
{
    return block_ops_potent(op.kind, op.pre, lists_bad, r.sflags, r.act, r.ext, r.wdr, cur, period);
}

}  // namespace

__global__ void __launch_bounds__(BLOCK_OPS_WG)
k_block_ops_lists(const BlockOpDev* __restrict__ ops, const uint32_t* __restrict__ slot_off, uint32_t n_ops,
                  const uint32_t* __restrict__ indices, uint64_t n_val, uint32_t n_slots, uint32_t* __restrict__ slot_val,
                  uint32_t* __restrict__ slot_op, uint32_t* __restrict__ op_bad)
{
    const uint32_t s = blockIdx.x * BLOCK_OPS_WG + threadIdx.x;
    if (s >= n_slots) return;
    const uint32_t o = block_ops_op_of_slot(slot_off, n_ops, s);
    const BlockOpDev op = ops[o];
    const BlockOpsSlot r = block_ops_slot(op, s - slot_off[o], indices, n_val);
    slot_val[s] = r.validator;
    slot_op[s] = o;
    if (r.bad) atomicOr(&op_bad[o], 1u);
}

__global__ void __launch_bounds__(BLOCK_OPS_WG)
k_block_ops_claim(const BlockOpDev* __restrict__ ops, const uint32_t* __restrict__ slot_val, const uint32_t* __restrict__ slot_op,
                  const uint32_t* __restrict__ op_bad, uint32_t n_slots, const BlockOpsRegistry R, uint64_t current_epoch,
                  uint64_t shard_committee_period, uint32_t* __restrict__ first_potent, uint32_t* __restrict__ first_slash)
{
    const uint32_t s = blockIdx.x * BLOCK_OPS_WG + threadIdx.x;
    if (s >= n_slots) return;
    const uint32_t v = slot_val[s];
    if (v == BLOCK_OPS_NONE) return;
    const uint32_t o = slot_op[s];
    const BlockOpDev op = ops[o];
    if (!potent(op, op_bad[o] != 0, load_row(R, v), current_epoch, shard_committee_period)) return;
    atomicMin(&first_potent[v], s);
    if (op.kind != BLOCK_OP_VOLUNTARY_EXIT) atomicMin(&first_slash[v], s);
}

// slots: n_slots candidates' positions and the call's last lane behind them, which holds no candidate here
__global__ void __launch_bounds__(BLOCK_OPS_WG)
k_block_ops_resolve(const BlockOpDev* __restrict__ ops, const uint32_t* __restrict__ slot_val, const uint32_t* __restrict__ slot_op,
                    const uint32_t* __restrict__ op_bad, uint32_t n_slots, const BlockOpsRegistry R, uint64_t current_epoch,
                    uint64_t shard_committee_period, const U64Div by_reward_quotient, const uint32_t* __restrict__ first_potent,
                    const uint32_t* __restrict__ first_slash, uint8_t* __restrict__ slot_ev, uint32_t* __restrict__ op_status,
                    uint32_t* __restrict__ op_hit, BlockOpsWgPart* __restrict__ wg_part)
{
    __shared__ BlockOpsWgPart parts[BLOCK_OPS_WAVES];
    const uint32_t s = blockIdx.x * BLOCK_OPS_WG + threadIdx.x;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t ev = 0;
    uint64_t eff = 0;
    const uint32_t v = s < n_slots ? slot_val[s] : BLOCK_OPS_NONE;
    if (v != BLOCK_OPS_NONE) {
        const uint32_t o = slot_op[s];
        const BlockOpDev op = ops[o];
        const Row r = load_row(R, v);
        const uint32_t fp = first_potent[v], fs = first_slash[v];
        ev = block_ops_events(op.kind, potent(op, op_bad[o] != 0, r, current_epoch, shard_committee_period), s, fp, fs, r.ext);
        if (op.kind == BLOCK_OP_VOLUNTARY_EXIT)
            op_status[o] = block_ops_exit_status(r.act, r.ext, current_epoch, shard_committee_period, fp < s, op.pre);
        else if (op.kind == BLOCK_OP_PROPOSER_SLASHING)
            op_status[o] = block_ops_proposer_status(block_ops_slashable(r.sflags, r.act, r.wdr, current_epoch), fs < s, op.pre);
        if (ev & BLOCK_EV_SLASH) {
            eff = R.eff_balance[v];
            if (op.kind == BLOCK_OP_ATTESTER_SLASHING) atomicOr(&op_hit[o], 1u);
        }
        slot_ev[s] = (uint8_t)ev;
    } else if (s < n_slots) {
        slot_ev[s] = 0;
    }
    const bool slash = ev & BLOCK_EV_SLASH;
    const unsigned long long b_fresh = __ballot(ev & BLOCK_EV_FRESH_EXIT), b_slash = __ballot(slash);
    const unsigned long long rewards = wave_sum<unsigned long long>(slash ? u64_div(eff, by_reward_quotient) : 0),
                             eff_sum = wave_sum<unsigned long long>(eff), eff_max = wave_max<unsigned long long>(eff);
    if ((threadIdx.x & 63) == 0) {
        BlockOpsWgPart p;
        p.n_fresh = (uint32_t)__builtin_popcountll(b_fresh);
        p.n_slashed = (uint32_t)__builtin_popcountll(b_slash);
        p.rewards = rewards;
        p.slashed_balance = eff_sum;
        p.max_eff_slashed = eff_max;
        parts[wave] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        BlockOpsWgPart p = parts[0];
#pragma unroll
        for (int w = 1; w < BLOCK_OPS_WAVES; ++w) {
            p.n_fresh += parts[w].n_fresh;
            p.n_slashed += parts[w].n_slashed;
            p.rewards += parts[w].rewards;
            p.slashed_balance += parts[w].slashed_balance;
            p.max_eff_slashed = max(p.max_eff_slashed, parts[w].max_eff_slashed);
        }
        wg_part[blockIdx.x] = p;
    }
}

// grid: ONE workgroup.  The carries are uniform across it; the loop's trip count depends on n_wg alone.
__global__ void __launch_bounds__(BLOCK_OPS_WG)
k_block_ops_scan(const BlockOpsWgPart* __restrict__ wg_part, uint32_t n_wg, BlockOpsWgOffset* __restrict__ wg_offset,
                 const unsigned long long* __restrict__ balances, uint32_t proposer_index, BlockOpsTotals* __restrict__ totals)
{
    __shared__ uint32_t wave_fresh[BLOCK_OPS_WAVES];
    __shared__ unsigned long long wave_rewards[BLOCK_OPS_WAVES], wave_acc[BLOCK_OPS_WAVES][3];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry_fresh = 0;
    unsigned long long carry_rewards = 0, n_slashed = 0, slashed_balance = 0, max_eff = 0;
    for (uint32_t tile = 0; tile < n_wg; tile += BLOCK_OPS_WG) {
        const uint32_t i = tile + threadIdx.x;
        BlockOpsWgPart p;
        p.n_fresh = p.n_slashed = 0;
        p.rewards = p.slashed_balance = p.max_eff_slashed = 0;
        if (i < n_wg) p = wg_part[i];
        n_slashed += p.n_slashed;
        slashed_balance += p.slashed_balance;
        max_eff = max(max_eff, p.max_eff_slashed);
        const uint32_t incl_fresh = wave_incl_scan(p.n_fresh);
        const unsigned long long incl_rewards = wave_incl_scan(p.rewards);
        if (lane == 63) {
            wave_fresh[wave] = incl_fresh;
            wave_rewards[wave] = incl_rewards;
        }
        __syncthreads();
        uint32_t before_fresh = carry_fresh, all_fresh = 0;
        unsigned long long before_rewards = carry_rewards, all_rewards = 0;
#pragma unroll
        for (int w = 0; w < BLOCK_OPS_WAVES; ++w) {
            before_fresh += (uint32_t)w < wave ? wave_fresh[w] : 0u;
            before_rewards += (uint32_t)w < wave ? wave_rewards[w] : 0ull;
            all_fresh += wave_fresh[w];
            all_rewards += wave_rewards[w];
        }
        if (i < n_wg) {
            BlockOpsWgOffset off;
            off.fresh = before_fresh + incl_fresh - p.n_fresh;
            off.pad = 0;
            off.rewards = before_rewards + incl_rewards - p.rewards;
            wg_offset[i] = off;
        }
        carry_fresh += all_fresh;
        carry_rewards += all_rewards;
        __syncthreads();  // the wave totals are rewritten by the next tile
    }
    n_slashed = wave_sum(n_slashed);
    slashed_balance = wave_sum(slashed_balance);
    max_eff = wave_max(max_eff);
    if (lane == 0) {
        wave_acc[wave][0] = n_slashed;
        wave_acc[wave][1] = slashed_balance;
        wave_acc[wave][2] = max_eff;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        BlockOpsTotals t;
        t.n_fresh = carry_fresh;
        t.rewards = carry_rewards;
        t.n_slashed = t.slashed_balance = t.max_eff_slashed = 0;
#pragma unroll
        for (int w = 0; w < BLOCK_OPS_WAVES; ++w) {
            t.n_slashed += wave_acc[w][0];
            t.slashed_balance += wave_acc[w][1];
            t.max_eff_slashed = max(t.max_eff_slashed, wave_acc[w][2]);
        }
        t.proposer_balance = balances[proposer_index];
        *totals = t;
    }
}

// sums[0] += Gwei debited, sums[1] += subtractions cut at 0 (integer sums: the same in any order); zeroed by the caller.
__global__ void __launch_bounds__(BLOCK_OPS_WG)
k_block_ops_apply(const BlockOpsScalars S, const uint32_t* __restrict__ slot_val, const uint8_t* __restrict__ slot_ev,
                  const BlockOpsWgOffset* __restrict__ wg_offset, const uint32_t* __restrict__ first_slash,
                  const unsigned long long* __restrict__ eff_balance, unsigned long long* __restrict__ exit_epoch,
                  unsigned long long* __restrict__ withdrawable, uint8_t* __restrict__ sflags,
                  unsigned long long* __restrict__ balances, unsigned long long* __restrict__ sums)
{
    __shared__ uint32_t wave_fresh[BLOCK_OPS_WAVES];
    __shared__ unsigned long long wave_rewards[BLOCK_OPS_WAVES];
    const uint32_t s = blockIdx.x * BLOCK_OPS_WG + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ev = s < S.n_slots ? slot_ev[s] : 0u;
    const uint32_t v = ev ? slot_val[s] : BLOCK_OPS_NONE;
    const bool fresh = ev & BLOCK_EV_FRESH_EXIT, slash = ev & BLOCK_EV_SLASH;
    const uint64_t eff = slash ? eff_balance[v] : 0;
    const unsigned long long reward = slash ? u64_div(eff, S.by_reward_quotient) : 0;
    const unsigned long long b_fresh = __ballot(fresh);
    const unsigned long long incl_rewards = wave_incl_scan(reward);
    if (lane == 63) {
        wave_fresh[wave] = (uint32_t)__builtin_popcountll(b_fresh);
        wave_rewards[wave] = incl_rewards;
    }
    __syncthreads();
    const BlockOpsWgOffset off = wg_offset[blockIdx.x];
    uint64_t k = off.fresh, rewards_before = off.rewards;
#pragma unroll
    for (int w = 0; w < BLOCK_OPS_WAVES; ++w) {
        k += (uint32_t)w < wave ? wave_fresh[w] : 0u;
        rewards_before += (uint32_t)w < wave ? wave_rewards[w] : 0ull;
    }
    k += lanes_below(b_fresh);
    rewards_before += incl_rewards - reward;
    if (fresh) {
        const uint64_t q = registry_exit_epoch(S.exit_base, S.exit_fill, k, S.by_churn_limit);
        const uint64_t w = q + S.withdrawability_delay;
        exit_epoch[v] = q;
        withdrawable[v] = first_slash[v] != BLOCK_OPS_NONE ? block_ops_slashed_withdrawable(w, S.slashed_withdrawable) : w;
    }
    unsigned long long debited = 0, saturated = 0;
    if (slash) {
        const bool is_proposer = v == S.proposer_index;
        const BlockOpsDebit d = block_ops_slash_balance(balances[v], u64_div(eff, S.by_penalty_quotient),
                                                        is_proposer ? rewards_before : 0, is_proposer ? S.total_rewards : 0);
        balances[v] = d.balance;
        sflags[v] = (uint8_t)(sflags[v] | REWARD_VAL_SLASHED);
        if (ev & BLOCK_EV_EXIT_WAS_SET) withdrawable[v] = block_ops_slashed_withdrawable(withdrawable[v], S.slashed_withdrawable);
        debited = d.debited;
        saturated = d.saturated;
    }
    // the call's last lane: the proposer's rewards where no lane slashes it
    if (s == S.n_slots && S.total_rewards && first_slash[S.proposer_index] == BLOCK_OPS_NONE)
        balances[S.proposer_index] += S.total_rewards;
    debited = wave_sum(debited);
    saturated = wave_sum(saturated);
    if (lane == 0 && (debited || saturated)) {
        atomicAdd(&sums[0], debited);
        atomicAdd(&sums[1], saturated);
    }
}

uint32_t block_ops_workgroups(uint32_t n_slots) { return n_slots / BLOCK_OPS_WG + 1; }  // n_slots + 1 lanes

void launch_block_ops_lists(hipStream_t s, const BlockOpDev* d_ops, const uint32_t* d_slot_off, uint32_t n_ops,
                            const uint32_t* d_indices, uint64_t n_val, uint32_t n_slots, uint32_t* d_slot_val, uint32_t* d_slot_op,
                            uint32_t* d_op_bad)
{
    if (n_slots == 0) return;
    hipLaunchKernelGGL(k_block_ops_lists, dim3(block_ops_workgroups(n_slots)), dim3(BLOCK_OPS_WG), 0, s, d_ops, d_slot_off, n_ops,
                       d_indices, n_val, n_slots, d_slot_val, d_slot_op, d_op_bad);
}

void launch_block_ops_resolve(hipStream_t s, const BlockOpDev* d_ops, const uint32_t* d_slot_val, const uint32_t* d_slot_op,
                              const uint32_t* d_op_bad, uint32_t n_slots, const BlockOpsRegistry& R, uint64_t current_epoch,
                              uint64_t shard_committee_period, const U64Div& by_reward_quotient, uint32_t* d_first_potent,
                              uint32_t* d_first_slash, uint8_t* d_slot_ev, uint32_t* d_op_status, uint32_t* d_op_hit,
                              BlockOpsWgPart* d_wg_part, BlockOpsWgOffset* d_wg_offset, uint32_t proposer_index,
                              BlockOpsTotals* d_totals)
{
    const uint32_t n_wg = block_ops_workgroups(n_slots);
    if (n_slots)
        hipLaunchKernelGGL(k_block_ops_claim, dim3(n_wg), dim3(BLOCK_OPS_WG), 0, s, d_ops, d_slot_val, d_slot_op, d_op_bad, n_slots, R,
                           current_epoch, shard_committee_period, d_first_potent, d_first_slash);
    hipLaunchKernelGGL(k_block_ops_resolve, dim3(n_wg), dim3(BLOCK_OPS_WG), 0, s, d_ops, d_slot_val, d_slot_op, d_op_bad, n_slots, R,
                       current_epoch, shard_committee_period, by_reward_quotient, (const uint32_t*)d_first_potent,
                       (const uint32_t*)d_first_slash, d_slot_ev, d_op_status, d_op_hit, d_wg_part);
    hipLaunchKernelGGL(k_block_ops_scan, dim3(1), dim3(BLOCK_OPS_WG), 0, s, (const BlockOpsWgPart*)d_wg_part, n_wg, d_wg_offset,
                       reinterpret_cast<const unsigned long long*>(R.balances), proposer_index, d_totals);
}

void launch_block_ops_apply(hipStream_t s, const BlockOpsScalars& S, const uint32_t* d_slot_val, const uint8_t* d_slot_ev,
                            const BlockOpsWgOffset* d_wg_offset, const uint32_t* d_first_slash, const uint64_t* d_eff_balance,
                            uint64_t* d_exit_epoch, uint64_t* d_withdrawable, uint8_t* d_sflags, uint64_t* d_balances,
                            uint64_t* d_sums)
{
    hipLaunchKernelGGL(k_block_ops_apply, dim3(block_ops_workgroups(S.n_slots)), dim3(BLOCK_OPS_WG), 0, s, S, d_slot_val, d_slot_ev,
                       d_wg_offset, d_first_slash, reinterpret_cast<const unsigned long long*>(d_eff_balance),
                       reinterpret_cast<unsigned long long*>(d_exit_epoch), reinterpret_cast<unsigned long long*>(d_withdrawable),
                       d_sflags, reinterpret_cast<unsigned long long*>(d_balances), reinterpret_cast<unsigned long long*>(d_sums));
}

}  // namespace posevo
