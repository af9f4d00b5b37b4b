// registry_kernels.hip -- process_registry_updates and process_slashings over the resident registry, for gfx950.
// The per-validator predicates and arithmetic are registry_row.h; the host steps are engine_epoch.cpp (pe_registry_updates,
// pe_process_slashings).
//
// process_registry_updates, one lane per validator and REGISTRY_WG of them per workgroup:
//   k_registry_census   read-only: the two epochs, the eligibility epoch and the effective balance (coalesced 8-byte loads),
//                       a wave64 ballot and its popcount per predicate -> per workgroup the active, marked, freshly ejected
//                       and queued counts and the pair (largest exit epoch set, how many hold it)
//   k_registry_scan     ONE workgroup walks a count column ACTIVE_SCAN_TILE at a time (k_active_scan's form): exclusive
//                       offsets, the total; with the census also the other totals and the pair, joined as a monoid
//   k_registry_select   read-only, only where the queue is longer than the activation churn limit: the histogram of one
//                       byte of the eligibility epoch over the queued validators that agree with the threshold's known high
//                       bytes (LDS bins, then one add per bin and workgroup: integer counts, exact in any order)
//   k_registry_ties     read-only: per workgroup the queued validators AT the threshold epoch (scanned as above)
//   k_registry_apply    the predicates again; rank among the ejected (and among the ties) = the workgroup's offset + the
//                       counts of the waves before + mbcnt(ballot); writes exit_epoch, withdrawable_epoch,
//                       activation_eligibility_epoch and activation_epoch where they change
// No rank and no order comes from an atomic, no workgroup waits for another (plain launches on one stream), no scratch.
//
// process_slashings: k_slashings_census (read-only: the count and the largest effective balance of the validators the
// penalty falls on, per-workgroup partials) and, after the host step, k_slashings_apply (one streaming pass over flags,
// withdrawable epoch, effective balance and balance).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "registry_row.h"
#include "wave64.h"

namespace posevo {

namespace {

constexpr int REGISTRY_WAVES = REGISTRY_WG / 64;
static_assert(REGISTRY_WG % 64 == 0 && REGISTRY_WG >= 256, "whole waves, and one lane per histogram bin");

__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// the pair over a wave, in every lane (xor butterfly over the monoid)
__device__ __forceinline__ RegistryExitMax wave_exit_max(RegistryExitMax v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        RegistryExitMax o;
        o.epoch = __shfl_xor(v.epoch, off, 64);
        o.count = __shfl_xor(v.count, off, 64);
        v = registry_exit_max_join(v, o);
    }
    return v;
}

}  // namespace

__global__ void __launch_bounds__(REGISTRY_WG)
k_registry_census(const unsigned long long* __restrict__ eligibility, const unsigned long long* __restrict__ activation_epoch,
                  const unsigned long long* __restrict__ exit_epoch, const unsigned long long* __restrict__ eff_balance,
                  uint64_t n_val, uint64_t current_epoch, uint64_t finalized_epoch, uint64_t max_effective_balance,
                  uint64_t ejection_balance, RegistryWgCensus* __restrict__ wg_census, uint32_t* __restrict__ wg_eject)
{
    __shared__ uint32_t counts[REGISTRY_WAVES][4];
    __shared__ RegistryExitMax pairs[REGISTRY_WAVES];
    const uint64_t v = (uint64_t)blockIdx.x * REGISTRY_WG + threadIdx.x;
    const uint32_t wave = threadIdx.x >> 6;
    const bool in = v < n_val;
    const uint64_t el = in ? eligibility[v] : 0, act = in ? activation_epoch[v] : 0, ext = in ? exit_epoch[v] : 0,
                   eff = in ? eff_balance[v] : 0;
    const bool active = in && registry_active(act, ext, current_epoch);
    const bool marked = in && registry_mark(el, eff, max_effective_balance);
    const bool fresh = in && registry_eject_fresh(act, ext, eff, current_epoch, ejection_balance);
    const bool queued = in && registry_queued(el, act, finalized_epoch);
    const unsigned long long b_active = __ballot(active), b_marked = __ballot(marked), b_fresh = __ballot(fresh),
                             b_queued = __ballot(queued);
    RegistryExitMax mine;
    mine.epoch = ext;
    mine.count = in && ext != REGISTRY_FAR_FUTURE_EPOCH ? 1u : 0u;
    mine = wave_exit_max(mine);
    if ((threadIdx.x & 63) == 0) {
        counts[wave][0] = (uint32_t)__builtin_popcountll(b_active);
        counts[wave][1] = (uint32_t)__builtin_popcountll(b_marked);
        counts[wave][2] = (uint32_t)__builtin_popcountll(b_fresh);
        counts[wave][3] = (uint32_t)__builtin_popcountll(b_queued);
        pairs[wave] = mine;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        RegistryWgCensus c;
        c.n_active = c.n_marked = c.n_eject = c.n_queue = 0;
        RegistryExitMax p = pairs[0];
#pragma unroll
        for (int w = 0; w < REGISTRY_WAVES; ++w) {
            c.n_active += counts[w][0];
            c.n_marked += counts[w][1];
            c.n_eject += counts[w][2];
            c.n_queue += counts[w][3];
            if (w) p = registry_exit_max_join(p, pairs[w]);
        }
        c.max_exit = p.epoch;
        c.n_at_max = p.count;
        wg_census[blockIdx.x] = c;
        wg_eject[blockIdx.x] = c.n_eject;
    }
}

// grid: ONE workgroup.  carry is uniform across it; the loop's trip count depends on n_wg alone.  wg_census may be null
// (the tie scan): totals then carries the count alone.
__global__ void __launch_bounds__(ACTIVE_SCAN_TILE)
k_registry_scan(const uint32_t* __restrict__ wg_count, const RegistryWgCensus* __restrict__ wg_census, uint32_t n_wg,
                uint32_t* __restrict__ wg_offset, RegistryTotals* __restrict__ totals)
{
    constexpr int WAVES = ACTIVE_SCAN_TILE / 64;
    __shared__ uint32_t wave_total[WAVES];
    __shared__ unsigned long long wave_sums[WAVES][3];
    __shared__ RegistryExitMax wave_pair[WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    unsigned long long n_active = 0, n_marked = 0, n_queue = 0;
    RegistryExitMax pair;
    pair.epoch = 0;
    pair.count = 0;
    for (uint32_t tile = 0; tile < n_wg; tile += ACTIVE_SCAN_TILE) {
        const uint32_t i = tile + threadIdx.x;
        const uint32_t count = i < n_wg ? wg_count[i] : 0u;
        if (wg_census && i < n_wg) {
            const RegistryWgCensus c = wg_census[i];
            n_active += c.n_active;
            n_marked += c.n_marked;
            n_queue += c.n_queue;
            RegistryExitMax o;
            o.epoch = c.max_exit;
            o.count = c.n_at_max;
            pair = registry_exit_max_join(pair, o);
        }
        uint32_t inclusive = count;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(inclusive, off, 64);
            if (lane >= (uint32_t)off) inclusive += up;
        }
        if (lane == 63) wave_total[wave] = inclusive;
        __syncthreads();
        uint32_t before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t t = wave_total[w];
            before += (uint32_t)w < wave ? t : 0u;
            all += t;
        }
        if (i < n_wg) wg_offset[i] = before + inclusive - count;
        carry += all;
        __syncthreads();  // wave_total is rewritten by the next tile
    }
    n_active = wave_sum(n_active);
    n_marked = wave_sum(n_marked);
    n_queue = wave_sum(n_queue);
    pair = wave_exit_max(pair);
    if (lane == 0) {
        wave_sums[wave][0] = n_active;
        wave_sums[wave][1] = n_marked;
        wave_sums[wave][2] = n_queue;
        wave_pair[wave] = pair;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        RegistryTotals t;
        t.n_active = t.n_marked = t.n_queue = 0;
        RegistryExitMax p = wave_pair[0];
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            t.n_active += wave_sums[w][0];
            t.n_marked += wave_sums[w][1];
            t.n_queue += wave_sums[w][2];
            if (w) p = registry_exit_max_join(p, wave_pair[w]);
        }
        t.n_counted = carry;
        t.max_exit = p.epoch;
        t.n_at_max = p.count;
        *totals = t;
    }
}

// hist[b] += the queued validators whose eligibility epoch has byte `byte` = b and agrees with `prefix` above that byte
// (prefix = the threshold's known bytes, already shifted down: eligibility >> (8 * (byte + 1)); byte 7 has no prefix).
// hist: 256 words, zeroed by the caller.
__global__ void __launch_bounds__(REGISTRY_WG)
k_registry_select(const unsigned long long* __restrict__ eligibility, const unsigned long long* __restrict__ activation_epoch,
                  uint64_t n_val, uint64_t finalized_epoch, uint32_t byte, uint64_t prefix, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t bins[256];
    if (threadIdx.x < 256) bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t v = (uint64_t)blockIdx.x * REGISTRY_WG + threadIdx.x;
    if (v < n_val) {
        const uint64_t el = eligibility[v];
        const uint64_t high = byte == 7 ? 0 : el >> (8 * (byte + 1));
        if (registry_queued(el, activation_epoch[v], finalized_epoch) && high == prefix)
            atomicAdd(&bins[(uint32_t)(el >> (8 * byte)) & 0xFFu], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 256) {
        const uint32_t c = bins[threadIdx.x];
        if (c) atomicAdd(&hist[threadIdx.x], c);
    }
}

__global__ void __launch_bounds__(REGISTRY_WG)
k_registry_ties(const unsigned long long* __restrict__ eligibility, const unsigned long long* __restrict__ activation_epoch,
                uint64_t n_val, uint64_t finalized_epoch, uint64_t threshold, uint32_t* __restrict__ wg_ties)
{
    __shared__ uint32_t counts[REGISTRY_WAVES];
    const uint64_t v = (uint64_t)blockIdx.x * REGISTRY_WG + threadIdx.x;
    bool tie = false;
    if (v < n_val) {
        const uint64_t el = eligibility[v];
        tie = el == threshold && registry_queued(el, activation_epoch[v], finalized_epoch);
    }
    const unsigned long long ballot = __ballot(tie);
    if ((threadIdx.x & 63) == 0) counts[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < REGISTRY_WAVES; ++w) c += counts[w];
        wg_ties[blockIdx.x] = c;
    }
}

// TIES: the queue is longer than the activation churn limit, tie_offset is read.  partials[workgroup] = validators activated.
template <bool TIES>
__global__ void __launch_bounds__(REGISTRY_WG)
k_registry_apply(const RegistryScalars S, const unsigned long long* __restrict__ eff_balance, uint64_t n_val,
                 const uint32_t* __restrict__ eject_offset, const uint32_t* __restrict__ tie_offset,
                 unsigned long long* __restrict__ eligibility, unsigned long long* __restrict__ activation_epoch,
                 unsigned long long* __restrict__ exit_epoch, unsigned long long* __restrict__ withdrawable,
                 uint32_t* __restrict__ partials)
{
    __shared__ uint32_t counts[REGISTRY_WAVES][3];
    const uint64_t v = (uint64_t)blockIdx.x * REGISTRY_WG + threadIdx.x;
    const uint32_t wave = threadIdx.x >> 6;
    const bool in = v < n_val;
    const uint64_t el = in ? eligibility[v] : 0, act = in ? activation_epoch[v] : 0, ext = in ? exit_epoch[v] : 0,
                   eff = in ? eff_balance[v] : 0;
    const bool marked = in && registry_mark(el, eff, S.max_effective_balance);
    const bool fresh = in && registry_eject_fresh(act, ext, eff, S.current_epoch, S.ejection_balance);
    const bool queued = in && registry_queued(el, act, S.finalized_epoch);
    const bool tie = TIES && queued && el == S.threshold;
    const unsigned long long b_fresh = __ballot(fresh), b_tie = __ballot(tie);
    if ((threadIdx.x & 63) == 0) {
        counts[wave][0] = (uint32_t)__builtin_popcountll(b_fresh);
        counts[wave][1] = (uint32_t)__builtin_popcountll(b_tie);
    }
    __syncthreads();
    uint64_t k = eject_offset[blockIdx.x], tie_rank = 0;
    if constexpr (TIES) tie_rank = tie_offset[blockIdx.x];
#pragma unroll
    for (int w = 0; w < REGISTRY_WAVES; ++w) {
        k += (uint32_t)w < wave ? counts[w][0] : 0u;
        tie_rank += (uint32_t)w < wave ? counts[w][1] : 0u;
    }
    k += lanes_below(b_fresh);
    tie_rank += lanes_below(b_tie);
    if (marked) eligibility[v] = S.eligibility_mark;
    if (fresh) {
        const uint64_t q = registry_exit_epoch(S.exit_base, S.exit_fill, k, S.by_churn_limit);
        exit_epoch[v] = q;
        withdrawable[v] = q + S.withdrawability_delay;
    }
    const bool activated = queued && registry_activated(S, el, tie_rank);
    if (activated) activation_epoch[v] = S.activation_epoch;
    const unsigned long long b_activated = __ballot(activated);
    if ((threadIdx.x & 63) == 0) counts[wave][2] = (uint32_t)__builtin_popcountll(b_activated);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < REGISTRY_WAVES; ++w) c += counts[w][2];
        partials[blockIdx.x] = c;
    }
}

static uint32_t registry_workgroups(uint64_t n_val) { return (uint32_t)((n_val + REGISTRY_WG - 1) / REGISTRY_WG); }

size_t registry_scratch_bytes(uint64_t n_val)
{
    // wg_census | eject count, eject offset, tie count, tie offset, activated per workgroup (u32 each)
    return (sizeof(RegistryWgCensus) + 5 * sizeof(uint32_t)) * (size_t)registry_workgroups(n_val);
}

namespace {
struct RegistryScratch {
    RegistryWgCensus* census;
    uint32_t *eject_count, *eject_offset, *tie_count, *tie_offset, *activated;
    uint32_t n_wg;
};
RegistryScratch registry_scratch(void* d_wg, uint64_t n_val)
{
    RegistryScratch s;
    s.n_wg = registry_workgroups(n_val);
    s.census = static_cast<RegistryWgCensus*>(d_wg);
    s.eject_count = reinterpret_cast<uint32_t*>(s.census + s.n_wg);
    s.eject_offset = s.eject_count + s.n_wg;
    s.tie_count = s.eject_offset + s.n_wg;
    s.tie_offset = s.tie_count + s.n_wg;
    s.activated = s.tie_offset + s.n_wg;
    return s;
}
const unsigned long long* ull(const uint64_t* p) { return reinterpret_cast<const unsigned long long*>(p); }
unsigned long long* ull(uint64_t* p) { return reinterpret_cast<unsigned long long*>(p); }
}  // namespace

void launch_registry_census(hipStream_t s, const uint64_t* d_eligibility, const uint64_t* d_activation_epoch,
                            const uint64_t* d_exit_epoch, const uint64_t* d_eff_balance, uint64_t n_val, uint64_t current_epoch,
                            uint64_t finalized_epoch, uint64_t max_effective_balance, uint64_t ejection_balance, void* d_wg,
                            RegistryTotals* d_totals)
{
    if (n_val == 0) return;
    const RegistryScratch w = registry_scratch(d_wg, n_val);
    hipLaunchKernelGGL(k_registry_census, dim3(w.n_wg), dim3(REGISTRY_WG), 0, s, ull(d_eligibility), ull(d_activation_epoch),
                       ull(d_exit_epoch), ull(d_eff_balance), n_val, current_epoch, finalized_epoch, max_effective_balance,
                       ejection_balance, w.census, w.eject_count);
    hipLaunchKernelGGL(k_registry_scan, dim3(1), dim3(ACTIVE_SCAN_TILE), 0, s, (const uint32_t*)w.eject_count,
                       (const RegistryWgCensus*)w.census, w.n_wg, w.eject_offset, d_totals);
}

void launch_registry_select(hipStream_t s, const uint64_t* d_eligibility, const uint64_t* d_activation_epoch, uint64_t n_val,
                            uint64_t finalized_epoch, uint32_t byte, uint64_t prefix, uint32_t* d_hist)
{
    if (n_val == 0) return;
    hipLaunchKernelGGL(k_registry_select, dim3(registry_workgroups(n_val)), dim3(REGISTRY_WG), 0, s, ull(d_eligibility),
                       ull(d_activation_epoch), n_val, finalized_epoch, byte, prefix, d_hist);
}

void launch_registry_ties(hipStream_t s, const uint64_t* d_eligibility, const uint64_t* d_activation_epoch, uint64_t n_val,
                          uint64_t finalized_epoch, uint64_t threshold, void* d_wg, RegistryTotals* d_totals)
{
    if (n_val == 0) return;
    const RegistryScratch w = registry_scratch(d_wg, n_val);
    hipLaunchKernelGGL(k_registry_ties, dim3(w.n_wg), dim3(REGISTRY_WG), 0, s, ull(d_eligibility), ull(d_activation_epoch),
                       n_val, finalized_epoch, threshold, w.tie_count);
    hipLaunchKernelGGL(k_registry_scan, dim3(1), dim3(ACTIVE_SCAN_TILE), 0, s, (const uint32_t*)w.tie_count,
                       (const RegistryWgCensus*)nullptr, w.n_wg, w.tie_offset, d_totals);
}

const uint32_t* launch_registry_apply(hipStream_t s, const RegistryScalars& S, const uint64_t* d_eff_balance, uint64_t n_val,
                                      void* d_wg, uint64_t* d_eligibility, uint64_t* d_activation_epoch, uint64_t* d_exit_epoch,
                                      uint64_t* d_withdrawable, uint32_t* out_n_wg)
{
    *out_n_wg = 0;
    if (n_val == 0) return nullptr;
    const RegistryScratch w = registry_scratch(d_wg, n_val);
    if (S.take_all)
        hipLaunchKernelGGL(k_registry_apply<false>, dim3(w.n_wg), dim3(REGISTRY_WG), 0, s, S, ull(d_eff_balance), n_val,
                           (const uint32_t*)w.eject_offset, (const uint32_t*)nullptr, ull(d_eligibility),
                           ull(d_activation_epoch), ull(d_exit_epoch), ull(d_withdrawable), w.activated);
    else
        hipLaunchKernelGGL(k_registry_apply<true>, dim3(w.n_wg), dim3(REGISTRY_WG), 0, s, S, ull(d_eff_balance), n_val,
                           (const uint32_t*)w.eject_offset, (const uint32_t*)w.tie_offset, ull(d_eligibility),
                           ull(d_activation_epoch), ull(d_exit_epoch), ull(d_withdrawable), w.activated);
    *out_n_wg = w.n_wg;
    return w.activated;
}

// ------------------------------------------------------------------ process_slashings
namespace {
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

// partials[workgroup][SLASHINGS_CENSUS_Q] = {validators the penalty falls on, the largest effective balance among them}
__global__ void __launch_bounds__(256)
k_slashings_census(const unsigned long long* __restrict__ eff_balance, const uint8_t* __restrict__ sflags,
                   const unsigned long long* __restrict__ withdrawable, uint64_t n_val, uint64_t target_epoch,
                   unsigned long long* __restrict__ partials)
{
    unsigned long long count = 0, max_eff = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_val; v += (uint64_t)gridDim.x * blockDim.x) {
        if (slashing_applies(sflags[v], withdrawable[v], target_epoch)) {
            count += 1;
            max_eff = max(max_eff, eff_balance[v]);
        }
    }
    __shared__ unsigned long long lds[4][SLASHINGS_CENSUS_Q];
    const unsigned long long mine[SLASHINGS_CENSUS_Q] = {wave_sum(count), wave_max(max_eff)};
    const unsigned long long r = wg_combine<SLASHINGS_CENSUS_Q>(lds, mine, [](uint32_t q, unsigned long long a, unsigned long long b) {
        return q == 0 ? a + b : max(a, b);
    });
    if (threadIdx.x < SLASHINGS_CENSUS_Q) partials[(uint64_t)blockIdx.x * SLASHINGS_CENSUS_Q + threadIdx.x] = r;
}

// partials[workgroup][SLASHINGS_APPLY_Q] = {validators penalised, Gwei debited (after the cut at 0), subtractions cut at 0}
__global__ void __launch_bounds__(256)
k_slashings_apply(const SlashingScalars S, const unsigned long long* __restrict__ eff_balance, const uint8_t* __restrict__ sflags,
                  const unsigned long long* __restrict__ withdrawable, uint64_t n_val, unsigned long long* __restrict__ balances,
                  unsigned long long* __restrict__ partials)
{
    unsigned long long count = 0, penalties = 0, saturated = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_val; v += (uint64_t)gridDim.x * blockDim.x) {
        if (!slashing_applies(sflags[v], withdrawable[v], S.target_epoch)) continue;
        uint64_t penalty = slashing_penalty(S, eff_balance[v]);
        const uint64_t balance = balances[v];
        if (penalty > balance) {  // decrease_balance's cut at 0
            penalty = balance;
            saturated += 1;
        }
        if (penalty) balances[v] = balance - penalty;
        count += 1;
        penalties += penalty;
    }
    __shared__ unsigned long long lds[4][SLASHINGS_APPLY_Q];
    const unsigned long long mine[SLASHINGS_APPLY_Q] = {wave_sum(count), wave_sum(penalties), wave_sum(saturated)};
    const unsigned long long r = wg_combine<SLASHINGS_APPLY_Q>(lds, mine, [](uint32_t, unsigned long long a, unsigned long long b) {
        return a + b;
    });
    if (threadIdx.x < SLASHINGS_APPLY_Q) partials[(uint64_t)blockIdx.x * SLASHINGS_APPLY_Q + threadIdx.x] = r;
}

uint32_t launch_slashings_census(hipStream_t s, const uint64_t* eff_balance, const uint8_t* sflags, const uint64_t* withdrawable,
                                 uint64_t n_val, uint64_t target_epoch, uint64_t* partials)
{
    if (n_val == 0) return 0;
    uint64_t blocks = (n_val + 256 * 16 - 1) / (256 * 16);  // launch_reward_sums' sizing and cap
    if (blocks > SLASHINGS_CENSUS_MAX_WG) blocks = SLASHINGS_CENSUS_MAX_WG;
    hipLaunchKernelGGL(k_slashings_census, dim3((unsigned)blocks), dim3(256), 0, s, ull(eff_balance), sflags, ull(withdrawable),
                       n_val, target_epoch, ull(partials));
    return (uint32_t)blocks;
}

uint32_t launch_slashings_apply(hipStream_t s, const SlashingScalars& S, const uint64_t* eff_balance, const uint8_t* sflags,
                                const uint64_t* withdrawable, uint64_t n_val, uint64_t* balances, uint64_t* partials)
{
    if (n_val == 0) return 0;
    uint64_t blocks = (n_val + 255) / 256;  // launch_reward_apply's sizing and cap
    if (blocks > SLASHINGS_APPLY_MAX_WG) blocks = SLASHINGS_APPLY_MAX_WG;
    hipLaunchKernelGGL(k_slashings_apply, dim3((unsigned)blocks), dim3(256), 0, s, S, ull(eff_balance), sflags,
                       ull(withdrawable), n_val, ull(balances), ull(partials));
    return (uint32_t)blocks;
}

}  // namespace posevo
