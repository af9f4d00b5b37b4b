// sync_kernels.hip -- Altair's sync committee on gfx950 (the rules restated in tests/sync_committee_model.py).
//   k_sync_sample   get_next_sync_committee_indices: one candidate i per lane over SYNC_SAMPLE_BATCH candidates a launch -- the
//                   round pivots once per workgroup into LDS, the walk and the acceptance of sample_walk.h (k_proposer_sample's
//                   own), then an ORDERED compaction of the accepting lanes inside the workgroup: wave64 ballot, the waves'
//                   counts through LDS -> wg_entry[b][0 .. wg_count[b])
//   k_sync_append   one wave: an exclusive scan over the workgroups' counts behind the running count in device memory; the
//                   first `size` acceptances of all batches in order of i -> members[], and the i of the last one
//   k_sync_members  per aggregate: the set bits of its Bitvector over the resident committee -> the participants' validator
//                   indices in committee order (duplicates kept), their count, a flag for a set bit at a position >= size, and
//                   the signing root sha256(block_root || domain)
//   k_sync_rewards  process_sync_aggregate's balance changes with the reference's sequential semantics and no atomics: one lane
//                   OWNS one distinct validator and replays that validator's events in the order (aggregate, position)
// Integer / hash work, no MFMA.  No kernel here may use scratch memory (tests/test_sync_committee_build.py reads the log).
#include "kernels.h"
#include "sample_walk.h"
#include "sha256.h"
#include "wave64.h"

namespace posevo {

static_assert(SYNC_SAMPLE_BATCH % SYNC_SAMPLE_WG == 0 && SYNC_SAMPLE_BATCH / SYNC_SAMPLE_WG == 64,
              "k_sync_append scans the workgroups' counts in ONE wave");
static_assert(SYNC_SAMPLE_WG % 64 == 0 && SYNC_SAMPLE_WG >= (int)PROP_MAX_ROUNDS, "whole waves; a pivot per lane in one pass");
constexpr int SYNC_SAMPLE_WAVES = SYNC_SAMPLE_WG / 64;
constexpr uint32_t SYNC_SAMPLE_NWG = SYNC_SAMPLE_BATCH / SYNC_SAMPLE_WG;

// lanes of the wave below this one whose bit of the ballot is set
__device__ __forceinline__ uint32_t ballot_rank(unsigned long long ballot)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// grid: SYNC_SAMPLE_NWG workgroups; lane t of workgroup b examines i = base + b * SYNC_SAMPLE_WG + t.  i >= max_tries never accepts.
__global__ void __launch_bounds__(SYNC_SAMPLE_WG)
k_sync_sample(const uint32_t* __restrict__ seed_be /* 8 big-endian words */, uint32_t total, uint32_t rounds,
              const uint32_t* __restrict__ indices /* [total] or null = identity */,
              const unsigned long long* __restrict__ eff_balance, unsigned long long max_eff, unsigned long long base,
              unsigned long long max_tries, uint32_t* __restrict__ wg_count /* [SYNC_SAMPLE_NWG] */,
              uint2* __restrict__ wg_entry /* [SYNC_SAMPLE_NWG][SYNC_SAMPLE_WG]: (validator, i) */)
{
    __shared__ uint32_t pivots[PROP_MAX_ROUNDS];
    __shared__ uint32_t wave_count[SYNC_SAMPLE_WAVES];
    const uint32_t t = threadIdx.x, wave = t >> 6;
    uint32_t w[16];
    uint32_t dig[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = seed_be[k];
    if (t < rounds) pivots[t] = sample_pivot(w, dig, t, total);
    __syncthreads();
    const unsigned long long i = base + (unsigned long long)blockIdx.x * SYNC_SAMPLE_WG + t;
    const uint32_t index = sample_walk(w, dig, pivots, rounds, total, i);
    const unsigned long long random_byte = sample_random_byte(w, dig, i);
    const uint32_t candidate = indices ? indices[index] : index;
    const bool accept = i < max_tries && sample_accepts(eff_balance[candidate], max_eff, random_byte);
    const unsigned long long ballot = __ballot(accept);
    if ((t & 63) == 0) wave_count[wave] = (uint32_t)__builtin_popcountll(ballot);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < SYNC_SAMPLE_WAVES; ++k) {
        const uint32_t c = wave_count[k];
        before += (uint32_t)k < wave ? c : 0u;
        all += c;
    }
    // before + rank < all <= SYNC_SAMPLE_WG: inside the workgroup's own row
    if (accept) wg_entry[(size_t)blockIdx.x * SYNC_SAMPLE_WG + before + ballot_rank(ballot)] = make_uint2(candidate, (uint32_t)i);
    if (t == 0) wg_count[blockIdx.x] = all;
}

// grid: ONE wave.  state->count acceptances are in members[] already; this batch's follow in the order of i.
__global__ void __launch_bounds__(64)
k_sync_append(const uint32_t* __restrict__ wg_count, const uint2* __restrict__ wg_entry, uint32_t size,
              SyncSampleState* __restrict__ state, uint32_t* __restrict__ members /* [size] */)
{
    const uint32_t b = threadIdx.x;
    const uint32_t run = state->count;  // every lane reads it before lane 63 rewrites it below
    const uint32_t count = b < SYNC_SAMPLE_NWG ? min(wg_count[b], (uint32_t)SYNC_SAMPLE_WG) : 0u;
    const uint32_t inclusive = wave_incl_scan(count);
    const uint32_t first = run + inclusive - count;
    for (uint32_t r = 0; r < count; ++r) {
        const uint32_t pos = first + r;
        if (pos >= size) break;
        const uint2 e = wg_entry[(size_t)b * SYNC_SAMPLE_WG + r];
        members[pos] = e.x;
        if (pos == size - 1) state->tries = e.y + 1;  // the i of the last accepted candidate + 1
    }
    if (b == 63) state->count = min(size, run + inclusive);
}

int launch_sync_sample(hipStream_t s, const uint32_t* d_seed_be, uint32_t total, uint32_t rounds, const uint32_t* d_indices,
                        const uint64_t* d_eff_balance, uint64_t max_eff, uint64_t base, uint64_t max_tries, uint32_t size,
                        uint32_t* d_wg_count, uint32_t* d_wg_entry, SyncSampleState* d_state, uint32_t* d_members)
{
    if (total == 0 || rounds >= PROP_MAX_ROUNDS || size == 0 || size > SYNC_COMMITTEE_MAX) return -1;
    hipLaunchKernelGGL(k_sync_sample, dim3(SYNC_SAMPLE_NWG), dim3(SYNC_SAMPLE_WG), 0, s, d_seed_be, total, rounds, d_indices,
                       reinterpret_cast<const unsigned long long*>(d_eff_balance), (unsigned long long)max_eff,
                       (unsigned long long)base, (unsigned long long)max_tries, d_wg_count, reinterpret_cast<uint2*>(d_wg_entry));
    hipLaunchKernelGGL(k_sync_append, dim3(1), dim3(64), 0, s, d_wg_count, reinterpret_cast<const uint2*>(d_wg_entry), size,
                       d_state, d_members);
    return 0;
}

// ------------------------------------------------------------------ process_sync_aggregate
// An aggregate as it travels (pe_sync_aggregate, include/posevo.h) in 32-bit words: bits 16 | signature 24 | block_root 8 |
// domain 8 | proposer_index 1 | pad 1.  Bit p of the Bitvector is (bits[p / 8] >> (p % 8)) & 1 = bit (p % 32) of word p / 32
// read little-endian.
constexpr uint32_t SYNC_AGG_BITS = 0, SYNC_AGG_ROOT = 40, SYNC_AGG_PROPOSER = 56;
constexpr int SYNC_MEMBERS_WAVES = SYNC_COMMITTEE_MAX / 64;

// grid: one workgroup per aggregate, one lane per committee position.
__global__ void __launch_bounds__(SYNC_COMMITTEE_MAX)
k_sync_members(const uint32_t* __restrict__ aggs, const uint32_t* __restrict__ committee, uint32_t size,
               uint32_t* __restrict__ lists /* [n][SYNC_COMMITTEE_MAX] */, uint32_t* __restrict__ counts /* [n] */,
               uint32_t* __restrict__ bad /* [n] */, uint32_t* __restrict__ roots /* [n][8]: the digest's bytes in order */)
{
    __shared__ uint32_t wave_count[SYNC_MEMBERS_WAVES], wave_bad[SYNC_MEMBERS_WAVES];
    const uint32_t p = threadIdx.x, wave = p >> 6, b = blockIdx.x;
    const uint32_t* agg = aggs + (size_t)SYNC_AGG_WORDS * b;
    const bool bit = (agg[SYNC_AGG_BITS + (p >> 5)] >> (p & 31u)) & 1u;
    const unsigned long long ballot = __ballot(bit && p < size);
    const unsigned long long outside = __ballot(bit && p >= size);
    if ((p & 63) == 0) {
        wave_count[wave] = (uint32_t)__builtin_popcountll(ballot);
        wave_bad[wave] = outside != 0;
    }
    __syncthreads();
    uint32_t before = 0, all = 0, any_bad = 0;
#pragma unroll
    for (int k = 0; k < SYNC_MEMBERS_WAVES; ++k) {
        const uint32_t c = wave_count[k];
        before += (uint32_t)k < wave ? c : 0u;
        all += c;
        any_bad |= wave_bad[k];
    }
    if (bit && p < size) lists[(size_t)SYNC_COMMITTEE_MAX * b + before + ballot_rank(ballot)] = committee[p];
    if (p == 0) {
        counts[b] = all;
        bad[b] = any_bad;
        // hash_tree_root(SigningData(object_root = block_root, domain)) = sha256 of the 64 bytes: two compressions, the second
        // over the constant padding block
        uint32_t in[16], dig[8];
#pragma unroll
        for (int k = 0; k < 16; ++k) in[k] = __builtin_bswap32(agg[SYNC_AGG_ROOT + k]);
        sha256_64(in, dig);
#pragma unroll
        for (int k = 0; k < 8; ++k) roots[8 * (size_t)b + k] = __builtin_bswap32(dig[k]);
    }
}

int launch_sync_members(hipStream_t s, const uint32_t* d_aggs, uint32_t n, const uint32_t* d_committee, uint32_t size,
                         uint32_t* d_lists, uint32_t* d_counts, uint32_t* d_bad, uint32_t* d_roots)
{
    if (n == 0 || n > SYNC_MAX_BATCH || size == 0 || size > SYNC_COMMITTEE_MAX) return -1;
    hipLaunchKernelGGL(k_sync_members, dim3(n), dim3(SYNC_COMMITTEE_MAX), 0, s, d_aggs, d_committee, size, d_lists, d_counts,
                       d_bad, d_roots);
    return 0;
}

// Lane t < SYNC_COMMITTEE_MAX stands for committee position t, lane SYNC_COMMITTEE_MAX + b for the proposer of aggregate b.
// A lane owns its validator where it is the validator's FIRST appearance: the first position that lists it, or -- for a
// proposer outside the committee -- the first aggregate that names it.  The owner alone touches balances[v], with plain loads
// and stores, and walks every (aggregate b, position p) in order:
//   member[p] == v, bit set     += participant_reward
//   member[p] == v, bit clear   decrease_balance: -= min(balance, participant_reward)
//   proposer_b == v, bit set    += proposer_reward
// (within one (b, p) the participant's change comes first, as in the reference's loop body).  Additions wrap unchecked, as in
// k_reward_apply.  stats: Gwei credited | Gwei debited | decreases cut at 0.
constexpr int SYNC_REWARDS_WG = SYNC_COMMITTEE_MAX + SYNC_MAX_BATCH;
constexpr int SYNC_REWARDS_WAVES = SYNC_REWARDS_WG / 64;
static_assert(SYNC_REWARDS_WG % 64 == 0 && SYNC_REWARDS_WG <= 1024, "whole waves of one workgroup");

__global__ void __launch_bounds__(SYNC_REWARDS_WG)
k_sync_rewards(const uint32_t* __restrict__ aggs, uint32_t n, const uint32_t* __restrict__ committee, uint32_t size,
               unsigned long long participant_reward, unsigned long long proposer_reward,
               unsigned long long* __restrict__ balances, unsigned long long* __restrict__ stats /* [3] */)
{
    __shared__ uint32_t member[SYNC_COMMITTEE_MAX];
    __shared__ uint32_t bits[SYNC_MAX_BATCH * 16];
    __shared__ uint32_t proposer[SYNC_MAX_BATCH];
    __shared__ unsigned long long wave_stats[SYNC_REWARDS_WAVES][3];
    const uint32_t t = threadIdx.x;
    if (t < SYNC_COMMITTEE_MAX) member[t] = t < size ? committee[t] : NONE32;
    for (uint32_t k = t; k < 16 * n; k += SYNC_REWARDS_WG) bits[k] = aggs[(size_t)SYNC_AGG_WORDS * (k >> 4) + SYNC_AGG_BITS + (k & 15u)];
    if (t < n) proposer[t] = aggs[(size_t)SYNC_AGG_WORDS * t + SYNC_AGG_PROPOSER];
    __syncthreads();
    bool owner;
    uint32_t v;
    if (t < SYNC_COMMITTEE_MAX) {
        v = member[t];
        owner = t < size;
        for (uint32_t q = 0; q < t && owner; ++q) owner = member[q] != v;
    } else {
        const uint32_t b = t - SYNC_COMMITTEE_MAX;
        owner = b < n;
        v = owner ? proposer[b] : NONE32;
        for (uint32_t q = 0; q < size && owner; ++q) owner = member[q] != v;
        for (uint32_t q = 0; q < b && owner; ++q) owner = proposer[q] != v;
    }
    unsigned long long credited = 0, debited = 0, saturated = 0;
    if (owner) {
        unsigned long long balance = balances[v];
        for (uint32_t b = 0; b < n; ++b) {
            const bool proposes = proposer[b] == v;
            for (uint32_t p = 0; p < size; ++p) {
                const bool listed = member[p] == v;
                if (!listed && !proposes) continue;
                const bool bit = (bits[16 * b + (p >> 5)] >> (p & 31u)) & 1u;
                if (listed) {
                    if (bit) {
                        balance += participant_reward;
                        credited += participant_reward;
                    } else {
                        const unsigned long long cut = min(balance, participant_reward);
                        saturated += balance < participant_reward;
                        balance -= cut;
                        debited += cut;
                    }
                }
                if (proposes && bit) {
                    balance += proposer_reward;
                    credited += proposer_reward;
                }
            }
        }
        balances[v] = balance;
    }
    credited = wave_sum(credited);
    debited = wave_sum(debited);
    saturated = wave_sum(saturated);
    if ((t & 63) == 0) {
        wave_stats[t >> 6][0] = credited;
        wave_stats[t >> 6][1] = debited;
        wave_stats[t >> 6][2] = saturated;
    }
    __syncthreads();
    if (t < 3) {
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < SYNC_REWARDS_WAVES; ++k) sum += wave_stats[k][t];
        stats[t] = sum;
    }
}

int launch_sync_rewards(hipStream_t s, const uint32_t* d_aggs, uint32_t n, const uint32_t* d_committee, uint32_t size,
                         uint64_t participant_reward, uint64_t proposer_reward, uint64_t* d_balances, uint64_t* d_stats)
{
    if (n == 0 || n > SYNC_MAX_BATCH || size == 0 || size > SYNC_COMMITTEE_MAX) return -1;
    hipLaunchKernelGGL(k_sync_rewards, dim3(1), dim3(SYNC_REWARDS_WG), 0, s, d_aggs, n, d_committee, size,
                       (unsigned long long)participant_reward, (unsigned long long)proposer_reward,
                       reinterpret_cast<unsigned long long*>(d_balances), reinterpret_cast<unsigned long long*>(d_stats));
    return 0;
}

}  // namespace posevo
