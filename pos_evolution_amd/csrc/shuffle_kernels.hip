// shuffle_kernels.hip -- whole-epoch committee computation on gfx950.
//
// Replaces compute_committee (pe:495-504) over compute_shuffled_index (pe:513-534): the "swap-or-not" shuffle,
// SHUFFLE_ROUND_COUNT rounds, two SHA-256 per index and round in the literal form.  Here:
//   k_shuffle_tables   one SHA-256 per (round, 256-position block) -> the `source` hashes, plus the per-round pivot
//                      (bytes_to_uint64(hash(seed + round)[0:8]) % index_count)
//   k_shuffle_indices  one lane per list position walks its index through all rounds against those tables
//                      (flip, position = max(index, flip), bit (position % 256) of the block hash) and gathers
//                      members[i] = indices[shuffled(i)].
// Both the hash inputs and the bit addressing follow the reference text byte for byte:
//   pivot  = hash(seed + uint_to_bytes(uint8(round)))[0:8]  little-endian            (pe:522)
//   source = hash(seed + uint_to_bytes(uint8(round)) + uint_to_bytes(uint32(position // 256)))   (pe:525-529)
//   byte   = source[(position % 256) // 8] ; bit = (byte >> (position % 8)) % 2        (pe:530-531)
// Integer/hash work, no MFMA.  SURVEY.md 8(f) rank 1.
// Further down: proposer sampling (k_proposer_sample) and the active set the shuffles start from (k_active_compact).
#include "kernels.h"
#include "sample_walk.h"
#include "sha256.h"
#include "wave64.h"

namespace posevo {

// seed: 8 big-endian words.  grid: (n_blocks256 + 1) hashes per round; the extra one (b == n_blocks256) is the pivot.
__global__ void __launch_bounds__(256)
k_shuffle_tables(const uint32_t* __restrict__ seed_be, uint32_t n, uint32_t n_blocks256, uint32_t rounds,
                 uint32_t* __restrict__ source /* [rounds][n_blocks256][8] big-endian words */,
                 uint32_t* __restrict__ pivots /* [rounds] */)
{
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t per_round = (uint64_t)n_blocks256 + 1;
    if (gid >= per_round * rounds) return;
    const uint32_t r = (uint32_t)(gid / per_round);
    const uint32_t b = (uint32_t)(gid % per_round);
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = seed_be[i];
#pragma unroll
    for (int i = 8; i < 16; ++i) w[i] = 0;
    uint32_t dig[8];
    if (b == n_blocks256) {
        // hash(seed + uint8(round)): 33 bytes -> byte 32 = round, 0x80 pad at byte 33, bit length 264
        w[8] = (r << 24) | (0x80u << 16);
        w[15] = 33 * 8;
        sha256_one_block(w, dig);
        // bytes_to_uint64(digest[0:8]) little-endian: digest bytes are the big-endian bytes of dig[0], dig[1]
        const uint64_t lo = __builtin_bswap32(dig[0]), hi = __builtin_bswap32(dig[1]);
        pivots[r] = (uint32_t)(((hi << 32) | lo) % n);
    } else {
        // hash(seed + uint8(round) + uint32_le(b)): 37 bytes; bytes 33..36 = b little-endian, 0x80 at byte 37
        w[8] = (r << 24) | ((b & 0xffu) << 16) | (((b >> 8) & 0xffu) << 8) | ((b >> 16) & 0xffu);
        w[9] = ((b >> 24) << 24) | (0x80u << 16);
        w[15] = 37 * 8;
        sha256_one_block(w, dig);
        uint32_t* dst = source + ((uint64_t)r * n_blocks256 + b) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = dig[i];
    }
}

__global__ void __launch_bounds__(256)
k_shuffle_indices(const uint32_t* __restrict__ source, const uint32_t* __restrict__ pivots, uint32_t n,
                  uint32_t n_blocks256, uint32_t rounds, const uint32_t* __restrict__ indices,
                  uint32_t* __restrict__ members)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t index = i;
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t pivot = pivots[r];
        uint32_t flip = pivot + n - index;  // (pivot + index_count - index) % index_count, operands < n
        if (flip >= n) flip -= n;
        const uint32_t position = max(index, flip);
        // source[(position % 256) // 8]: byte k of the digest = byte (3 - k%4) of big-endian word k/4
        const uint32_t byte_idx = (position & 255u) >> 3;
        const uint32_t word = source[((uint64_t)r * n_blocks256 + (position >> 8)) * 8 + (byte_idx >> 2)];
        const uint32_t byte = (word >> (8 * (3 - (byte_idx & 3)))) & 0xffu;
        const uint32_t bit = (byte >> (position & 7u)) & 1u;
        index = bit ? flip : index;
    }
    members[i] = indices ? indices[index] : index;
}

// The same walk with each round's table in LDS.  The global-memory form above is bound by L2 line requests: every lane
// of a wave reads 4 bytes of a different 128-byte line (after a few rounds the 64 indices of a wave are spread over the
// whole list), 94 M requests per 1 M validators x 90 rounds = 0.3 ms.  But a round touches only HALF of its table:
//   index <= pivot: flip = pivot - index          -> position = max(index, flip) in [ceil(pivot / 2), pivot]
//   index >  pivot: flip = pivot + n - index      -> position                     in [ceil((pivot + n) / 2), n - 1]
// two contiguous ranges of n / 2 positions together = n / 16 bytes of hashes (64 KB per 1 M validators).  One workgroup
// of 1024 lanes x PER indices copies those two ranges into LDS with coalesced 16-byte loads (4x fewer line requests
// than the gather, all of them full lines that the workgroups of an XCD share in its L2), looks its indices up there,
// and goes on to the next round: 2 barriers per round.  Same arithmetic, same result.
constexpr int SHUF_WG = 1024;
constexpr size_t SHUF_LDS_CAP = 96 * 1024;
constexpr int SHUF_NQ = (int)(SHUF_LDS_CAP / 16 / SHUF_WG);  // 16-byte pieces of a round's table per lane: 6

// the two block ranges a round reads, in 256-position blocks
struct ShufRanges { uint32_t a0, len_a, b0, len_b; };
__device__ __forceinline__ ShufRanges shuffle_ranges(uint32_t pivot, uint32_t n)
{
    ShufRanges g;
    g.a0 = ((pivot + 1) >> 1) >> 8;                                  // [ceil(pivot / 2), pivot]
    g.len_a = (pivot >> 8) - g.a0 + 1;
    const uint32_t lo_b = (uint32_t)(((uint64_t)pivot + n + 1) >> 1);  // [ceil((pivot + n) / 2), n - 1]
    g.b0 = min(lo_b, n - 1) >> 8;
    g.len_b = ((n - 1) >> 8) - g.b0 + 1;
    return g;
}

// 16-byte pieces of a round's two ranges in registers: SHUF_NQ = 6 named values per lane (an indexed array, even with
// constant indices after unrolling, was kept in scratch memory by the compiler: 208 B per lane and a 3x slower kernel)
struct ShufPieces { uint4 v0, v1, v2, v3, v4, v5; };
static_assert(SHUF_NQ == 6, "ShufPieces holds six pieces");

__device__ __forceinline__ uint4 shuffle_piece(const uint4* __restrict__ src, const ShufRanges& g, uint32_t qa,
                                               uint32_t total, int j)
{
    const uint32_t q = min(threadIdx.x + j * SHUF_WG, total - 1);  // clamped: an unconditional load of a valid piece
    return src[q < qa ? 2 * (uint64_t)g.a0 + q : 2 * (uint64_t)g.b0 + (q - qa)];
}
__device__ __forceinline__ ShufPieces shuffle_prefetch(const uint32_t* __restrict__ source,
                                                       const uint32_t* __restrict__ pivots, uint32_t r, uint32_t n,
                                                       uint32_t n_blocks256)
{
    const ShufRanges g = shuffle_ranges(pivots[r], n);
    const uint4* src = reinterpret_cast<const uint4*>(source + (uint64_t)r * n_blocks256 * 8);
    const uint32_t qa = 2 * g.len_a, total = qa + 2 * g.len_b;  // 2 x uint4 per 32-byte block
    ShufPieces p;
    p.v0 = shuffle_piece(src, g, qa, total, 0);
    p.v1 = shuffle_piece(src, g, qa, total, 1);
    p.v2 = shuffle_piece(src, g, qa, total, 2);
    p.v3 = shuffle_piece(src, g, qa, total, 3);
    p.v4 = shuffle_piece(src, g, qa, total, 4);
    p.v5 = shuffle_piece(src, g, qa, total, 5);
    return p;
}

template <int PER>
__device__ __forceinline__ void shuffle_round(const ShufPieces p, uint32_t (&index)[PER], uint32_t* tab,
                                              uint32_t pivot, uint32_t n)
{
    const ShufRanges g = shuffle_ranges(pivot, n);
    const uint32_t total = 2 * (g.len_a + g.len_b);
    uint4* dst = reinterpret_cast<uint4*>(tab);
    const uint32_t t = threadIdx.x;
    if (t < total) dst[t] = p.v0;
    if (t + SHUF_WG < total) dst[t + SHUF_WG] = p.v1;
    if (t + 2 * SHUF_WG < total) dst[t + 2 * SHUF_WG] = p.v2;
    if (t + 3 * SHUF_WG < total) dst[t + 3 * SHUF_WG] = p.v3;
    if (t + 4 * SHUF_WG < total) dst[t + 4 * SHUF_WG] = p.v4;
    if (t + 5 * SHUF_WG < total) dst[t + 5 * SHUF_WG] = p.v5;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const uint32_t idx = index[k];
        uint32_t flip = pivot + n - idx;
        if (flip >= n) flip -= n;
        const uint32_t position = min(max(idx, flip), n - 1);  // idx >= n (padding lanes) stays harmless
        const uint32_t blk = position >> 8;
        const uint32_t lb = position <= pivot ? blk - g.a0 : g.len_a + (blk - g.b0);
        const uint32_t byte_idx = (position & 255u) >> 3;
        const uint32_t word = tab[lb * 8 + (byte_idx >> 2)];
        const uint32_t byte = (word >> (8 * (3 - (byte_idx & 3)))) & 0xffu;
        index[k] = (idx < n && ((byte >> (position & 7u)) & 1u)) ? flip : idx;
    }
}

template <int PER>
__global__ void __launch_bounds__(SHUF_WG)
k_shuffle_indices_lds(const uint32_t* __restrict__ source, const uint32_t* __restrict__ pivots, uint32_t n,
                      uint32_t n_blocks256, uint32_t rounds, const uint32_t* __restrict__ indices,
                      uint32_t* __restrict__ members)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t tab[];  // [blocks of range A | blocks of range B] x 8 words
    const uint32_t base = blockIdx.x * (SHUF_WG * PER) + threadIdx.x;
    uint32_t index[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) index[k] = base + k * SHUF_WG;  // lane-contiguous per k: coalesced final store
    // The tables of the next TWO rounds travel from L2 into registers while this round's lookups run from LDS: a round
    // costs an LDS write, two barriers and PER lookups instead of an exposed L2 round trip.
    ShufPieces p0 = shuffle_prefetch(source, pivots, 0, n, n_blocks256);
    ShufPieces p1 = shuffle_prefetch(source, pivots, rounds > 1 ? 1 : 0, n, n_blocks256);
    for (uint32_t r = 0; r < rounds; r += 2) {
        shuffle_round<PER>(p0, index, tab, pivots[r], n);
        p0 = shuffle_prefetch(source, pivots, min(r + 2, rounds - 1), n, n_blocks256);
        __syncthreads();  // the table is overwritten by the next round
        if (r + 1 < rounds) {
            shuffle_round<PER>(p1, index, tab, pivots[r + 1], n);
            p1 = shuffle_prefetch(source, pivots, min(r + 3, rounds - 1), n, n_blocks256);
            __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const uint32_t i = base + k * SHUF_WG;
        if (i < n) members[i] = indices ? indices[index[k]] : index[k];
    }
}

int launch_shuffle(hipStream_t s, const uint32_t* d_seed_be, uint32_t n, uint32_t rounds, uint32_t* d_source,
                   uint32_t* d_pivots, const uint32_t* d_indices, uint32_t* d_members)
{
    if (n == 0) return 0;
    const uint32_t nb = (n + 255) / 256;
    const uint64_t hashes = ((uint64_t)nb + 1) * rounds;
    if (hashes)
        hipLaunchKernelGGL(k_shuffle_tables, dim3((unsigned)((hashes + 255) / 256)), dim3(256), 0, s, d_seed_be, n, nb,
                           rounds, d_source, d_pivots);
    // the LDS form needs n / 16 bytes (+ the ragged ends) of LDS: up to ~1.5 M indices inside 96 KB; larger (and tiny) lists
    // take the gather
    const size_t lds_bytes = 32ull * ((size_t)nb / 2 + 4);
    constexpr size_t LDS_CAP = SHUF_LDS_CAP;
    if (lds_bytes <= LDS_CAP && n >= 4096 && rounds > 0) {
        constexpr int PER = 4;
        if (first_use_on_this_device<4242>())
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_shuffle_indices_lds<PER>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CAP);
        hipLaunchKernelGGL(k_shuffle_indices_lds<PER>, dim3((n + SHUF_WG * PER - 1) / (SHUF_WG * PER)), dim3(SHUF_WG), lds_bytes,
                           s, d_source, d_pivots, n, nb, rounds, d_indices, d_members);
        return 0;
    }
    hipLaunchKernelGGL(k_shuffle_indices, dim3((n + 255) / 256), dim3(256), 0, s, d_source, d_pivots, n, nb, rounds,
                       d_indices, d_members);
    return 0;
}

// ------------------------------------------------------------------ proposer sampling
// compute_proposer_index (pe:604-618): for i = 0, 1, ... the candidate indices[compute_shuffled_index(i % total, total, seed)]
// is accepted iff effective_balance * 255 >= MAX_EFFECTIVE_BALANCE * hash(seed + uint64_le(i // 32))[i % 32].
// One wave per seed.  Phase 1: the round pivots, once per seed, into LDS (lane r, r + 64, ...).  Phase 2: batches of 64
// candidates, lane l of batch b takes i = 64 b + l, walks i % total through all rounds and computes each round's `source`
// hash for its own position // 256 on the spot (one compression per round and lane; 64 candidates touch at most 64 of the
// blocks a table in memory would hold), then the random byte's hash; a ballot picks the lowest accepting lane.  The loop's
// exit is wave-uniform and bounded by max_tries: a registry that never accepts ends in NONE32.
constexpr int PROP_WAVE = 64;
// (the candidate's walk, its random byte and the acceptance rule: sample_walk.h, shared with k_sync_sample)

__global__ void __launch_bounds__(PROP_WAVE)
k_proposer_sample(const uint32_t* __restrict__ seeds_be /* [n_seeds][8] big-endian words */, uint32_t total,
                  uint32_t rounds, const uint32_t* __restrict__ indices /* [total] or null = identity */,
                  const unsigned long long* __restrict__ eff_balance, unsigned long long max_eff, uint32_t max_tries,
                  uint32_t* __restrict__ out_proposer, uint32_t* __restrict__ out_tries)
{
    __shared__ uint32_t pivots[PROP_MAX_ROUNDS];
    const uint32_t lane = threadIdx.x;
    const uint32_t* seed = seeds_be + 8ull * blockIdx.x;
    uint32_t w[16];
    uint32_t dig[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = seed[k];
    // ---- phase 1: the round pivots
    for (uint32_t r = lane; r < rounds; r += PROP_WAVE) pivots[r] = sample_pivot(w, dig, r, total);
    __syncthreads();
    // ---- phase 2
    const uint32_t n_batches = (uint32_t)(((uint64_t)max_tries + PROP_WAVE - 1) / PROP_WAVE);
    for (uint32_t b = 0; b < n_batches; ++b) {
        const uint64_t i = (uint64_t)b * PROP_WAVE + lane;
        const uint32_t index = sample_walk(w, dig, pivots, rounds, total, i);
        const unsigned long long random_byte = sample_random_byte(w, dig, i);
        const uint32_t candidate = indices ? indices[index] : index;
        const unsigned long long eb = eff_balance[candidate];
        const bool accept = i < max_tries && sample_accepts(eb, max_eff, random_byte);
        const unsigned long long ballot = __ballot(accept);
        if (ballot) {  // wave-uniform
            if (lane == (uint32_t)__builtin_ctzll(ballot)) {
                out_proposer[blockIdx.x] = candidate;
                out_tries[blockIdx.x] = (uint32_t)i;
            }
            return;
        }
    }
    if (lane == 0) {
        out_proposer[blockIdx.x] = NONE32;
        out_tries[blockIdx.x] = max_tries;
    }
}

void launch_proposer_sample(hipStream_t s, const uint32_t* d_seeds_be, uint32_t n_seeds, uint32_t total, uint32_t rounds,
                            const uint32_t* d_indices, const uint64_t* d_eff_balance, uint64_t max_eff, uint32_t max_tries,
                            uint32_t* d_out_proposer, uint32_t* d_out_tries)
{
    if (n_seeds == 0 || total == 0 || rounds >= PROP_MAX_ROUNDS) return;
    hipLaunchKernelGGL(k_proposer_sample, dim3(n_seeds), dim3(PROP_WAVE), 0, s, d_seeds_be, total, rounds, d_indices,
                       reinterpret_cast<const unsigned long long*>(d_eff_balance), (unsigned long long)max_eff, max_tries,
                       d_out_proposer, d_out_tries);
}

// ------------------------------------------------------------------ active set
// get_active_validator_indices(state, epoch): every v with activation_epoch[v] <= epoch < exit_epoch[v] (is_active_validator;
// both comparisons unsigned 64-bit, FAR_FUTURE_EPOCH = 2^64 - 1 is an ordinary value), in increasing order of v, with
// len(...) and the effective-balance sum get_total_balance needs.  Three launches on one stream:
//   k_active_compact<false>  one lane per validator, ACTIVE_WG of them per workgroup: the two epochs (coalesced 8-byte loads),
//                            a wave64 ballot, its popcount and the wave's balance sum; the four waves meet in LDS ->
//                            wg_count[b], wg_balance[b]
//   k_active_scan            one workgroup walks the counts ACTIVE_SCAN_TILE at a time: exclusive offsets, the total count
//                            and the total balance
//   k_active_compact<true>   the same ballot again; rank in the wave = mbcnt(ballot), the wave's base = the offset of the
//                            workgroup + the counts of the waves before it -> out_indices[base + rank] = v
// No atomics and no waiting of one workgroup for another: the order of the output is fixed by construction, and the
// integer sums are exact in any order.  The second pass re-reads the epochs (16 B per validator).
constexpr int ACTIVE_WAVES = ACTIVE_WG / 64;
static_assert(ACTIVE_WG % 64 == 0 && ACTIVE_SCAN_TILE % 64 == 0, "whole waves");

__device__ __forceinline__ bool is_active_validator(unsigned long long activation_epoch, unsigned long long exit_epoch,
                                                    unsigned long long epoch)
{
    return activation_epoch <= epoch && epoch < exit_epoch;
}

template <bool SCATTER>
__global__ void __launch_bounds__(ACTIVE_WG)
k_active_compact(const unsigned long long* __restrict__ activation_epoch, const unsigned long long* __restrict__ exit_epoch,
                 unsigned long long epoch, const unsigned long long* __restrict__ eff_balance, uint64_t n_val,
                 uint32_t* __restrict__ wg_count, unsigned long long* __restrict__ wg_balance,
                 const uint32_t* __restrict__ wg_offset, uint32_t* __restrict__ out_indices)
{
    __shared__ uint32_t wave_count[ACTIVE_WAVES];
    __shared__ unsigned long long wave_balance[ACTIVE_WAVES];
    const uint64_t v = (uint64_t)blockIdx.x * ACTIVE_WG + threadIdx.x;
    const uint32_t wave = threadIdx.x >> 6;
    const bool active = v < n_val && is_active_validator(activation_epoch[v], exit_epoch[v], epoch);
    const unsigned long long ballot = __ballot(active);
    if constexpr (!SCATTER) {
        const unsigned long long balance = wave_sum(active ? eff_balance[v] : 0ull);
        if ((threadIdx.x & 63) == 0) {
            wave_count[wave] = (uint32_t)__builtin_popcountll(ballot);
            wave_balance[wave] = balance;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t count = 0;
            unsigned long long sum = 0;
#pragma unroll
            for (int w = 0; w < ACTIVE_WAVES; ++w) { count += wave_count[w]; sum += wave_balance[w]; }
            wg_count[blockIdx.x] = count;
            wg_balance[blockIdx.x] = sum;
        }
    } else {
        if ((threadIdx.x & 63) == 0) wave_count[wave] = (uint32_t)__builtin_popcountll(ballot);
        __syncthreads();
        uint32_t base = wg_offset[blockIdx.x];
#pragma unroll
        for (int w = 0; w < ACTIVE_WAVES; ++w) base += (uint32_t)w < wave ? wave_count[w] : 0u;
        // active lanes below this one in the wave
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
        if (active) out_indices[base + rank] = (uint32_t)v;  // base + rank < the total count <= n_val
    }
}

// grid: ONE workgroup.  carry is uniform across it; the loop's trip count depends on n_wg alone.
__global__ void __launch_bounds__(ACTIVE_SCAN_TILE)
k_active_scan(const uint32_t* __restrict__ wg_count, const unsigned long long* __restrict__ wg_balance, uint32_t n_wg,
              uint32_t* __restrict__ wg_offset, ActiveTotals* __restrict__ totals)
{
    constexpr int WAVES = ACTIVE_SCAN_TILE / 64;
    __shared__ uint32_t wave_total[WAVES];
    __shared__ unsigned long long wave_balance[WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    unsigned long long balance = 0;
    for (uint32_t tile = 0; tile < n_wg; tile += ACTIVE_SCAN_TILE) {
        const uint32_t i = tile + threadIdx.x;
        const uint32_t count = i < n_wg ? wg_count[i] : 0u;
        if (i < n_wg) balance += wg_balance[i];
        uint32_t inclusive = count;  // prefix sum over the wave (not wave_incl_scan: the kernel's code differs)
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
    balance = wave_sum(balance);
    if (lane == 0) wave_balance[wave] = balance;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) sum += wave_balance[w];
        totals->balance = sum;
        totals->n_active = carry;
        totals->pad = 0;
    }
}

// scratch: wg_balance u64[n_wg] | wg_count u32[n_wg] | wg_offset u32[n_wg]
static uint32_t active_workgroups(uint64_t n_val) { return (uint32_t)((n_val + ACTIVE_WG - 1) / ACTIVE_WG); }
size_t active_scratch_bytes(uint64_t n_val) { return 16ull * active_workgroups(n_val); }

void launch_active_compact(hipStream_t s, const uint64_t* d_activation_epoch, const uint64_t* d_exit_epoch, uint64_t epoch,
                           const uint64_t* d_eff_balance, uint64_t n_val, void* d_wg, uint32_t* d_out_indices,
                           ActiveTotals* d_totals)
{
    if (n_val == 0) return;
    const uint32_t n_wg = active_workgroups(n_val);
    unsigned long long* wg_balance = static_cast<unsigned long long*>(d_wg);
    uint32_t* wg_count = reinterpret_cast<uint32_t*>(wg_balance + n_wg);
    uint32_t* wg_offset = wg_count + n_wg;
    const unsigned long long* act = reinterpret_cast<const unsigned long long*>(d_activation_epoch);
    const unsigned long long* ext = reinterpret_cast<const unsigned long long*>(d_exit_epoch);
    const unsigned long long* bal = reinterpret_cast<const unsigned long long*>(d_eff_balance);
    hipLaunchKernelGGL(k_active_compact<false>, dim3(n_wg), dim3(ACTIVE_WG), 0, s, act, ext, (unsigned long long)epoch, bal,
                       n_val, wg_count, wg_balance, (const uint32_t*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_active_scan, dim3(1), dim3(ACTIVE_SCAN_TILE), 0, s, wg_count, wg_balance, n_wg, wg_offset, d_totals);
    hipLaunchKernelGGL(k_active_compact<true>, dim3(n_wg), dim3(ACTIVE_WG), 0, s, act, ext, (unsigned long long)epoch, bal,
                       n_val, (uint32_t*)nullptr, (unsigned long long*)nullptr, wg_offset, d_out_indices);
}

// PE_VAL_ACTIVE (0x01) = activity at current_epoch, PE_VAL_ACTIVE_PREV (0x08) = activity at previous_epoch; the other bits stay.
__global__ void __launch_bounds__(256)
k_activity_flags(const unsigned long long* __restrict__ activation_epoch, const unsigned long long* __restrict__ exit_epoch,
                 unsigned long long current_epoch, unsigned long long previous_epoch, uint64_t n_val,
                 uint8_t* __restrict__ sflags)
{
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_val) return;
    const unsigned long long a = activation_epoch[v], x = exit_epoch[v];
    const uint32_t f = sflags[v] & ~0x09u;
    sflags[v] = (uint8_t)(f | (is_active_validator(a, x, current_epoch) ? 0x01u : 0u) |
                          (is_active_validator(a, x, previous_epoch) ? 0x08u : 0u));
}
void launch_activity_flags(hipStream_t s, const uint64_t* d_activation_epoch, const uint64_t* d_exit_epoch,
                           uint64_t current_epoch, uint64_t previous_epoch, uint64_t n_val, uint8_t* sflags)
{
    if (n_val == 0) return;
    hipLaunchKernelGGL(k_activity_flags, dim3((unsigned)((n_val + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(d_activation_epoch),
                       reinterpret_cast<const unsigned long long*>(d_exit_epoch), (unsigned long long)current_epoch,
                       (unsigned long long)previous_epoch, n_val, sflags);
}

}  // namespace posevo
