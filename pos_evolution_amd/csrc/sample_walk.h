// sample_walk.h -- one candidate of compute_proposer_index's loop (pe:604-618), the text k_proposer_sample
// (shuffle_kernels.hip) and k_sync_sample (sync_kernels.hip) share: for a given i the candidate is
// indices[compute_shuffled_index(i % total, total, seed)], accepted iff
// effective_balance * 255 >= MAX_EFFECTIVE_BALANCE * hash(seed + uint64_le(i // 32))[i % 32].
// Every function takes the lane's message block w with w[0..7] = the seed's 8 big-endian words, rewrites w[8..15] and
// leaves the seed in place.  dig is the lane's ONE digest buffer, shared by all three functions and overwritten by each: a
// caller declares it once, beside w.  The round pivots are the caller's (LDS): sample_pivot makes one.
#pragma once
#include <stdint.h>

#include "sha256.h"

namespace posevo {

constexpr uint32_t PROP_MAX_ROUNDS = 256;  // shuffle_round_count is a uint8 in the spec

// byte k (0..31) of a digest held as 8 big-endian words, without indexing the array by a run-time value
__device__ __forceinline__ uint32_t digest_byte(const uint32_t (&dig)[8], uint32_t k)
{
    const uint32_t j = k >> 2;
    uint32_t word = dig[0];
    word = j == 1 ? dig[1] : word;
    word = j == 2 ? dig[2] : word;
    word = j == 3 ? dig[3] : word;
    word = j == 4 ? dig[4] : word;
    word = j == 5 ? dig[5] : word;
    word = j == 6 ? dig[6] : word;
    word = j == 7 ? dig[7] : word;
    return (word >> (8 * (3 - (k & 3)))) & 0xffu;
}

// pivot[r] = bytes_to_uint64(hash(seed + uint8(r))[0:8]) % total   (pe:522)
__device__ __forceinline__ uint32_t sample_pivot(uint32_t (&w)[16], uint32_t (&dig)[8], uint32_t r, uint32_t total)
{
    w[8] = (r << 24) | (0x80u << 16);
#pragma unroll
    for (int k = 9; k < 15; ++k) w[k] = 0;
    w[15] = 33 * 8;
    sha256_one_block(w, dig);
    const uint64_t lo = __builtin_bswap32(dig[0]), hi = __builtin_bswap32(dig[1]);
    return (uint32_t)(((hi << 32) | lo) % total);
}

// compute_shuffled_index(i % total, total, seed): each round's `source` hash computed on the spot for the lane's own
// position // 256 (one compression per round and lane)
__device__ __forceinline__ uint32_t sample_walk(uint32_t (&w)[16], uint32_t (&dig)[8], const uint32_t* pivots, uint32_t rounds,
                                                uint32_t total, uint64_t i)
{
    uint32_t index = (uint32_t)(i % total);
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t pivot = pivots[r];
        uint32_t flip = pivot + total - index;  // (pivot + index_count - index) % index_count, operands < total
        if (flip >= total) flip -= total;
        const uint32_t position = max(index, flip);
        const uint32_t blk = position >> 8;
        // source = hash(seed + uint8(r) + uint32_le(position // 256)): 37 bytes   (pe:525-529)
        w[8] = (r << 24) | ((blk & 0xffu) << 16) | (((blk >> 8) & 0xffu) << 8) | ((blk >> 16) & 0xffu);
        w[9] = ((blk >> 24) << 24) | (0x80u << 16);
#pragma unroll
        for (int k = 10; k < 15; ++k) w[k] = 0;
        w[15] = 37 * 8;
        sha256_one_block(w, dig);
        const uint32_t byte = digest_byte(dig, (position & 255u) >> 3);
        index = ((byte >> (position & 7u)) & 1u) ? flip : index;
    }
    return index;
}

// random_byte = hash(seed + uint64_le(i // 32))[i % 32]: 40 bytes   (pe:614)
__device__ __forceinline__ unsigned long long sample_random_byte(uint32_t (&w)[16], uint32_t (&dig)[8], uint64_t i)
{
    const uint64_t q = i >> 5;
    w[8] = __builtin_bswap32((uint32_t)q);
    w[9] = __builtin_bswap32((uint32_t)(q >> 32));
    w[10] = 0x80000000u;
#pragma unroll
    for (int k = 11; k < 15; ++k) w[k] = 0;
    w[15] = 40 * 8;
    sha256_one_block(w, dig);
    return digest_byte(dig, (uint32_t)(i & 31u));
}

// effective_balance * 255 >= MAX_EFFECTIVE_BALANCE * random_byte over the whole u64 range: 128-bit products
__device__ __forceinline__ bool sample_accepts(unsigned long long eb, unsigned long long max_eff, unsigned long long random_byte)
{
    const unsigned long long l_hi = __umul64hi(eb, 255ull), l_lo = eb * 255ull;
    const unsigned long long r_hi = __umul64hi(max_eff, random_byte), r_lo = max_eff * random_byte;
    return l_hi > r_hi || (l_hi == r_hi && l_lo >= r_lo);
}

}  // namespace posevo
