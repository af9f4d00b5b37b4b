// ssz_kernels.hip -- SSZ hash_tree_root of the resident per-validator lists, for gfx950.
// The reference names hash_tree_root (pe:142, 423, 1016) and holds no text of it; the conventions are the SSZ
// specification's [UPSTREAM-MEMORY]: 32-byte chunks, basic values packed little-endian with the last chunk zero-padded,
// Z[0] = 0^32 and Z[k + 1] = H(Z[k] || Z[k]), merkleize(chunks, depth) = the root of the 2^depth-leaf tree whose absent
// leaves are Z[0].
//   k_ssz_merkle           T nodes of one height -> one node log2 T higher, per workgroup, through a tile in LDS
//   k_ssz_validator_roots  hash_tree_root(Validator) (pe:36-45), one lane per validator, 7 hashes
//   k_ssz_pubkey_roots     the 48 -> 32-byte pubkey leaf, once per registry
// Every hash is sha256_64 (sha256.h): 64 bytes in, two compressions, the second over a constant schedule.  Integer work,
// about 3 400 VALU operations per hash against 64 bytes read: nothing here is bound by memory, no MFMA, no scratch (the
// Makefile keeps the compiler's resource report, tests/test_ssz_model.py reads it).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "sha256.h"

namespace posevo {

namespace {

constexpr uint32_t SSZ_VAL_SLASHED = 0x02u;  // PE_VAL_SLASHED (include/posevo.h)

// a uint64 as the first 8 bytes of a chunk: little-endian bytes, read as two big-endian words
__device__ __forceinline__ void u64_leaf(unsigned long long v, uint32_t* w)
{
    w[0] = __builtin_bswap32((uint32_t)v);
    w[1] = __builtin_bswap32((uint32_t)(v >> 32));
#pragma unroll
    for (int k = 2; k < 8; ++k) w[k] = 0;
}

}  // namespace

// LDS: the tile, word-major -- word k of node i at lds[k * S + i], S = tile + 4: the staging writes of a 32-lane half (4 nodes x
// 8 words) then fall on 32 different banks, and a level's reads (nodes 2p, 2p + 1 of one word) are 8-byte reads side by side.
// Each level halves the tile in place: every lane reads its two children, all lanes meet, every lane writes its parent.
// blockDim.x = max(64, tile / 2): one parent per lane at the widest level.
template <bool RAW>
__global__ void __launch_bounds__(512)
k_ssz_merkle(const uint32_t* __restrict__ src, uint64_t n_bytes, uint32_t base, uint32_t levels,
             const uint32_t* __restrict__ zero_words, uint32_t* __restrict__ out)
{
    extern __shared__ uint32_t lds[];
    const uint32_t tile = 1u << levels, S = tile + 4;
    const uint64_t first_node = (uint64_t)blockIdx.x << levels;
    for (uint32_t w = threadIdx.x; w < tile * 8; w += blockDim.x) {
        const uint64_t gw = first_node * 8 + w, off = gw * 4;
        uint32_t v = 0;
        if (off < n_bytes) {  // nothing at or beyond n_bytes is trusted: not the allocation's tail, not a longer list's remains
            v = src[gw];
            if (RAW) {
                const uint64_t rem = n_bytes - off;
                if (rem < 4) v &= (1u << (8 * (uint32_t)rem)) - 1u;
                v = __builtin_bswap32(v);
            }
        }
        lds[(w & 7) * S + (w >> 3)] = v;
    }
    const uint64_t m = (n_bytes + 31) / 32 - first_node;  // the grid has a workgroup only where this is >= 1
    uint32_t count = m < tile ? (uint32_t)m : tile;
    __syncthreads();
    for (uint32_t j = 0; j < levels; ++j) {
        const uint32_t parents = (count + 1) >> 1, p = threadIdx.x;
        uint32_t node[8];
        if (p < parents) {
            uint32_t msg[16];
#pragma unroll
            for (int k = 0; k < 8; ++k) msg[k] = lds[k * S + 2 * p];
            if (2 * p + 1 < count) {
#pragma unroll
                for (int k = 0; k < 8; ++k) msg[8 + k] = lds[k * S + 2 * p + 1];
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) msg[8 + k] = zero_words[(base + j) * 8 + k];
            }
            sha256_64(msg, node);
        }
        __syncthreads();
        if (p < parents) {
#pragma unroll
            for (int k = 0; k < 8; ++k) lds[k * S + p] = node[k];
        }
        __syncthreads();
        count = parents;
    }
    if (threadIdx.x < 8) out[(uint64_t)blockIdx.x * 8 + threadIdx.x] = lds[threadIdx.x * S];
}

void launch_ssz_merkle(hipStream_t s, const void* src, uint64_t n_bytes, int raw, uint32_t base, uint32_t levels,
                       const uint32_t* zero_words, uint32_t* out)
{
    const uint64_t m = (n_bytes + 31) / 32, tile = 1ull << levels;
    if (m == 0 || levels > SSZ_TILE_LOG2) return;
    const unsigned grid = (unsigned)((m + tile - 1) / tile);
    const unsigned lanes = (unsigned)std::max<uint64_t>(64, tile / 2);
    const size_t lds_bytes = 4 * 8 * (size_t)(tile + 4);
    if (raw)
        hipLaunchKernelGGL(k_ssz_merkle<true>, dim3(grid), dim3(lanes), lds_bytes, s, static_cast<const uint32_t*>(src), n_bytes,
                           base, levels, zero_words, out);
    else
        hipLaunchKernelGGL(k_ssz_merkle<false>, dim3(grid), dim3(lanes), lds_bytes, s, static_cast<const uint32_t*>(src), n_bytes,
                           base, levels, zero_words, out);
}

__global__ void __launch_bounds__(256)
k_ssz_pubkey_roots(const uint32_t* __restrict__ pk, uint64_t n, uint32_t* __restrict__ out)
{
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    uint32_t msg[16], dig[8];
#pragma unroll
    for (int k = 0; k < 12; ++k) msg[k] = __builtin_bswap32(pk[v * 12 + k]);  // 48 bytes: chunk 0 and half of chunk 1
#pragma unroll
    for (int k = 12; k < 16; ++k) msg[k] = 0;
    sha256_64(msg, dig);
#pragma unroll
    for (int k = 0; k < 8; ++k) out[v * 8 + k] = __builtin_bswap32(dig[k]);
}

void launch_ssz_pubkey_roots(hipStream_t s, const uint8_t* pubkeys48, uint64_t n, uint8_t* out_leaves32)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_ssz_pubkey_roots, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const uint32_t*>(pubkeys48), n, reinterpret_cast<uint32_t*>(out_leaves32));
}

// The depth-3 tree over the 8 field leaves: hashes 0 .. 3 pair the leaves, 4 and 5 pair those, 6 is the root.  ONE copy of
// the unrolled hash in a loop of 7 (seven copies would be ~170 KB of code); a lane's four level-1 nodes wait in its own
// column of LDS -- lds[(slot * 8 + k) * 256 + lane], no lane reads another's, so no barrier -- and each later hash overwrites
// a slot it has already read (4: reads 0, 1, writes 0; 5: reads 2, 3, writes 1; 6: reads 0, 1).
__global__ void __launch_bounds__(256)
k_ssz_validator_roots(const SszValidatorArgs a)
{
    __shared__ uint32_t lds[4 * 8 * 256];
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n_val) return;
    const unsigned long long* eff = reinterpret_cast<const unsigned long long*>(a.effective_balance);
    const unsigned long long* elig = reinterpret_cast<const unsigned long long*>(a.activation_eligibility_epoch);
    const unsigned long long* act = reinterpret_cast<const unsigned long long*>(a.activation_epoch);
    const unsigned long long* ext = reinterpret_cast<const unsigned long long*>(a.exit_epoch);
    const unsigned long long* wdr = reinterpret_cast<const unsigned long long*>(a.withdrawable_epoch);
    const uint32_t* pkl = reinterpret_cast<const uint32_t*>(a.pubkey_leaf32);
    const uint32_t* wc = reinterpret_cast<const uint32_t*>(a.withdrawal_credentials32);
    uint32_t* col = lds + threadIdx.x;
    uint32_t dig[8];
#pragma unroll 1
    for (int i = 0; i < 7; ++i) {
        uint32_t msg[16];
        if (i == 0) {         // pubkey | withdrawal_credentials
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                msg[k] = __builtin_bswap32(pkl[v * 8 + k]);
                msg[8 + k] = __builtin_bswap32(wc[v * 8 + k]);
            }
        } else if (i == 1) {  // effective_balance | slashed
            u64_leaf(eff[v], msg);
#pragma unroll
            for (int k = 8; k < 16; ++k) msg[k] = 0;
            msg[8] = (a.sflags[v] & SSZ_VAL_SLASHED) ? 0x01000000u : 0u;
        } else if (i == 2) {  // activation_eligibility_epoch | activation_epoch
            u64_leaf(elig[v], msg);
            u64_leaf(act[v], msg + 8);
        } else if (i == 3) {  // exit_epoch | withdrawable_epoch
            u64_leaf(ext[v], msg);
            u64_leaf(wdr[v], msg + 8);
        } else {
            const int left = i == 5 ? 2 : 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                msg[k] = col[(left * 8 + k) * 256];
                msg[8 + k] = col[((left + 1) * 8 + k) * 256];
            }
        }
        sha256_64(msg, dig);
        const int slot = i < 4 ? i : i - 4;
        if (i < 6) {
#pragma unroll
            for (int k = 0; k < 8; ++k) col[(slot * 8 + k) * 256] = dig[k];
        }
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.out_roots32) + v * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = __builtin_bswap32(dig[k]);
}

void launch_ssz_validator_roots(hipStream_t s, const SszValidatorArgs& a)
{
    if (a.n_val == 0) return;
    hipLaunchKernelGGL(k_ssz_validator_roots, dim3((unsigned)((a.n_val + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace posevo
