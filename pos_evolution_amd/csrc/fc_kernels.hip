// fc_kernels.hip -- LMD-GHOST fork-choice and attestation bookkeeping kernels for gfx950.
//
//   k_votes          get_latest_attesting_balance's O(V) part (called from
//                    get_head pe:1116): stream vote/balance/flags (13 B per validator),
//                    LDS-privatised u64 histogram per workgroup, non-zero bins flushed
//                    with one global atomic each; also the active-balance totals the
//                    proposer boost needs.
//   k_tree           one workgroup, block tree resident in LDS in DFS pre-order:
//                    subtree weight = prefix-sum difference (pe:322: "B or descendants
//                    of B"), filter_block_tree viability (A.3) from a second scan,
//                    best child by (weight, root) (pe:1114-1116), then pointer jumping
//                    replaces the sequential descent of pe:1107-1116.
//   k_votes_remap    pe_prune: the latest messages' block indices follow the re-rooted block table
//                    (old index -> new index through a map staged in LDS).
//   k_lmd_*          update_latest_messages (pe:1435-1441) for a whole batch with the
//                    sequential semantics kept by a 64-bit atomicMax on (epoch+1, ~order).
//   k_participation  the flag loop of process_attestation (pe:744-749).
//   k_bits_union     aggregation_bits = OR (validator guide; pe:715, pe:730), popcount by
//                    wave reduction.
//
// The kernels here and their launchers; the bodies of votes, tree and bits_union are device functions in fc_bodies.inc,
// which pair_kernels.hip runs as block ranges of its paired launches as well.
//
// All of this is HBM/latency-bound integer work; no MFMA.
#include <cstdlib>
#include "fc_bodies.inc"

namespace posevo {

// ------------------------------------------------------------------ votes
template <int QUADS>
__global__ void __launch_bounds__(VOTES_WG)
k_votes(const VotesArgs a)
{
    POSEVO_FC_PRIO();
    extern __shared__ __attribute__((aligned(16))) unsigned long long hist[];  // n_blocks bins, by insertion index
    votes_body<QUADS>(blockIdx.x, gridDim.x, a, hist);
}

// A caller-owned exchange buffer (pe_votes_partial) has to read zero before k_votes adds into it; the engine's own buffers
// are kept zeroed by k_tree.
void votes_clear_exchange(hipStream_t s, uint64_t* direct, uint32_t n_blocks, VoteTotals* totals)
{
    (void)hipMemsetAsync(direct, 0, sizeof(uint64_t) * n_blocks, s);
    (void)hipMemsetAsync(totals, 0, sizeof(VoteTotals) * VOTES_MAX_WG, s);
}

void launch_votes(hipStream_t s, const VotesArgs& a, int lean)
{
    if (a.n_val == 0) return;
    // votes_blocks: few, fat workgroups.  Round 3 re-measured the alternatives against the 33.7 us p50 of this shape: eight
    // flush rows (workgroup w adds into row w % 8, k_tree sums the rows) with 256 workgroups 40.8 us; four quads in flight
    // per lane 30.0 vs 30.2 us (nothing); k_tree launched BESIDE k_votes on a second stream and released by a device-side
    // ticket 70 us -- the cross-stream event that keeps the next call ordered costs more than the launch gap it removes
    // (profiles/README.md).
    const unsigned blocks = votes_blocks(a.n_val);
    if (first_use_on_this_device<0>()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_votes<2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(uint64_t) * TREE_MAX_BLOCKS));
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_votes<1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(uint64_t) * TREE_MAX_BLOCKS));
    }
    if (lean)
        hipLaunchKernelGGL(k_votes<1>, dim3(blocks), dim3(VOTES_WG), sizeof(uint64_t) * a.n_blocks, s, a);
    else
        hipLaunchKernelGGL(k_votes<2>, dim3(blocks), dim3(VOTES_WG), sizeof(uint64_t) * a.n_blocks, s, a);
}

// ------------------------------------------------------------------ votes remap (pe_prune)
// The block table has been re-rooted at the finalized root: a latest message's block index goes through the map old
// insertion index -> new one.  NONE32 (no message), VOTE_PRUNED (orphaned by an earlier prune) and anything else
// >= n_old stay as they are; vote_key and vote_slot are not touched (a message keeps its epoch and slot).
__device__ __forceinline__ uint32_t remap_one(const uint32_t x, const uint32_t* __restrict__ lmap, const uint32_t n_old,
                                              uint32_t& remapped, uint32_t& orphaned)
{
    if (x >= n_old) return x;
    const uint32_t y = lmap[x];
    orphaned += y == VOTE_PRUNED ? 1u : 0u;  // sums, not a branch between the two counters: they stay in registers
    remapped += (y != VOTE_PRUNED && y != x) ? 1u : 0u;
    return y;
}

__global__ void __launch_bounds__(REMAP_WG)
k_votes_remap(const RemapArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lmap[];  // n_old entries (<= 32 KB)
    uint32_t* __restrict__ vote_block = a.vote_block;
    const uint64_t n_val = a.n_val;
    const uint32_t n_old = a.n_old;
    for (uint32_t b = threadIdx.x; b < n_old; b += REMAP_WG) lmap[b] = a.map[b];
    __syncthreads();
    uint32_t remapped = 0, orphaned = 0;
    const uint64_t n_quads = (n_val + 3) / 4;
    const uint64_t stride = (uint64_t)gridDim.x * REMAP_WG;
    for (uint64_t q = (uint64_t)blockIdx.x * REMAP_WG + threadIdx.x; q < n_quads; q += stride) {
        const uint64_t v0 = q * 4;
        if (v0 + 4 <= n_val) {  // the array is 16-byte aligned and v0 % 4 == 0
            const uint4 t = *reinterpret_cast<const uint4*>(vote_block + v0);
            const uint32_t x = remap_one(t.x, lmap, n_old, remapped, orphaned);
            const uint32_t y = remap_one(t.y, lmap, n_old, remapped, orphaned);
            const uint32_t z = remap_one(t.z, lmap, n_old, remapped, orphaned);
            const uint32_t w = remap_one(t.w, lmap, n_old, remapped, orphaned);
            *reinterpret_cast<uint4*>(vote_block + v0) = make_uint4(x, y, z, w);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (v0 + k < n_val) vote_block[v0 + k] = remap_one(vote_block[v0 + k], lmap, n_old, remapped, orphaned);
        }
    }
    // wave reduce -> LDS -> one device atomic per workgroup and count
    __shared__ uint32_t wg_cnt[2];
    if (threadIdx.x == 0) { wg_cnt[0] = 0; wg_cnt[1] = 0; }
    remapped = wave_sum(remapped);
    orphaned = wave_sum(orphaned);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        if (remapped) atomicAdd(&wg_cnt[0], remapped);
        if (orphaned) atomicAdd(&wg_cnt[1], orphaned);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (wg_cnt[0]) atomicAdd(a.counts, (unsigned long long)wg_cnt[0]);
        if (wg_cnt[1]) atomicAdd(a.counts + 1, (unsigned long long)wg_cnt[1]);
    }
}

void launch_votes_remap(hipStream_t s, const RemapArgs& a)
{
    if (a.n_val == 0 || a.n_old == 0 || a.n_old > (uint32_t)TREE_MAX_BLOCKS) return;
    const uint64_t n_quads = (a.n_val + 3) / 4;
    uint64_t blocks = (n_quads + REMAP_WG - 1) / REMAP_WG;
    if (blocks > REMAP_MAX_WG) blocks = REMAP_MAX_WG;
    hipLaunchKernelGGL(k_votes_remap, dim3((unsigned)blocks), dim3(REMAP_WG), sizeof(uint32_t) * a.n_old, s, a);
}

// ------------------------------------------------------------------ tree
template <int TREE_WG, int TREE_PER_THREAD, bool LEAN = false>
__global__ void __launch_bounds__(TREE_WG)
k_tree(const TreeArgs a, const uint32_t lds_entries)
{
    POSEVO_FC_PRIO();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    tree_body<TREE_WG, TREE_PER_THREAD, LEAN>(a, lds_entries, smem);
}

template <int WG, int PER, bool LEAN = false>
static void launch_tree_shape(hipStream_t s, const TreeArgs& a)
{
    if (first_use_on_this_device<1000 + WG + PER + (LEAN ? 5000 : 0)>()) {  // > 64 KiB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_tree<WG, PER, LEAN>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)TREE_LDS_MAX);
    }
    const uint32_t entries = tree_lds_entries<PER>(a.tree.n);
    hipLaunchKernelGGL((k_tree<WG, PER, LEAN>), dim3(1), dim3(WG), tree_lds_bytes(entries), s, a, entries);
}

void launch_tree(hipStream_t s, const TreeArgs& a, int lean)
{
    const uint32_t n = a.tree.n;
    if (n <= 1024) launch_tree_shape<1024, 1>(s, a);  // 40 VGPRs x 4 waves per SIMD: lean as it is
    else if (lean && n <= 2048) launch_tree_shape<512, 4, true>(s, a);
    else if (lean && n <= 4096) launch_tree_shape<512, 8, true>(s, a);
    else if (n <= 2048) launch_tree_shape<1024, 2>(s, a);
    else if (n <= 4096) launch_tree_shape<1024, 4>(s, a);
    else launch_tree_shape<1024, 8>(s, a);
}

// ------------------------------------------------------------------ LMD update
// One wave per attestation; lane l walks bit words l, l+64, ...
__device__ __forceinline__ unsigned long long lmd_key(uint32_t epoch_p1, uint32_t order)
{
    return ((unsigned long long)epoch_p1 << 32) | (unsigned long long)(0xFFFFFFFEu - order);
}

template <int PHASE>
__global__ void __launch_bounds__(256)
k_lmd(const AttRow* __restrict__ rows, uint32_t n_rows, const uint32_t* __restrict__ members,
      const uint32_t* __restrict__ bit_arena, const uint8_t* __restrict__ flags,
      unsigned long long* __restrict__ vote_key, uint32_t* __restrict__ vote_block,
      uint32_t* __restrict__ vote_slot, const uint32_t* __restrict__ gates)
{
    const uint32_t a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const AttRow r = rows[a];
    if (gates && r.gate != NONE32 && gates[r.gate] != 0) return;  // voided on the device (overlapping members)
    const unsigned long long key = lmd_key(r.epoch_p1, r.order);
    // lane-parallel over bit positions: every lane tests its own bit (the 32 lanes sharing a word hit one line)
    for (uint32_t i = lane; i < r.n_bits; i += 64) {
        const uint32_t word = bit_arena[r.bits_word + (i >> 5)];
        if (!((word >> (i & 31)) & 1u)) continue;
        const uint32_t v = members[r.member_base + i];
        if (PHASE == 0) {
            if (flags[v] & VAL_EQUIVOCATING) continue;  // pe:1438
            atomicMax(&vote_key[v], key);                // strictly-later epoch wins; first in batch among equals
        } else {
            if (vote_key[v] == key) {                    // unique winner: (epoch, order) identifies one attestation
                vote_block[v] = r.block_idx;
                if (vote_slot) vote_slot[v] = r.slot;
                vote_key[v] = ((unsigned long long)r.epoch_p1 << 32) | 0xFFFFFFFFull;  // settled
            }
        }
    }
}

// Inverse of a committee table that partitions the validators: inv[v] = (committee id, index in committee).
__global__ void __launch_bounds__(256)
k_invert_committees(const uint32_t* __restrict__ members, const uint32_t* __restrict__ offsets, uint32_t n_committees,
                    uint32_t* __restrict__ inv_comm, uint32_t* __restrict__ inv_pos)
{
    const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_committees) return;
    const uint32_t b = offsets[c], e = offsets[c + 1];
    for (uint32_t i = b + (threadIdx.x & 63); i < e; i += 64) {
        const uint32_t v = members[i];
        inv_comm[v] = c;
        inv_pos[v] = i - b;
    }
}

void launch_invert_committees(hipStream_t s, const uint32_t* members, const uint32_t* offsets, uint32_t n_committees,
                              uint32_t* inv_comm, uint32_t* inv_pos, uint64_t n_val)
{
    (void)hipMemsetAsync(inv_comm, 0xFF, 4ull * n_val, s);
    if (n_committees == 0) return;
    hipLaunchKernelGGL(k_invert_committees, dim3((n_committees + 3) / 4), dim3(256), 0, s, members, offsets,
                       n_committees, inv_comm, inv_pos);
}

// update_latest_messages (pe:1435-1441), validator-major: one lane per validator walks the batch rows of ITS
// committee in batch order -- literally the spec's sequential loop, so no atomics and no tie-break tag are needed;
// vote/flag/key tables are streamed (coalesced) instead of hit by a million random 8-byte atomics.
// crow_start/crow_list: CSR of batch rows per committee id (rows in batch order).
__global__ void __launch_bounds__(256)
k_lmd_validator_major(const AttRow* __restrict__ rows, const uint32_t* __restrict__ crow_start,
                      const uint32_t* __restrict__ crow_list, const uint32_t* __restrict__ inv_comm,
                      const uint32_t* __restrict__ inv_pos, const uint32_t* __restrict__ bit_arena,
                      const uint8_t* __restrict__ flags, uint64_t n_val, unsigned long long* __restrict__ vote_key,
                      uint32_t* __restrict__ vote_block, uint32_t* __restrict__ vote_slot,
                      const uint32_t* __restrict__ gates)
{
    POSEVO_FC_PRIO();
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_val) return;
    const uint32_t c = inv_comm[v];
    if (c == NONE32) return;
    const uint32_t kb = crow_start[c], ke = crow_start[c + 1];
    if (kb == ke) return;
    if (flags[v] & VAL_EQUIVOCATING) return;  // pe:1438
    const uint32_t i = inv_pos[v];
    uint32_t epoch_p1 = (uint32_t)(vote_key[v] >> 32);  // 0 = no latest message
    uint32_t new_block = NONE32, new_slot = 0;
    for (uint32_t k = kb; k < ke; ++k) {
        const AttRow r = rows[crow_list[k]];
        if (i >= r.n_bits) continue;
        if (gates && r.gate != NONE32 && gates[r.gate] != 0) continue;  // voided on the device
        if (!((bit_arena[r.bits_word + (i >> 5)] >> (i & 31)) & 1u)) continue;
        if (r.epoch_p1 > epoch_p1) {  // "i not in latest_messages or target.epoch > latest_messages[i].epoch"
            epoch_p1 = r.epoch_p1;
            new_block = r.block_idx;
            new_slot = r.slot;
        }
    }
    if (new_block != NONE32) {
        vote_key[v] = ((unsigned long long)epoch_p1 << 32) | 0xFFFFFFFFull;
        vote_block[v] = new_block;
        if (vote_slot) vote_slot[v] = new_slot;
    }
}

void launch_lmd_validator_major(hipStream_t s, const AttRow* rows, const uint32_t* crow_start,
                                const uint32_t* crow_list, const uint32_t* inv_comm, const uint32_t* inv_pos,
                                const uint32_t* bit_arena, const uint8_t* flags, uint64_t n_val, uint64_t* vote_key,
                                uint32_t* vote_block, uint32_t* vote_slot, const uint32_t* gates)
{
    if (n_val == 0) return;
    hipLaunchKernelGGL(k_lmd_validator_major, dim3((unsigned)((n_val + 255) / 256)), dim3(256), 0, s, rows, crow_start,
                       crow_list, inv_comm, inv_pos, bit_arena, flags, n_val,
                       reinterpret_cast<unsigned long long*>(vote_key), vote_block, vote_slot, gates);
}

void launch_lmd_update(hipStream_t s, const AttRow* rows, uint32_t n_rows, const uint32_t* members,
                       const uint32_t* bit_arena, const uint8_t* flags, uint64_t* vote_key, uint32_t* vote_block,
                       uint32_t* vote_slot, const uint32_t* gates)
{
    if (n_rows == 0) return;
    const unsigned blocks = (n_rows + 3) / 4;
    hipLaunchKernelGGL(k_lmd<0>, dim3(blocks), dim3(256), 0, s, rows, n_rows, members, bit_arena, flags,
                       reinterpret_cast<unsigned long long*>(vote_key), vote_block, vote_slot, gates);
    hipLaunchKernelGGL(k_lmd<1>, dim3(blocks), dim3(256), 0, s, rows, n_rows, members, bit_arena, flags,
                       reinterpret_cast<unsigned long long*>(vote_key), vote_block, vote_slot, gates);
}

// ------------------------------------------------------------------ participation
__global__ void __launch_bounds__(256)
k_participation(const AttRow* __restrict__ rows, uint32_t n_rows, const uint32_t* __restrict__ members,
                const uint32_t* __restrict__ bit_arena, const uint16_t* __restrict__ eff_increments,
                unsigned long long base_reward_per_increment, uint32_t* __restrict__ part_cur,
                uint32_t* __restrict__ part_prev, unsigned long long* __restrict__ numerators,
                const uint32_t* __restrict__ numerator_slot, const uint32_t* __restrict__ gates)
{
    const uint32_t a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= n_rows) return;
    const int lane = threadIdx.x & 63;
    const AttRow r = rows[a];
    uint32_t* part = r.which ? part_prev : part_cur;
    unsigned long long num = 0;
    const uint32_t n_use = (gates && r.gate != NONE32 && gates[r.gate] != 0) ? 0u : r.n_bits;  // voided on the device
    for (uint32_t i = lane; i < n_use; i += 64) {
        const uint32_t word = bit_arena[r.bits_word + (i >> 5)];
        if (!((word >> (i & 31)) & 1u)) continue;
        const uint32_t v = members[r.member_base + i];
        // attestations of one round touch pairwise disjoint validators, and byte stores do not disturb the
        // neighbouring bytes: a plain byte read-modify-write is exact here (no atomics on the hot path)
        uint8_t* pb = reinterpret_cast<uint8_t*>(part) + v;
        const uint32_t old = *pb;
        const uint32_t fresh = r.flag_mask & ~old & 0x7u;
        if (fresh) {
            *pb = (uint8_t)(old | r.flag_mask);
            // PARTICIPATION_FLAG_WEIGHTS = [14, 26, 14] (Appendix A.9)
            const uint32_t wsum = ((fresh & 1u) ? 14u : 0u) + ((fresh & 2u) ? 26u : 0u) + ((fresh & 4u) ? 14u : 0u);
            num += (unsigned long long)eff_increments[v] * base_reward_per_increment * wsum;
        }
    }
    num = wave_sum(num);
    if (lane == 0) numerators[numerator_slot[a]] = num;
}

void launch_participation(hipStream_t s, const AttRow* rows, uint32_t n_rows, const uint32_t* members,
                          const uint32_t* bit_arena, const uint16_t* eff_increments,
                          uint64_t base_reward_per_increment, uint32_t* part_cur_words, uint32_t* part_prev_words,
                          uint64_t* numerators, const uint32_t* numerator_slot, const uint32_t* gates)
{
    if (n_rows == 0) return;
    hipLaunchKernelGGL(k_participation, dim3((n_rows + 3) / 4), dim3(256), 0, s, rows, n_rows, members, bit_arena,
                       eff_increments, (unsigned long long)base_reward_per_increment, part_cur_words,
                       part_prev_words, reinterpret_cast<unsigned long long*>(numerators), numerator_slot, gates);
}

// ------------------------------------------------------------------ indexed attestations
// get_indexed_attestation (call sites pe:736, pe:975): attesting_indices =
// sorted(committee[i] for i with bits[i]).  One workgroup per attestation: compaction by a block prefix sum over the
// set bits (wave ballot + popcount), then a bitonic sort in LDS (committees hold <= 8192 members).
constexpr int IDX_WG = 256;
constexpr int IDX_MAX = 8192;

__global__ void __launch_bounds__(IDX_WG)
k_indexed_attestations(const AttRow* __restrict__ rows, uint32_t n_rows, const uint32_t* __restrict__ members,
                       const uint32_t* __restrict__ bit_arena, const uint32_t* __restrict__ out_offsets,
                       uint32_t* __restrict__ out_indices)
{
    __shared__ uint32_t keys[IDX_MAX];
    __shared__ uint32_t wave_cnt[IDX_WG / 64];
    __shared__ uint32_t base_s;
    const uint32_t a = blockIdx.x;
    if (a >= n_rows) return;
    const AttRow r = rows[a];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base_s = 0;
    __syncthreads();
    // compaction, 256 bit positions per pass: ballot the set bits, rank = popcount of lower lanes + wave offsets
    for (uint32_t i0 = 0; i0 < r.n_bits; i0 += IDX_WG) {
        const uint32_t i = i0 + tid;
        bool set = false;
        if (i < r.n_bits) set = (bit_arena[r.bits_word + (i >> 5)] >> (i & 31)) & 1u;
        const unsigned long long ballot = __ballot(set);
        const uint32_t below = __builtin_popcountll(ballot & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wave] = __builtin_popcountll(ballot);
        __syncthreads();
        uint32_t off = base_s;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        if (set) keys[off + below] = members[r.member_base + i];
        __syncthreads();
        if (tid == 0) base_s += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    const uint32_t count = base_s;
    uint32_t n2 = 1;
    while (n2 < count) n2 <<= 1;
    for (uint32_t i = count + tid; i < n2; i += IDX_WG) keys[i] = NONE32;  // pad: sorts to the end
    __syncthreads();
    for (uint32_t k = 2; k <= n2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < n2; i += IDX_WG) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const uint32_t x = keys[i], y = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) { keys[i] = y; keys[ixj] = x; }
                }
            }
            __syncthreads();
        }
    }
    const uint32_t o = out_offsets[a];
    for (uint32_t i = tid; i < count; i += IDX_WG) out_indices[o + i] = keys[i];
}

void launch_indexed_attestations(hipStream_t s, const AttRow* rows, uint32_t n_rows, const uint32_t* members,
                                 const uint32_t* bit_arena, const uint32_t* out_offsets, uint32_t* out_indices)
{
    if (n_rows == 0) return;
    hipLaunchKernelGGL(k_indexed_attestations, dim3(n_rows), dim3(IDX_WG), 0, s, rows, n_rows, members, bit_arena,
                       out_offsets, out_indices);
}

// ------------------------------------------------------------------ FFG balance sums
// The three Gwei sums process_justification_and_finalization (pe:791-802) feeds to
// weigh_justification_and_finalization (pe:815-853):
//   total_active_balance     sum over validators active in the current epoch
//   previous_target_balance  sum over unslashed validators active in the previous epoch whose
//                            previous_epoch_participation has TIMELY_TARGET (get_unslashed_participating_indices)
//   current_target_balance   same for the current epoch
// One streaming pass (balance u64 + state flags u8 + two participation bytes), per-workgroup partials.
constexpr uint32_t SVAL_ACTIVE_CUR = 0x01u, SVAL_SLASHED = 0x02u, SVAL_ACTIVE_PREV = 0x08u, TIMELY_TARGET_BIT = 0x02u;

__global__ void __launch_bounds__(256)
k_ffg_balances(const uint64_t* __restrict__ balance, const uint8_t* __restrict__ sflags,
               const uint8_t* __restrict__ part_cur, const uint8_t* __restrict__ part_prev, uint64_t n_val,
               unsigned long long* __restrict__ partials /* [gridDim.x][3] */)
{
    unsigned long long tot = 0, prev = 0, cur = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_val; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t f = sflags[v];
        const unsigned long long b = balance[v];
        if (f & SVAL_ACTIVE_CUR) tot += b;
        if (!(f & SVAL_SLASHED)) {
            if ((f & SVAL_ACTIVE_PREV) && (part_prev[v] & TIMELY_TARGET_BIT)) prev += b;
            if ((f & SVAL_ACTIVE_CUR) && (part_cur[v] & TIMELY_TARGET_BIT)) cur += b;
        }
    }
    __shared__ unsigned long long acc[3];
    if (threadIdx.x == 0) { acc[0] = 0; acc[1] = 0; acc[2] = 0; }
    tot = wave_sum(tot);
    prev = wave_sum(prev);
    cur = wave_sum(cur);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { atomicAdd(&acc[0], tot); atomicAdd(&acc[1], prev); atomicAdd(&acc[2], cur); }
    __syncthreads();
    if (threadIdx.x < 3) partials[blockIdx.x * 3 + threadIdx.x] = acc[threadIdx.x];
}

uint32_t launch_ffg_balances(hipStream_t s, const uint64_t* balance, const uint8_t* sflags, const uint8_t* part_cur,
                             const uint8_t* part_prev, uint64_t n_val, uint64_t* partials)
{
    uint64_t blocks = (n_val + 256 * 16 - 1) / (256 * 16);
    if (blocks > 256) blocks = 256;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_ffg_balances, dim3((unsigned)blocks), dim3(256), 0, s, balance, sflags, part_cur, part_prev,
                       n_val, reinterpret_cast<unsigned long long*>(partials));
    return (uint32_t)blocks;
}

// ------------------------------------------------------------------ effective-balance hysteresis
// process_effective_balance_updates (pe:122-133), one lane per validator over the working-state view:
//   if balance + DOWNWARD_THRESHOLD < effective_balance or effective_balance + UPWARD_THRESHOLD < balance:
//       effective_balance = min(balance - balance % EFFECTIVE_BALANCE_INCREMENT, MAX_EFFECTIVE_BALANCE)
// The two comparisons are written as differences, which say the same over the reference's unbounded integers and cannot
// wrap in 64 bits.  Writes the balance and its u16 increment count where the value changed; *n_changed counts those
// (a ballot per wave, one atomic per wave).
__global__ void __launch_bounds__(256)
k_effective_balance_update(const unsigned long long* __restrict__ balances, unsigned long long* __restrict__ eff_balance,
                           uint16_t* __restrict__ increments, uint64_t n_val, unsigned long long increment,
                           unsigned long long downward_threshold, unsigned long long upward_threshold,
                           unsigned long long max_eff, unsigned long long* __restrict__ n_changed)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool changed = false;
    if (i < n_val) {
        const unsigned long long balance = balances[i], eff = eff_balance[i];
        if ((eff > balance && eff - balance > downward_threshold) || (balance > eff && balance - eff > upward_threshold)) {
            const unsigned long long next = min(balance - balance % increment, max_eff);
            if (next != eff) {
                eff_balance[i] = next;
                increments[i] = (uint16_t)(next / increment);  // <= max_eff / increment <= 65535 (checked by the host)
                changed = true;
            }
        }
    }
    const unsigned long long ballot = __ballot(changed);
    if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(n_changed, (unsigned long long)__builtin_popcountll(ballot));
}

void launch_effective_balance_update(hipStream_t s, const uint64_t* balances, uint64_t* eff_balance, uint16_t* increments,
                                     uint64_t n_val, uint64_t increment, uint64_t downward_threshold,
                                     uint64_t upward_threshold, uint64_t max_eff, uint64_t* n_changed)
{
    if (n_val == 0) return;
    hipLaunchKernelGGL(k_effective_balance_update, dim3((unsigned)((n_val + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(balances),
                       reinterpret_cast<unsigned long long*>(eff_balance), increments, n_val,
                       (unsigned long long)increment, (unsigned long long)downward_threshold,
                       (unsigned long long)upward_threshold, (unsigned long long)max_eff,
                       reinterpret_cast<unsigned long long*>(n_changed));
}

// ------------------------------------------------------------------ working-state view = registry
__global__ void __launch_bounds__(256)
k_state_view_from_registry(const uint8_t* __restrict__ flags, const unsigned long long* __restrict__ balance,
                           unsigned long long increment, uint64_t n_val, uint8_t* __restrict__ sflags,
                           uint16_t* __restrict__ increments)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_val) return;
    const uint32_t f = flags[i];
    sflags[i] = (uint8_t)((f & (VAL_ACTIVE | VAL_SLASHED)) | ((f & VAL_ACTIVE) ? 0x08u : 0u));  // PE_VAL_ACTIVE_PREV
    increments[i] = (uint16_t)(balance[i] / increment);
}
void launch_state_view_from_registry(hipStream_t s, const uint8_t* flags, const uint64_t* balance, uint64_t increment,
                                     uint64_t n_val, uint8_t* sflags, uint16_t* increments)
{
    if (n_val == 0) return;
    hipLaunchKernelGGL(k_state_view_from_registry, dim3((unsigned)((n_val + 255) / 256)), dim3(256), 0, s, flags,
                       reinterpret_cast<const unsigned long long*>(balance), (unsigned long long)increment, n_val,
                       sflags, increments);
}

// ------------------------------------------------------------------ bitfield union
__global__ void __launch_bounds__(256)
k_bits_union(const UnionArgs a)
{
    POSEVO_FC_PRIO();
    bits_union_body(blockIdx.x * 4 + (threadIdx.x >> 6), a);
}

void launch_bits_union(hipStream_t s, const UnionArgs& a)
{
    if (a.n_groups == 0) return;
    hipLaunchKernelGGL(k_bits_union, dim3((a.n_groups + 3) / 4), dim3(256), 0, s, a);
}

}  // namespace posevo
