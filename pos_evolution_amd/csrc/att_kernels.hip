// att_kernels.hip -- attestation rows resident in device memory: what the host does per row in engine_attest.cpp,
// done on the device so that the host only enqueues launches (the host paced the step).
//
//   k_att_ingest          one lane per input row: hash the 128-byte AttestationData (pe:689-697) + len(aggregation_bits),
//                         insert into an open-addressing table in HBM; a slot's value is the SMALLEST row index of its
//                         class (atomicMin), i.e. the row of first appearance -- the grouping rule of pe_aggregate
//                         ("attestations with identical AttestationData and n_bits form one group, groups ordered by
//                         first appearance").
//   k_att_plan            one workgroup: group ids by a prefix count over the representatives, committee resolution
//                         (get_beacon_committee's index arithmetic, A.6) against the store's current / previous
//                         epoch tables, offsets of the unions (prefix sums), member counts, the G1 plan, the
//                         rows-per-committee lists the handlers walk.  Writes the very descriptor arrays the host
//                         path uploads (UnionGroup, G1Group), so k_bits_union / k_g1_* run unchanged.
//   k_att_members         one lane per input row: group_of[], the group's member list, AND of the signature verdicts,
//                         the output rows; clears the hash table for the next call.
//   k_att_validate_fc     validate_on_attestation (A.4, called at pe:970) + is_valid_indexed_attestation's structural
//                         part per group: root -> block lookups in a device hash table, the LMD/FFG consistency walk
//                         (at most SLOTS_PER_EPOCH parent steps once the two slot checks passed), one AttRow + one
//                         pe_att_status per group.
//   k_att_validate_state  the asserts of process_attestation (pe:724-730) and
//                         get_attestation_participation_flag_indices (A.9) per group.
//                         (Both validators ask att_rules.h for the status: one text with the host routes.)
//   k_lmd_vm_tables       update_latest_messages (pe:1435-1441), validator-major, both candidate tables in one launch.
//   k_participation_tables the flag loop of pe:745-749, one wave per committee, rows of a committee in batch order.
//
// The kernels here and their launchers; the bodies of ingest, plan, members, validate_fc and lmd_vm_tables are device
// functions in att_bodies.inc, which pair_kernels.hip runs as block ranges of its paired launches as well.
//
// Integer / byte work, latency- and HBM-bound: no MFMA.
#include <cstdlib>
#include "att_bodies.inc"

namespace posevo {

// ------------------------------------------------------------------ ingest: hash + insert
__global__ void __launch_bounds__(256)
k_att_ingest(const IngestArgs a)
{
    __builtin_amdgcn_s_setprio(3);  // in front of a head, beside the previous step's G1 kernels (see fc_kernels.hip)
    att_ingest_body(blockIdx.x, gridDim.x, a);
}

void launch_att_ingest(hipStream_t s, const IngestArgs& a)
{
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_att_ingest, dim3(att_ingest_blocks(a)), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------ plan: one lane per input row, many workgroups
__global__ void __launch_bounds__(PLAN_WG) __attribute__((amdgpu_waves_per_eu(6, 8)))
k_att_plan(const AttPlanArgs a)
{
    __builtin_amdgcn_s_setprio(3);
    att_plan_body(blockIdx.x, gridDim.x, a);
}

void launch_att_plan(hipStream_t s, const AttPlanArgs& a)
{
    hipLaunchKernelGGL(k_att_plan, dim3(att_plan_blocks(a)), dim3(PLAN_WG), 0, s, a);
}

// ------------------------------------------------------------------ members
__global__ void __launch_bounds__(256)
k_att_members(const MembersArgs a)
{
    __builtin_amdgcn_s_setprio(3);
    att_members_body(blockIdx.x * 256 + threadIdx.x, a);
}

void launch_att_members(hipStream_t s, const MembersArgs& a)
{
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_att_members, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------ committee-sharded exchange (pe_aggregate_exchange)
// Every rank aggregates the rows of ITS committees; what the other ranks need of the result -- the aggregate attestation
// itself: AttestationData + OR-ed bits (pe:714-717), its attester count and its verdict flags -- is packed into fixed
// slots, all-gathered, and unpacked into one dense batch that the receiving rank ingests like any batch of rows.
//   send buffer: [0] groups packed, [1] error, [2..3] reserved | slot g: 36 words row, count, reserved, `wps` words of bits
__global__ void __launch_bounds__(256)
k_att_pack(const uint4* __restrict__ rows, const AttGroup* __restrict__ grp, const AttPlan* __restrict__ plan,
           const uint32_t* __restrict__ res_bits, const uint32_t* __restrict__ res_info, uint32_t slots, uint32_t wps,
           uint32_t* __restrict__ send)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ng_all = plan->n_groups;
    const uint32_t ng = min(ng_all, slots);
    if (g == 0) {
        send[0] = ng;
        send[1] = ng_all > slots ? ERR_CAPACITY : plan->last_error;  // not plan->error: k_att_members has cleared it
        send[2] = send[3] = 0;
    }
    if (g >= ng) return;
    const AttGroup G = grp[g];
    const uint32_t slot_words = 38 + wps;
    uint32_t* o = send + 4 + (size_t)g * slot_words;
    const uint4* r = rows + (size_t)9 * G.rep;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint4 q = r[k];
        o[4 * k] = q.x; o[4 * k + 1] = q.y; o[4 * k + 2] = q.z; o[4 * k + 3] = q.w;
    }
    const uint32_t count = res_info[2 * g], overlap = res_info[2 * g + 1];
    uint32_t flags = r[8].z & ~FLAG_SIG_VALID;
    if (G.sig_valid && !overlap) flags |= FLAG_SIG_VALID;   // the AND of the members' verdicts; overlapping members never verify (A.8)
    if (overlap) flags |= FLAG_OVERLAPPING;
    o[32] = 0;          // bits_offset: set by the receiver
    o[33] = G.n_bits;
    o[34] = flags;
    o[35] = 0;
    o[36] = count;
    o[37] = 0;
    const uint32_t nw = (G.n_bits + 31) >> 5;
    if (nw > wps) { atomicMax(&send[1], ERR_CAPACITY); return; }
    for (uint32_t j = 0; j < wps; ++j) o[38 + j] = j < nw ? res_bits[G.out_word + j] : 0u;
}

void launch_att_pack(hipStream_t s, const void* rows, const AttGroup* grp, const AttPlan* plan, const uint32_t* res_bits,
                     const uint32_t* res_info, uint32_t slots, uint32_t wps, uint32_t* send)
{
    hipLaunchKernelGGL(k_att_pack, dim3((std::max(slots, 1u) + 255) / 256), dim3(256), 0, s, static_cast<const uint4*>(rows), grp,
                       plan, res_bits, res_info, slots, wps, send);
}

// recv: `world` send buffers back to back.  Rank r's groups land behind those of ranks < r: out_rows[base_r + j] with
// bits_offset = (base_r + j) * 4 * wps into out_bits; *n_dev = the total; *err = the first non-zero error word.
__global__ void __launch_bounds__(256)
k_att_unpack(const uint32_t* __restrict__ recv, uint32_t world, uint32_t slots, uint32_t wps, uint32_t* __restrict__ out_rows,
             uint32_t* __restrict__ out_bits, uint32_t* __restrict__ n_dev, uint32_t* __restrict__ err_host)
{
    const uint32_t slot_words = 38 + wps;
    const size_t rank_words = 4 + (size_t)slots * slot_words;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t r = t / slots, j = t % slots;
    if (t == 0) {
        uint32_t total = 0, err = 0;
        for (uint32_t q = 0; q < world; ++q) {
            total += recv[q * rank_words];
            if (!err) err = recv[q * rank_words + 1];
        }
        *n_dev = err ? 0u : total;   // a rank whose aggregate failed: nothing is applied anywhere
        if (err_host) *err_host = err;
    }
    if (r >= world) return;
    uint32_t base = 0;
    for (uint32_t q = 0; q < r; ++q) base += recv[q * rank_words];
    if (j >= recv[r * rank_words]) return;
    const uint32_t* in = recv + r * rank_words + 4 + (size_t)j * slot_words;
    const uint32_t dst = base + j;
    uint32_t* o = out_rows + (size_t)36 * dst;
#pragma unroll
    for (int k = 0; k < 36; ++k) o[k] = in[k];
    o[32] = dst * 4 * wps;
    uint32_t* b = out_bits + (size_t)dst * wps;
    for (uint32_t k = 0; k < wps; ++k) b[k] = in[38 + k];
}

void launch_att_unpack(hipStream_t s, const uint32_t* recv, uint32_t world, uint32_t slots, uint32_t wps, void* out_rows,
                       uint32_t* out_bits, uint32_t* n_dev, uint32_t* err_host)
{
    const uint32_t n = std::max(world * slots, 1u);
    hipLaunchKernelGGL(k_att_unpack, dim3((n + 255) / 256), dim3(256), 0, s, recv, world, slots, wps,
                       static_cast<uint32_t*>(out_rows), out_bits, n_dev, err_host);
}

// ------------------------------------------------------------------ validate_on_attestation (A.4) per group
__global__ void __launch_bounds__(256)
k_att_validate_fc(const ValidateFcArgs a)
{
    __builtin_amdgcn_s_setprio(3);
    att_validate_fc_body(blockIdx.x * 256 + threadIdx.x, a);
}

void launch_att_validate_fc(hipStream_t s, const ValidateFcArgs& a)
{
    if (a.n_bound == 0) return;
    hipLaunchKernelGGL(k_att_validate_fc, dim3((a.n_bound + 255) / 256), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------ process_attestation's asserts + flag indices per group
namespace {
__device__ __forceinline__ bool root_equals(const uint8_t* root32, const uint4& r0, const uint4& r1)
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(root32);
    return w[0] == r0.x && w[1] == r0.y && w[2] == r0.z && w[3] == r0.w && w[4] == r1.x && w[5] == r1.y && w[6] == r1.z &&
           w[7] == r1.w;
}
// the row adapter of att_state_status (att_rules.h): the committee as k_att_plan resolved it, the source against the
// justified checkpoint of the row's epoch, and the block roots of the state's chain the host resolved (StateCtxDev)
struct StateRowDev {
    const Row9& r;
    const AttGroup& G;
    const BlockTableDev& bt;
    const StateCtxDev& S;
    const bool is_cur;
    const unsigned long long slot;
    __device__ __forceinline__ int32_t committee_status() const { return (int32_t)G.status_agg; }
    __device__ __forceinline__ bool index_over() const { return G.index_over != 0; }
    __device__ __forceinline__ bool source_matches() const
    {
        const uint4 s0 = make_uint4(r.q[3].z, r.q[3].w, r.q[4].x, r.q[4].y), s1 = make_uint4(r.q[4].z, r.q[4].w, r.q[5].x, r.q[5].y);
        return row_source_epoch(r) == (is_cur ? S.cj_epoch : S.pj_epoch) && root_equals(is_cur ? S.cj_root : S.pj_root, s0, s1);
    }
    __device__ __forceinline__ bool matching_target() const
    {
        const uint32_t tgt_blk = S.tgt_blk[is_cur ? 0 : 1];
        return tgt_blk != NONE32 && root_equals(bt.roots + 32ull * tgt_blk, r.q[6], r.q[7]);
    }
    __device__ __forceinline__ bool matching_head() const
    {
        const unsigned long long j = slot + S.slots_per_epoch - S.slot;  // pe:726 puts data.slot into [state.slot - spe, state.slot)
        const uint32_t head_blk = j < 64 ? S.head_blk[j] : NONE32;
        return head_blk != NONE32 && root_equals(bt.roots + 32ull * head_blk, r.q[1], r.q[2]);
    }
};
}  // namespace
__global__ void __launch_bounds__(256)
k_att_validate_state(const uint4* __restrict__ rows, const AttGroup* __restrict__ grp, const AttPlan* __restrict__ plan,
                     uint32_t cap, BlockTableDev bt, const StateCtxDev S,
                     const uint32_t* __restrict__ union_info, AttRow* __restrict__ out_rows,
                     int32_t* __restrict__ status_dev, int32_t* __restrict__ status_host, uint32_t* __restrict__ err_host)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ng = plan->n_groups;
    if (ng > cap) {
        if (g < ng) status_dev[g] = -1;
        if (g == 0) *err_host = ERR_CAPACITY;
        return;
    }
    if (g >= ng) return;
    const AttGroup G = grp[g];
    Row9 r;
    load_row(r, rows, G.rep);
    const unsigned long long slot = row_slot(r), tep = row_target_epoch(r);
    const uint32_t which = att_which(tep, S.cur_epoch);
    const StateClock sc{S.slot, S.cur_epoch, S.prev_epoch, S.slots_per_epoch, S.min_inclusion_delay, S.sqrt_spe};
    const StateVerdict v = att_state_status(StateRowDev{r, G, bt, S, which == 0, slot}, slot, tep, sc);
    int32_t st = v.status;
    const uint32_t cnt = union_info[2 * g], overlap = union_info[2 * g + 1];
    if (st == ST_OK) st = att_indexed_status(G.sig_valid != 0, overlap != 0, cnt);  // pe:736
    out_rows[g] = att_row_flags(G.member_base, G.size, G.out_word, v.flag_mask, which, g, g);
    status_dev[g] = st;
    status_host[g] = st;
}

void launch_att_validate_state(hipStream_t s, const void* rows, const AttGroup* grp, const AttPlan* plan, uint32_t n_bound,
                               uint32_t cap, BlockTableDev bt, const StateCtxDev& st, const uint32_t* union_info,
                               AttRow* out_rows, int32_t* status_dev, int32_t* status_host, uint32_t* err_host)
{
    if (n_bound == 0) return;
    hipLaunchKernelGGL(k_att_validate_state, dim3((n_bound + 255) / 256), dim3(256), 0, s, static_cast<const uint4*>(rows),
                       grp, plan, cap, bt, st, union_info, out_rows, status_dev, status_host, err_host);
}

// ------------------------------------------------------------------ LMD update, validator-major, both tables
__global__ void __launch_bounds__(256)
k_lmd_vm_tables(const LmdVmArgs a)
{
    __builtin_amdgcn_s_setprio(3);  // in front of a head, beside the previous step's G1 kernels (see fc_kernels.hip)
    lmd_vm_tables_body((unsigned long long)blockIdx.x * 256 + threadIdx.x, a);
}

void launch_lmd_vm_tables(hipStream_t s, const LmdVmArgs& a)
{
    if (a.n_val == 0) return;
    hipLaunchKernelGGL(k_lmd_vm_tables, dim3((unsigned)((a.n_val + 255) / 256)), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------ participation flags, one wave per committee
__global__ void __launch_bounds__(256)
k_participation_tables(const AttRow* __restrict__ rows, TablesDev tables, const uint32_t* __restrict__ cs0,
                       const uint32_t* __restrict__ cs1, const uint32_t* __restrict__ cl0,
                       const uint32_t* __restrict__ cl1, const AttPlan* __restrict__ plan,
                       const uint32_t* __restrict__ bit_arena, const uint16_t* __restrict__ eff_increments,
                       unsigned long long base_reward_per_increment, uint32_t* __restrict__ part_cur,
                       uint32_t* __restrict__ part_prev, unsigned long long* __restrict__ numerators,
                       const uint32_t* __restrict__ gates, uint32_t cap)
{
    const int t = blockIdx.y;
    // more groups than the caller's arrays hold: k_att_validate_state reported ERR_CAPACITY, nothing is applied and
    // numerators[] (sized by cap) is not written
    if (plan->n_groups > cap) return;
    if (!tables.t[t].valid || plan->n_rows_table[t] == 0) return;
    const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= tables.t[t].n_committees) return;
    const uint32_t* crow_start = t ? cs1 : cs0;
    const uint32_t* crow_list = t ? cl1 : cl0;
    const uint32_t kb = crow_start[c], ke = crow_start[c + 1];
    if (kb == ke) return;
    const int lane = threadIdx.x & 63;
    const uint32_t* members = tables.t[t].members;
    // the committee's rows in batch order (ascending group id): a selection loop, the lists hold one or a few rows
    uint32_t last = NONE32;  // NONE32 + 1 == 0
    for (uint32_t done = kb; done < ke; ++done) {
        uint32_t g = NONE32;
        for (uint32_t k = kb; k < ke; ++k) {
            const uint32_t x = crow_list[k];
            if ((last == NONE32 || x > last) && x < g) g = x;
        }
        last = g;
        const AttRow r = rows[g];
        unsigned long long num = 0;
        if (gates[r.gate] == 0) {
            uint32_t* part = r.which ? part_prev : part_cur;
            for (uint32_t i = lane; i < r.n_bits; i += 64) {
                const uint32_t word = bit_arena[r.bits_word + (i >> 5)];
                if (!((word >> (i & 31)) & 1u)) continue;
                const uint32_t v = members[r.member_base + i];
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
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) num += __shfl_xor(num, off, 64);  // (not wave_sum: the kernel's code differs)
        if (lane == 0) numerators[g] = num;
        // the next row of this committee may touch the same validators: this wave's byte stores must be visible to its
        // own later loads (same wave, program order: they are)
    }
}

void launch_participation_tables(hipStream_t s, const AttRow* rows, TablesDev tables, uint32_t* const crow_start[2],
                                 uint32_t* const crow_list[2], const AttPlan* plan, const uint32_t* bit_arena,
                                 const uint16_t* eff_increments, uint64_t base_reward_per_increment,
                                 uint32_t* part_cur_words, uint32_t* part_prev_words, uint64_t* numerators,
                                 const uint32_t* gates, uint32_t cap)
{
    uint32_t nc = tables.t[0].valid ? tables.t[0].n_committees : 0u;
    if (tables.t[1].valid) nc = nc > tables.t[1].n_committees ? nc : tables.t[1].n_committees;
    if (nc == 0) return;
    const unsigned ny = tables.t[1].valid ? 2u : 1u;
    hipLaunchKernelGGL(k_participation_tables, dim3((nc + 3) / 4, ny), dim3(256), 0, s, rows, tables, crow_start[0],
                       crow_start[1], crow_list[0], crow_list[1], plan, bit_arena, eff_increments,
                       (unsigned long long)base_reward_per_increment, part_cur_words, part_prev_words,
                       reinterpret_cast<unsigned long long*>(numerators), gates, cap);
}

}  // namespace posevo
