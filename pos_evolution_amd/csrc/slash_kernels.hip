// slash_kernels.hip -- slashing detection on the device: the two Casper conditions (pe:1128) as the reference's
// is_slashable_attestation_data (pe:1134-1143) states them, over every new vote of a validator and its history.
//
// One lane per validator, as k_lmd_validator_major: the lane finds its committee through the inverse map, walks the
// batch rows of that committee in batch order and keeps the rows that carry its bit -- the sequential semantics of
// pe_slasher_ingest need no atomics.  The history is a streaming read: 8 bytes per target epoch of the window and per
// attesting validator, coalesced because it is epoch-major (kernels.h).  Up to SLASH_NV new votes are held in registers
// and compared in ONE pass over the H slots; a validator with more new votes in one call (rare: that many different
// votes in one batch) takes further passes, each behind the records the previous one wrote.
// The kernel is a guest beside the G1 accumulation like the flag passes: it does not raise its wave priority.
//
// The k_slash_rows_* kernels behind it feed that scan from the groups of a resident aggregate (PE_ROWS_RESIDENT): statuses,
// AttestationData ids out of the per-slot tables in device memory, one SlashRow per group and the committees' group lists
// in ascending order (kernels.h, SlashRowsArgs / SlashListsArgs).  What one phase hands to the next crosses a kernel boundary; inside a
// launch lanes meet only in atomics on table entries (a compare-and-swap claims an entry, atomicMin keeps the lowest
// group), and no id comes out of an atomic: ids are the slot's count plus an ordered scan over the groups.
#include <algorithm>
#include "kernels.h"
#include "wave64.h"

namespace posevo {

namespace {

constexpr uint32_t SLASH_DOUBLE = 1u, SLASH_SURROUND = 2u;  // PE_SLASH_DOUBLE / PE_SLASH_SURROUND (include/posevo.h)
constexpr uint8_t SLASH_VAL_EQUIVOCATING = 0x04u;           // PE_VAL_EQUIVOCATING

__device__ __forceinline__ void slash_emit(const SlashArgs& a, uint32_t v, uint32_t kind, uint32_t t1, uint32_t id1,
                                           uint32_t t2, uint32_t id2)
{
    const uint32_t at = atomicAdd(a.counter, 1u);  // device scope; evidence is rare
    if (at >= a.cap) return;                       // dropped: the count stays exact
    uint32_t* e = a.evidence + 6ull * at;
    e[0] = v; e[1] = kind; e[2] = t1; e[3] = id1; e[4] = t2; e[5] = id2;
}

// new vote (s, t, id) against a record (sb, tb, idb) the validator holds: every slashable pair is one piece of evidence.
// Same target epoch: the caller has ruled out equal data, so it is a double vote, d1 = the recorded one.  Otherwise the
// two orders of the surround clause; d1 = the surrounding vote.
__device__ __forceinline__ bool slash_compare(const SlashArgs& a, uint32_t v, uint32_t s, uint32_t t, uint32_t id,
                                              uint32_t sb, uint32_t tb, uint32_t idb)
{
    if (tb == t) { slash_emit(a, v, SLASH_DOUBLE, tb, idb, t, id); return true; }
    if (s < sb && tb < t) { slash_emit(a, v, SLASH_SURROUND, t, id, tb, idb); return true; }
    if (sb < s && t < tb) { slash_emit(a, v, SLASH_SURROUND, tb, idb, t, id); return true; }
    return false;
}

// the first row at or behind `from` (batch order) that carries v's bit, over every table of the batch; NONE32 = none
__device__ __forceinline__ uint32_t slash_next_row(const SlashArgs& a, uint64_t v, uint32_t from)
{
    uint32_t best = NONE32;
    for (uint32_t ti = 0; ti < a.n_tables; ++ti) {
        const SlashTable tb = a.tables[ti];
        const uint32_t c = tb.inv_comm[v];
        if (c == NONE32) continue;
        const uint32_t kb = tb.crow_start[c], ke = tb.crow_start[c + 1];
        if (kb == ke) continue;
        const uint32_t i = tb.inv_pos[v];
        for (uint32_t k = kb; k < ke; ++k) {
            const uint32_t r = a.crow_list[k];
            if (r < from) continue;
            if (r >= best) break;  // ascending inside a committee
            const SlashRow row = a.rows[r];
            if (i < row.n_bits && ((a.bits[(uint64_t)row.bits_byte + (i >> 3)] >> (i & 7)) & 1u)) { best = r; break; }
        }
    }
    return best;
}

}  // namespace

__global__ void __launch_bounds__(256)
k_slash_scan(const SlashArgs a)
{
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n_val) return;
    const uint32_t H = a.history;
    bool any = false;
    uint32_t from = 0;
    for (;;) {
        // ---- the next SLASH_NV new votes of this validator, in batch order
        uint32_t ns[SLASH_NV], nt[SLASH_NV], nid[SLASH_NV];
        int k = 0;
        while (k < SLASH_NV) {
            const uint32_t r = slash_next_row(a, v, from);
            if (r == NONE32) break;
            const SlashRow row = a.rows[r];
#pragma unroll
            for (int q = 0; q < SLASH_NV; ++q)
                if (q == k) { ns[q] = row.source; nt[q] = row.target; nid[q] = row.id; }
            from = r + 1;
            ++k;
        }
        if (k == 0) break;
        // ---- which of them meet their own data again (nothing happens), which will be recorded.  The record a vote sees
        // for its target epoch is the one in memory or, where that slot is empty, the first earlier new vote for that epoch.
        bool skip[SLASH_NV], recd[SLASH_NV];
#pragma unroll
        for (int j = 0; j < SLASH_NV; ++j) {
            skip[j] = recd[j] = false;
            if (j >= k) continue;
            const uint64_t at = (uint64_t)(nt[j] % H) * a.n_val + v;
            if (a.rec[at] != 0) {
                skip[j] = a.ids[at] == nid[j];
            } else {
                bool first = true;
#pragma unroll
                for (int i = 0; i < j; ++i)
                    if (first && nt[i] == nt[j]) { first = false; skip[j] = nid[i] == nid[j]; }
                recd[j] = first;
            }
        }
        // ---- ONE pass over the history against all of them
        for (uint32_t slot = 0; slot < H; ++slot) {
            const uint64_t at = (uint64_t)slot * a.n_val + v;
            const unsigned long long m = a.rec[at];
            if (m == 0) continue;
            const uint32_t tb = (uint32_t)(m >> 32) - 1u, sb = (uint32_t)m;
            bool hit = false;
#pragma unroll
            for (int j = 0; j < SLASH_NV; ++j)
                if (j < k && !skip[j]) hit |= tb == nt[j] || (ns[j] < sb && tb < nt[j]) || (sb < ns[j] && nt[j] < tb);
            if (!hit) continue;
            const uint32_t idb = a.ids[at];  // read on a hit only
#pragma unroll
            for (int j = 0; j < SLASH_NV; ++j)
                if (j < k && !skip[j]) any |= slash_compare(a, (uint32_t)v, ns[j], nt[j], nid[j], sb, tb, idb);
        }
        // ---- ... and against the earlier new votes that are being recorded
#pragma unroll
        for (int j = 1; j < SLASH_NV; ++j) {
            if (j >= k || skip[j]) continue;
#pragma unroll
            for (int i = 0; i < j; ++i)
                if (recd[i]) any |= slash_compare(a, (uint32_t)v, ns[j], nt[j], nid[j], ns[i], nt[i], nid[i]);
        }
        // ---- record
#pragma unroll
        for (int j = 0; j < SLASH_NV; ++j) {
            if (!recd[j]) continue;
            const uint64_t at = (uint64_t)(nt[j] % H) * a.n_val + v;
            a.rec[at] = ((unsigned long long)(nt[j] + 1u) << 32) | ns[j];
            a.ids[at] = nid[j];
        }
        if (k < SLASH_NV) break;
    }
    if (any && a.flags) a.flags[v] |= SLASH_VAL_EQUIVOCATING;  // pe:1459-1461; a byte of this lane's own
}

void launch_slash_scan(hipStream_t s, const SlashArgs& a)
{
    if (a.n_val == 0 || a.history == 0) return;
    hipLaunchKernelGGL(k_slash_scan, dim3((unsigned)((a.n_val + 255) / 256)), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------ rows, ids and lists from a resident aggregate
namespace {

constexpr int32_t SL_BITS_LENGTH = 10, SL_FUTURE_TARGET = 32, SL_TOO_OLD = 33, SL_TABLE_FULL = 34;  // include/posevo.h

struct Data8 { uint4 q[8]; };  // one AttestationData as struct pe_attestation lays it out: 128 bytes
__device__ __forceinline__ void load_data(Data8& d, const uint4* p)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) d.q[k] = p[k];
}
__device__ __forceinline__ bool same_data(const Data8& d, const uint4* p)
{
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint4 x = p[k];
        diff |= (x.x ^ d.q[k].x) | (x.y ^ d.q[k].y) | (x.z ^ d.q[k].z) | (x.w ^ d.q[k].w);
    }
    return diff == 0;
}
__device__ __forceinline__ uint32_t slash_mix(uint32_t h, uint32_t v)
{
    h ^= v;
    h *= 0x9E3779B1u;
    return h ^ (h >> 15);
}
// the key of both tables: the 32 little-endian words of the data, folded in order (tests/test_gpu_slasher_rows.py holds a
// twin of it to place collisions)
__device__ __forceinline__ uint32_t slash_data_hash(const Data8& d)
{
    uint32_t h = 0x85EBCA6Bu;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        h = slash_mix(h, d.q[k].x);
        h = slash_mix(h, d.q[k].y);
        h = slash_mix(h, d.q[k].z);
        h = slash_mix(h, d.q[k].w);
    }
    return h;
}
__device__ __forceinline__ const uint4* group_data(const SlashRowsArgs& a, const AttGroup& G)
{
    return static_cast<const uint4*>(a.rows) + (size_t)9 * G.rep;
}
__device__ __forceinline__ unsigned long long u64_of(uint32_t lo, uint32_t hi) { return ((unsigned long long)hi << 32) | lo; }

}  // namespace

__global__ void __launch_bounds__(256)
k_slash_rows_check(const SlashRowsArgs a)
{
    const uint32_t g = blockIdx.x * SLASH_ROWS_WG + threadIdx.x;
    if (g >= a.n_groups) return;
    const AttGroup G = a.grp[g];
    const uint4* p = group_data(a, G);
    const uint4 q3 = p[3], q5 = p[5];
    const unsigned long long sep = u64_of(q3.x, q3.y), tep = u64_of(q5.z, q5.w);
    if (tep >= 0xFFFFFFFEull || sep >= 0xFFFFFFFFull) atomicOr(a.err, 1u);  // the whole call fails (engine_slash.cpp)
    int32_t st = 0;
    if (tep > a.window) st = SL_FUTURE_TARGET;
    else if (tep + a.history <= a.window) st = SL_TOO_OLD;
    // no table among the two candidates, or no such committee; the aggregate's own len(bits) != len(committee) is left to the
    // slasher's rule (bits longer than the committee take part, as with host rows: the group's committee is resolved then)
    else if (G.status_agg && G.status_agg != (uint32_t)SL_BITS_LENGTH) st = (int32_t)G.status_agg;
    else if (G.n_bits < G.size) st = SL_BITS_LENGTH;
    a.status[g] = st;
}

__global__ void __launch_bounds__(256)
k_slash_rows_lookup(const SlashRowsArgs a)
{
    const uint32_t g = blockIdx.x * SLASH_ROWS_WG + threadIdx.x;
    if (g >= a.n_groups) return;
    uint32_t id = NONE32, cslot = NONE32;
    if (a.status[g] == 0) {
        const AttGroup G = a.grp[g];
        Data8 d;
        load_data(d, group_data(a, G));
        const uint32_t h = slash_data_hash(d);
        const uint32_t slot = a.slot_of_table[G.table & 1u];
        const uint32_t* tab = a.tab + (size_t)slot * (a.tab_mask + 1u);
        const uint4* data = reinterpret_cast<const uint4*>(a.data) + (size_t)slot * a.max_data * 8;
        for (uint32_t at = h & a.tab_mask;; at = (at + 1) & a.tab_mask) {  // at most half of the entries are taken
            const uint32_t e = tab[at];
            if (e == NONE32) break;
            if (same_data(d, data + (size_t)e * 8)) { id = e; break; }
        }
        if (id == NONE32) {  // new to the slot: the lowest group among those that carry this data will insert it
            cslot = h & a.cand_mask;
            for (;;) {
                const uint32_t prev = atomicCAS(&a.cand_tab[cslot], NONE32, g);
                if (prev == NONE32) break;
                if (same_data(d, group_data(a, a.grp[prev]))) {  // any group of the entry carries the entry's data
                    atomicMin(&a.cand_tab[cslot], g);
                    break;
                }
                cslot = (cslot + 1) & a.cand_mask;
            }
        }
    }
    a.id[g] = id;
    a.cand_slot[g] = cslot;
}

__global__ void __launch_bounds__(256)
k_slash_rows_ids(const SlashRowsArgs a)
{
    __shared__ uint32_t s_wave[SLASH_ROWS_WG / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t slot0 = a.slot_of_table[0], slot1 = a.slot_of_table[1];
    const uint32_t cnt0 = a.count[slot0], cnt1 = a.count[slot1];
    uint32_t carry0 = 0, carry1 = 0;  // new data of each slot in the tiles in front of this one
    for (uint32_t base = 0; base < a.n_groups; base += SLASH_ROWS_WG) {
        const uint32_t g = base + tid;
        bool leader = false;
        uint32_t t = 0;
        if (g < a.n_groups) {
            const uint32_t cs = a.cand_slot[g];
            if (cs != NONE32 && a.cand_tab[cs] == g) { leader = true; t = a.grp[g].table & 1u; }
        }
        const uint32_t v = leader ? (t ? 0x10000u : 1u) : 0u;  // both slots' counts in one word: a tile holds <= 256
        const uint32_t inc = wave_incl_scan(v);
        __syncthreads();  // the previous tile has read s_wave
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < SLASH_ROWS_WG / 64; ++w) {
            const uint32_t x = s_wave[w];
            if (w < wave) before += x;
            total += x;
        }
        if (leader) {
            const uint32_t ex = before + inc - v;
            const uint32_t nid = t ? cnt1 + carry1 + (ex >> 16) : cnt0 + carry0 + (ex & 0xFFFFu);
            if (nid < a.max_data) {
                const uint32_t slot = t ? slot1 : slot0;
                Data8 d;
                load_data(d, group_data(a, a.grp[g]));
                uint32_t* tab = a.tab + (size_t)slot * (a.tab_mask + 1u);
                uint32_t at = slash_data_hash(d) & a.tab_mask;
                while (atomicCAS(&tab[at], NONE32, nid) != NONE32) at = (at + 1) & a.tab_mask;  // distinct data: claim a free entry
                uint4* out = reinterpret_cast<uint4*>(a.data) + ((size_t)slot * a.max_data + nid) * 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) out[k] = d.q[k];
                a.id[g] = nid;
            } else {
                a.id[g] = SLASH_ID_FULL;
            }
        }
        carry0 += total & 0xFFFFu;
        carry1 += total >> 16;
    }
    // (a slot without new data is left alone: at epoch 0 both candidate tables name the same slot)
    if (tid == 0 && carry0) a.count[slot0] = min(cnt0 + carry0, a.max_data);
    if (tid == 0 && carry1) a.count[slot1] = min(cnt1 + carry1, a.max_data);
}

__global__ void __launch_bounds__(256)
k_slash_rows_emit(const SlashRowsArgs a)
{
    const uint32_t g = blockIdx.x * SLASH_ROWS_WG + threadIdx.x;
    if (g >= a.n_groups) return;
    SlashRow r;
    r.bits_byte = r.n_bits = r.source = r.target = r.id = 0;  // n_bits = 0: no position is below it, the scan skips the row
    r.pad[0] = r.pad[1] = r.pad[2] = 0;
    if (a.status[g] == 0) {
        const uint32_t cs = a.cand_slot[g];
        const uint32_t id = cs == NONE32 ? a.id[g] : a.id[a.cand_tab[cs]];
        if (id == SLASH_ID_FULL) {
            a.status[g] = SL_TABLE_FULL;
        } else {
            const AttGroup G = a.grp[g];
            const uint4* p = group_data(a, G);
            r.bits_byte = 4u * G.out_word;
            r.n_bits = G.size;
            r.source = p[3].x;
            r.target = p[5].z;
            r.id = id;
        }
    }
    a.out_rows[g] = r;
}

namespace {
// the committee of a group that takes part, in the one index space of both tables; NONE32 = it takes no part
__device__ __forceinline__ uint32_t list_key(const SlashListsArgs& a, uint32_t g)
{
    if (a.rows[g].n_bits == 0) return NONE32;
    const AttGroup& G = a.grp[g];
    return ((G.table & 1u) ? a.n_committees[0] : 0u) + G.pos;
}
}  // namespace

__global__ void __launch_bounds__(256)
k_slash_lists_count(const SlashListsArgs a)
{
    const uint32_t g = blockIdx.x * SLASH_ROWS_WG + threadIdx.x;
    if (g >= a.n_groups) return;
    const uint32_t key = list_key(a, g);
    if (key != NONE32) atomicAdd(&a.cnt[key], 1u);
}

__global__ void __launch_bounds__(256)
k_slash_lists_scan(const SlashListsArgs a)
{
    __shared__ uint32_t s_wave[SLASH_ROWS_WG / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nc = a.n_committees[0] + a.n_committees[1];
    if (tid == 0)
        for (uint32_t t = 0; t < a.n_tables; ++t) a.tables[t] = a.table_val[t];
    uint32_t carry = 0;
    for (uint32_t base = 0; base <= nc; base += SLASH_ROWS_WG) {  // entry nc: the end mark
        const uint32_t i = base + tid;
        const uint32_t v = i < nc ? a.cnt[i] : 0u;
        const uint32_t inc = wave_incl_scan(v);
        __syncthreads();  // the previous tile has read s_wave
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < SLASH_ROWS_WG / 64; ++w) {
            const uint32_t x = s_wave[w];
            if (w < wave) before += x;
            total += x;
        }
        if (i <= nc) a.start[i] = a.cursor[i] = carry + before + inc - v;
        carry += total;
    }
}

__global__ void __launch_bounds__(256)
k_slash_lists_fill(const SlashListsArgs a)
{
    const uint32_t g = blockIdx.x * SLASH_ROWS_WG + threadIdx.x;
    if (g >= a.n_groups) return;
    const uint32_t key = list_key(a, g);
    if (key != NONE32) a.crow_list[atomicAdd(&a.cursor[key], 1u)] = g;  // the committee's own range: start[key] .. start[key + 1]
}

__global__ void __launch_bounds__(256)
k_slash_lists_sort(const SlashListsArgs a)
{
    const uint32_t c = blockIdx.x * SLASH_ROWS_WG + threadIdx.x;
    if (c >= a.n_committees[0] + a.n_committees[1]) return;
    const uint32_t kb = a.start[c], ke = a.start[c + 1];
    uint32_t* out = a.crow_list;
    for (uint32_t k = kb + 1; k < ke; ++k) {  // a committee has a handful of groups: insertion sort
        const uint32_t x = out[k];
        uint32_t j = k;
        for (; j > kb && out[j - 1] > x; --j) out[j] = out[j - 1];
        out[j] = x;
    }
}

__global__ void __launch_bounds__(256)
k_slash_table_build(const uint8_t* data, const uint32_t* count, uint32_t* tab, uint32_t max_data, uint32_t tab_mask)
{
    const uint32_t slot = blockIdx.y, id = blockIdx.x * SLASH_ROWS_WG + threadIdx.x;
    if (id >= min(count[slot], max_data)) return;
    Data8 d;
    load_data(d, reinterpret_cast<const uint4*>(data) + ((size_t)slot * max_data + id) * 8);
    uint32_t* t = tab + (size_t)slot * (tab_mask + 1u);
    uint32_t at = slash_data_hash(d) & tab_mask;
    while (atomicCAS(&t[at], NONE32, id) != NONE32) at = (at + 1) & tab_mask;
}

static unsigned slash_rows_blocks(uint32_t n) { return (n + SLASH_ROWS_WG - 1) / SLASH_ROWS_WG; }
void launch_slash_rows_check(hipStream_t s, const SlashRowsArgs& a)
{
    if (a.n_groups) hipLaunchKernelGGL(k_slash_rows_check, dim3(slash_rows_blocks(a.n_groups)), dim3(SLASH_ROWS_WG), 0, s, a);
}
void launch_slash_rows_lookup(hipStream_t s, const SlashRowsArgs& a)
{
    if (a.n_groups) hipLaunchKernelGGL(k_slash_rows_lookup, dim3(slash_rows_blocks(a.n_groups)), dim3(SLASH_ROWS_WG), 0, s, a);
}
void launch_slash_rows_ids(hipStream_t s, const SlashRowsArgs& a)
{
    if (a.n_groups) hipLaunchKernelGGL(k_slash_rows_ids, dim3(1), dim3(SLASH_ROWS_WG), 0, s, a);
}
void launch_slash_rows_emit(hipStream_t s, const SlashRowsArgs& a)
{
    if (a.n_groups) hipLaunchKernelGGL(k_slash_rows_emit, dim3(slash_rows_blocks(a.n_groups)), dim3(SLASH_ROWS_WG), 0, s, a);
}
void launch_slash_rows_lists(hipStream_t s, const SlashListsArgs& a)
{
    const uint32_t nc = a.n_committees[0] + a.n_committees[1];
    if (!a.n_groups || !nc) return;
    const dim3 per_group(slash_rows_blocks(a.n_groups)), per_committee(slash_rows_blocks(nc)), wg(SLASH_ROWS_WG);
    hipLaunchKernelGGL(k_slash_lists_count, per_group, wg, 0, s, a);
    hipLaunchKernelGGL(k_slash_lists_scan, dim3(1), wg, 0, s, a);
    hipLaunchKernelGGL(k_slash_lists_fill, per_group, wg, 0, s, a);
    hipLaunchKernelGGL(k_slash_lists_sort, per_committee, wg, 0, s, a);
}
void launch_slash_table_build(hipStream_t s, const uint8_t* data, const uint32_t* count, uint32_t* tab, uint32_t max_data,
                              uint32_t tab_mask, uint32_t history)
{
    if (!max_data || !history) return;
    hipLaunchKernelGGL(k_slash_table_build, dim3(slash_rows_blocks(max_data), history), dim3(SLASH_ROWS_WG), 0, s, data, count,
                       tab, max_data, tab_mask);
}

}  // namespace posevo
