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
#include "kernels.h"

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

}  // namespace posevo
