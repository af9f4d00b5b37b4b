// fc_bodies.inc -- the fork-choice kernels' bodies: device functions that take their block index (or their wave's group)
// as an argument, with the helpers and constants they need, the POSEVO_FC_PRIO macro and the host helpers that size their
// grids and their LDS.  Included at file scope by fc_kernels.hip, which wraps each body in a __global__ kernel of its own
// and launches it, and by pair_kernels.hip, which runs the same bodies as block ranges of the paired launches: one text, so
// the two forms cannot differ.  Like fp381_lazy.inc it has no include guard; unlike it, it opens namespace posevo itself.
// No __global__ function, no launcher and no __device__ variable belongs here.
#include <algorithm>
#include "kernels.h"
#include "wave64.h"

namespace posevo {

constexpr uint32_t VAL_ACTIVE = 0x01u, VAL_SLASHED = 0x02u, VAL_EQUIVOCATING = 0x04u;

// The kernels in front of a head (union, LMD, votes, tree) are latency-critical guests beside the long G1 kernels of
// the previous step; the SIMD's issue arbiter serves the oldest wave first, i.e. the G1 kernel's.  Raising their wave
// priority puts them first (POSEVO_FC_PRIO=0 builds without it, for comparison).
#ifndef POSEVO_FC_PRIO_LEVEL
#define POSEVO_FC_PRIO_LEVEL 3
#endif
#if POSEVO_FC_PRIO_LEVEL > 0
#define POSEVO_FC_PRIO() __builtin_amdgcn_s_setprio(POSEVO_FC_PRIO_LEVEL)
#else
#define POSEVO_FC_PRIO() ((void)0)
#endif

// ------------------------------------------------------------------ votes
constexpr int VOTES_WG = 512;  // 256 lanes: 21 us, 512: 15.8, 1024: 15.4 at 1 M validators / 64 workgroups
constexpr int VOTES_PER_THREAD = 4;

// QUADS = quads of validators in flight per lane and iteration.  2: the stand-alone get_head (63 VGPRs, fastest).
// 1: the lean form for pipelined steps, where this kernel runs BESIDE k_g1_accumulate of the previous aggregate:
// that kernel's two waves per SIMD hold 464 of the 512 registers, and only a wave of <= 48 fits into the rest and can
// start before the accumulation's last workgroup retires.
// (body: block index and grid size are arguments, hist = the workgroup's n_blocks bins of LDS -- the same code runs as a
// kernel of its own and as one block range of a paired launch, pair_kernels.hip)
template <int QUADS>
__device__ __forceinline__ void votes_body(const uint32_t bid, const uint32_t nblk, const VotesArgs& a,
                                           unsigned long long* __restrict__ hist)
{
    const uint32_t* __restrict__ vote_block = a.vote_block;
    const uint64_t* __restrict__ eff_balance = a.eff_balance;
    const uint8_t* __restrict__ flags = a.flags;
    const uint64_t n_val = a.n_val;
    const uint32_t filter_slashed = a.filter_slashed;
    const uint32_t* __restrict__ pos_of_idx = a.pos_of_idx;
    const uint32_t n_blocks = a.n_blocks;
    unsigned long long* __restrict__ direct = reinterpret_cast<unsigned long long*>(a.direct);
    VoteTotals* __restrict__ totals = a.totals;
    const uint32_t* __restrict__ vote_slot = a.vote_slot;
    const uint32_t min_vote_slot = a.min_vote_slot;
    for (uint32_t b = threadIdx.x; b < n_blocks; b += VOTES_WG) hist[b] = 0;
    __syncthreads();

    unsigned long long act_bal = 0;
    uint32_t act_num = 0;
    const uint64_t n_quads = (n_val + VOTES_PER_THREAD - 1) / VOTES_PER_THREAD;
    const uint64_t stride = (uint64_t)nblk * VOTES_WG;
    // QUADS quads (4 validators each: 16 + 32 + 4 bytes of vector loads) in flight per lane per iteration
    for (uint64_t q0 = (uint64_t)bid * VOTES_WG + threadIdx.x; q0 < n_quads; q0 += QUADS * stride) {
        uint32_t vb[4 * QUADS];
        unsigned long long bal[4 * QUADS];
        uint32_t fl[4 * QUADS];
#pragma unroll
        for (int u = 0; u < QUADS; ++u) {
            const uint64_t q = q0 + u * stride;
            const uint64_t v0 = q * VOTES_PER_THREAD;
            if (q < n_quads && v0 + 4 <= n_val) {  // arrays are 16-byte aligned and v0 % 4 == 0
                const uint4 t = *reinterpret_cast<const uint4*>(vote_block + v0);
                vb[4 * u] = t.x; vb[4 * u + 1] = t.y; vb[4 * u + 2] = t.z; vb[4 * u + 3] = t.w;
                const ulonglong2 b01 = *reinterpret_cast<const ulonglong2*>(eff_balance + v0);
                const ulonglong2 b23 = *reinterpret_cast<const ulonglong2*>(eff_balance + v0 + 2);
                bal[4 * u] = b01.x; bal[4 * u + 1] = b01.y; bal[4 * u + 2] = b23.x; bal[4 * u + 3] = b23.y;
                const uint32_t f = *reinterpret_cast<const uint32_t*>(flags + v0);
                fl[4 * u] = f & 0xff; fl[4 * u + 1] = (f >> 8) & 0xff; fl[4 * u + 2] = (f >> 16) & 0xff; fl[4 * u + 3] = f >> 24;
                if (vote_slot) {  // vote-expiry variant (RLMD-GHOST, pe:1585-1596): an expired message counts as none
                    const uint4 sl = *reinterpret_cast<const uint4*>(vote_slot + v0);
                    if (sl.x < min_vote_slot) vb[4 * u] = NONE32;
                    if (sl.y < min_vote_slot) vb[4 * u + 1] = NONE32;
                    if (sl.z < min_vote_slot) vb[4 * u + 2] = NONE32;
                    if (sl.w < min_vote_slot) vb[4 * u + 3] = NONE32;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool ok = q < n_quads && v0 + k < n_val;
                    vb[4 * u + k] = ok ? vote_block[v0 + k] : NONE32;
                    bal[4 * u + k] = ok ? eff_balance[v0 + k] : 0ull;
                    fl[4 * u + k] = ok ? flags[v0 + k] : 0u;
                    if (ok && vote_slot && vote_slot[v0 + k] < min_vote_slot) vb[4 * u + k] = NONE32;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4 * QUADS; ++k) {
            if (!(fl[k] & VAL_ACTIVE)) continue;
            act_bal += bal[k];
            act_num += 1;
            if (fl[k] & VAL_EQUIVOCATING) continue;
            if (filter_slashed && (fl[k] & VAL_SLASHED)) continue;
            if (vb[k] >= n_blocks) continue;  // NONE32 = no latest message
            atomicAdd(&hist[vb[k]], bal[k]);  // ds_add_u64
        }
    }
    // active-balance totals: wave reduce -> LDS -> ONE plain store per workgroup into its own slot
    // (same-address device-scope atomics cost ~12 ns each and serialise: 4096 of them were 50 us)
    __shared__ unsigned long long wg_tot[2];
    if (threadIdx.x == 0) { wg_tot[0] = 0; wg_tot[1] = 0; }
    act_bal = wave_sum(act_bal);
    act_num = wave_sum(act_num);
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && act_num) {
        atomicAdd(&wg_tot[0], act_bal);
        atomicAdd(&wg_tot[1], (unsigned long long)act_num);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        totals[bid].total_active_balance = wg_tot[0];
        totals[bid].num_active = wg_tot[1];
    }
    // The slots no workgroup of THIS launch owns must read zero: after an in-place all-reduce they hold the other ranks'
    // sums of the previous round (ranks with unequal shards launch different grids), and a shrinking registry leaves
    // stale partials behind (ADVICE r2: the sharded head double-counted them).  Workgroup 0 clears them: no memset.
    if (bid == 0)
        for (uint32_t j = nblk + threadIdx.x; j < (uint32_t)VOTES_MAX_WG; j += VOTES_WG) {
            totals[j].total_active_balance = 0;
            totals[j].num_active = 0;
        }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n_blocks; b += VOTES_WG) {
        const unsigned long long w = hist[b];
        if (w) atomicAdd(&direct[pos_of_idx[b]], w);
    }
}
// workgroups of a votes launch over n_val validators
inline unsigned votes_blocks(uint64_t n_val)
{
    const uint64_t n_quads = (n_val + VOTES_PER_THREAD - 1) / VOTES_PER_THREAD;
    uint64_t blocks = (n_quads + VOTES_WG - 1) / VOTES_WG;
    // Grid-stride over few, fat workgroups: every workgroup zeroes, scans and flushes a whole n_blocks histogram, so
    // at 1 M validators 64 workgroups (16 K validators each) beat 256 (k_votes 16 us vs 23 us, get_head p50 46 vs 53 us);
    // the count grows with the registry up to one workgroup per CU (launch_votes, fc_kernels.hip, has the measured alternatives).
    uint64_t cap = n_val / 16384;
    cap = cap < 64 ? 64 : cap > (uint64_t)VOTES_MAX_WG ? (uint64_t)VOTES_MAX_WG : cap;
    return (unsigned)(blocks > cap ? cap : blocks);
}

// ------------------------------------------------------------------ tree
// (A fused get_head -- votes phase in every workgroup, tree phase in the last one to pass a device-scope ticket --
// was built and measured: p50 46 us against 33 us for the two launches below.  The fat 1024-lane / 147 KB-LDS
// workgroups slow the votes phase by more than the saved launch gap; dropped.)
// The kernel is instantiated for a few items-per-thread counts: 1024 lanes x PER >= n, picked by the host from the
// block count.  The per-item loops, not the ~25 barriers, set the time: a 4096-block tree measures 19.8 us at
// 1024 x 4, 26 us at 512 x 8 or 1024 x 8 (half the lanes idle) and 34 us at 256 x 16.
//
// LDS index skew: thread t owns items PER*t .. PER*t+PER-1, i.e. a lane stride of PER elements = a PER-way (u32) bank
// conflict on every own-item access.  i -> i + i/PER turns the stride into PER+1 (odd): conflict-free.
template <int PER>
__host__ __device__ __forceinline__ uint32_t SKT(uint32_t i) { return PER == 1 ? i : i + i / PER; }
// largest skewed index over the shapes in use: 8192 blocks at PER = 8 (PER = 4 only serves n <= 4096)
constexpr uint32_t TREE_LDS_ENTRIES = TREE_MAX_BLOCKS + 2 + ((TREE_MAX_BLOCKS + 2) >> 3) + 1;

// Exclusive prefix sum over n <= 8192 values held as 8 consecutive items per thread.
// out[SK(i)] (LDS, n+1 entries) = sum of in[0..i); wave shuffles + one LDS hop across the 16 waves.
template <typename T, int TREE_WG, int TREE_PER_THREAD>
__device__ __forceinline__ void block_exclusive_scan(const T (&item)[TREE_PER_THREAD], T* out, T* wave_tot, uint32_t n)
{
    auto SK = [](uint32_t i) { return SKT<TREE_PER_THREAD>(i); };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T local = 0;
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) local += item[k];
    const T incl = wave_incl_scan(local);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    T base = 0;
    for (int w = 0; w < wave; ++w) base += wave_tot[w];
    T run = base + incl - local;
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) {
        const uint32_t i = tid * TREE_PER_THREAD + k;
        if (i <= n) out[SK(i)] = run;
        run += item[k];
    }
    if (tid == TREE_WG - 1 && (uint32_t)(TREE_WG * TREE_PER_THREAD) <= n) out[SK(n)] = run;
    __syncthreads();
}

// Two exclusive prefix sums (u64 weights, u32 leaf counts) through ONE pair of barriers.
template <int TREE_WG, int TREE_PER_THREAD>
__device__ __forceinline__ void block_exclusive_scan2(const unsigned long long (&a)[TREE_PER_THREAD], unsigned long long* out_a,
                                                      unsigned long long* wave_a, const uint32_t (&b)[TREE_PER_THREAD],
                                                      uint32_t* out_b, uint32_t* wave_b, uint32_t n)
{
    auto SK = [](uint32_t i) { return SKT<TREE_PER_THREAD>(i); };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long la = 0;
    uint32_t lb = 0;
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) { la += a[k]; lb += b[k]; }
    unsigned long long ia = la;
    uint32_t ib = lb;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {  // (the two scans interleaved: not wave_incl_scan twice, the kernels' code differs)
        const unsigned long long oa = __shfl_up(ia, off, 64);
        const uint32_t ob = __shfl_up(ib, off, 64);
        if (lane >= off) { ia += oa; ib += ob; }
    }
    if (lane == 63) { wave_a[wave] = ia; wave_b[wave] = ib; }
    __syncthreads();
    unsigned long long base_a = 0;
    uint32_t base_b = 0;
    for (int w = 0; w < wave; ++w) { base_a += wave_a[w]; base_b += wave_b[w]; }
    unsigned long long ra = base_a + ia - la;
    uint32_t rb = base_b + ib - lb;
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) {
        const uint32_t i = tid * TREE_PER_THREAD + k;
        if (i <= n) { out_a[SK(i)] = ra; out_b[SK(i)] = rb; }
        ra += a[k];
        rb += b[k];
    }
    if (tid == TREE_WG - 1 && (uint32_t)(TREE_WG * TREE_PER_THREAD) <= n) { out_a[SK(n)] = ra; out_b[SK(n)] = rb; }
    __syncthreads();
}

// LEAN: the form that fits beside a running k_g1_accumulate (one wave of 232 VGPRs per SIMD in streaming steps leaves
// 280 registers per SIMD lane -- rounds 2-3: two waves of 168, 176 left; a 512-lane workgroup = two waves per SIMD of <= 88
// here, where the 1024-lane shapes take 4 x 84).  Parent, rank and block index are loaded where they
// are used instead of up front -- three more round trips to L2, ~6 us -- so only pipelined calls use it.
// lds_entries: skewed index range of this launch (the host sizes the dynamic LDS for the block count at hand, not for
// the 8192-block maximum: 82 KB at 4096 blocks leaves room for another kernel's workgroup on the CU).
template <int TREE_WG, int TREE_PER_THREAD, bool LEAN = false>
__device__ __forceinline__ void tree_body(const TreeArgs& a, const uint32_t lds_entries, unsigned char* smem)  // ONE workgroup
{
    const TreeDev& tree = a.tree;
    unsigned long long* __restrict__ direct = reinterpret_cast<unsigned long long*>(a.direct);
    const VoteTotals* __restrict__ totals = a.totals;
    const unsigned long long ov_balance = a.ov_balance, ov_num = a.ov_num;
    const int use_override = a.use_override;
    const uint32_t justified_pos = a.justified_pos, boost_pos = a.boost_pos;
    const unsigned long long slots_per_epoch = a.slots_per_epoch, boost_percent = a.boost_percent,
                             balance_increment = a.balance_increment;
    unsigned long long* __restrict__ weights_by_idx = reinterpret_cast<unsigned long long*>(a.weights_by_idx);
    uint32_t* __restrict__ head_idx = a.head_idx;
    const int clear_direct = a.clear_direct;
    // LDS plan (n <= 8192, skewed indices):  S u64 (later bestW) | L u32 (later bestRank) | jump u32 | scratch
    // u64 regions first so that every 64-bit LDS access (ds_*_b64, ds_add_u64, ds_max_u64) is 8-byte aligned
    unsigned long long* S = reinterpret_cast<unsigned long long*>(smem);
    unsigned long long* wave_tot64 = S + lds_entries;         // 16 waves
    unsigned long long* tot = wave_tot64 + 16;                // 2 words
    uint32_t* L = reinterpret_cast<uint32_t*>(tot + 2);
    uint32_t* jump = L + lds_entries;
    uint32_t* wave_tot32 = jump + lds_entries;                // 16 waves

    const uint32_t n = tree.n;
    const int tid = threadIdx.x;
    auto SK = [](uint32_t i) { return SKT<TREE_PER_THREAD>(i); };

    // every global read up front: one round trip of memory latency for the whole kernel
    unsigned long long w_item[TREE_PER_THREAD];
    uint32_t l_item[TREE_PER_THREAD], sz[TREE_PER_THREAD], par_g[TREE_PER_THREAD], rk_g[TREE_PER_THREAD],
        idx_g[TREE_PER_THREAD];
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) {
        const uint32_t i = tid * TREE_PER_THREAD + k;
        const bool in = i < n;
        sz[k] = in ? tree.size[i] : 0u;
        w_item[k] = in ? direct[i] : 0ull;
        l_item[k] = (in && tree.leaf_ok[i]) ? 1u : 0u;
        if (!LEAN) {
            par_g[k] = in ? tree.parent[i] : NONE32;
            rk_g[k] = in ? tree.rank[i] + 1 : 0u;  // 0 = "no viable child yet"
            idx_g[k] = in ? tree.idx_of_pos[i] : 0u;
        }
    }
    unsigned long long t_bal = 0, t_num = 0;
    if (boost_pos != NONE32 && !use_override) {
        for (int j = tid; j < VOTES_MAX_WG; j += TREE_WG) {
            t_bal += totals[j].total_active_balance;
            t_num += totals[j].num_active;
        }
    }
    if (clear_direct) {  // leave the engine's weight buffer zeroed for the next get_head (no memset launch)
#pragma unroll
        for (int k = 0; k < TREE_PER_THREAD; ++k) {
            const uint32_t i = tid * TREE_PER_THREAD + k;
            if (i < n) direct[i] = 0ull;
        }
    }
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) l_item[k] = (l_item[k] && sz[k] == 1) ? 1u : 0u;

    // proposer boost (A.1): one extra "vote" of proposer_score at the boosted block -- it then
    // counts for that block and every ancestor, exactly the get_ancestor(...) == root test.
    if (boost_pos != NONE32) {
        // sum the votes kernel's per-workgroup partial totals (all ranks' partials after the all-reduce)
        if (tid == 0) { tot[0] = 0; tot[1] = 0; }
        __syncthreads();
        if (t_num) { atomicAdd(&tot[0], t_bal); atomicAdd(&tot[1], t_num); }
        __syncthreads();
        unsigned long long total = use_override ? ov_balance : tot[0];
        const unsigned long long num = use_override ? ov_num : tot[1];
        unsigned long long boost = 0;
        if (num > 0) {
            if (total < balance_increment) total = balance_increment;  // get_total_balance's max()
            const unsigned long long avg_balance = total / num;
            const unsigned long long committee_size = num / slots_per_epoch;
            const unsigned long long committee_weight = committee_size * avg_balance;
            // committee_weight * boost_percent can exceed 64 bits only beyond 1.8e17 Gwei * percent: split
            const unsigned long long q = committee_weight / 100, r = committee_weight % 100;
            boost = q * boost_percent + (r * boost_percent) / 100;
        }
#pragma unroll
        for (int k = 0; k < TREE_PER_THREAD; ++k)
            if ((uint32_t)(tid * TREE_PER_THREAD + k) == boost_pos) w_item[k] += boost;
    }

    block_exclusive_scan2<TREE_WG, TREE_PER_THREAD>(w_item, S, wave_tot64, l_item, L, wave_tot32, n);

    unsigned long long W[TREE_PER_THREAD];
    uint32_t viable = 0;
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) {
        const uint32_t i = tid * TREE_PER_THREAD + k;
        W[k] = 0;
        if (i < n) {
            W[k] = S[SK(i + sz[k])] - S[SK(i)];
            if (L[SK(i + sz[k])] - L[SK(i)] > 0) viable |= 1u << k;
            weights_by_idx[LEAN ? tree.idx_of_pos[i] : idx_g[k]] = W[k];
        }
    }
    __syncthreads();
    // best child, pass 1: max weight among viable children
    unsigned long long* bestW = S;
    uint32_t* bestRank = L;
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) {
        const uint32_t i = tid * TREE_PER_THREAD + k;
        if (i < n) { bestW[SK(i)] = 0; bestRank[SK(i)] = 0; }
    }
    __syncthreads();
    uint32_t par[TREE_PER_THREAD];
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) {
        const uint32_t i = tid * TREE_PER_THREAD + k;
        par[k] = ((viable >> k) & 1u) ? (LEAN ? tree.parent[i] : par_g[k]) : NONE32;  // viable => i < n
        if (par[k] != NONE32) atomicMax(&bestW[SK(par[k])], W[k]);
    }
    __syncthreads();
    // pass 2: among the heaviest, the lexicographically highest root
    if (LEAN) {
#pragma unroll
        for (int k = 0; k < TREE_PER_THREAD; ++k) {
            const uint32_t i = tid * TREE_PER_THREAD + k;
            rk_g[k] = par[k] != NONE32 ? tree.rank[i] + 1 : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k)
        if (par[k] != NONE32 && W[k] == bestW[SK(par[k])]) atomicMax(&bestRank[SK(par[k])], rk_g[k]);
    __syncthreads();
    // The descent of pe:1107-1116 without walking: the head is the deepest node of the chain justified root -> best child
    // -> best child ...  A node lies on that chain iff no ancestor-or-self below the justified root fails to be its
    // parent's best child.  In pre-order a subtree is the interval [pos, pos + size), so with g(u) = 1 for every node
    // strictly inside the justified subtree that is NOT the best child of its parent (0 elsewhere), the number of such
    // ancestors-or-self of position p is the prefix sum of  D[pos(u)] += g(u), D[pos(u) + size(u)] -= g(u)  at p --
    // one more block scan instead of up to log2(n) rounds of pointer jumping with two barriers each.  Chain nodes have
    // count 0, their pre-order positions grow downwards: the head is the largest such position inside the subtree.
    const uint32_t j_end = justified_pos + tree.size[justified_pos];
    uint32_t* D = jump;            // n + 1 signed counters
    uint32_t g_item[TREE_PER_THREAD];
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) {
        const uint32_t i = tid * TREE_PER_THREAD + k;
        const bool best = par[k] != NONE32 && W[k] == bestW[SK(par[k])] && rk_g[k] == bestRank[SK(par[k])];
        g_item[k] = (i < n && i > justified_pos && i < j_end && !best) ? 1u : 0u;
        if (i <= n) D[SK(i)] = g_item[k];   // entry n: only ever decremented
    }
    if (tid == TREE_WG - 1 && (uint32_t)(TREE_WG * TREE_PER_THREAD) <= n) D[SK(n)] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k)
        if (g_item[k]) atomicSub(&D[SK(tid * TREE_PER_THREAD + k + sz[k])], 1u);
    __syncthreads();
    uint32_t d_item[TREE_PER_THREAD];
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) {
        const uint32_t i = tid * TREE_PER_THREAD + k;
        d_item[k] = i < n ? D[SK(i)] : 0u;
    }
    uint32_t* C = L;  // bestRank's region: every lane has read it above (the scan's first barrier orders the reuse)
    block_exclusive_scan<uint32_t, TREE_WG, TREE_PER_THREAD>(d_item, C, wave_tot32, n);
    uint32_t best_pos = justified_pos;
#pragma unroll
    for (int k = 0; k < TREE_PER_THREAD; ++k) {
        const uint32_t i = tid * TREE_PER_THREAD + k;
        if (i > justified_pos && i < j_end && i < n && C[SK(i)] + d_item[k] == 0u && ((viable >> k) & 1u)) best_pos = max(best_pos, i);
    }
    best_pos = wave_max(best_pos);
    uint32_t* head_pos = wave_tot32;  // reused: the scan is through with it
    __syncthreads();
    if (tid == 0) head_pos[0] = justified_pos;
    __syncthreads();
    if ((tid & 63) == 0) atomicMax(&head_pos[0], best_pos);
    __syncthreads();
    if (tid == 0)  // host-coherent pinned word polled by the host: system-scope release
        __hip_atomic_store(head_idx, tree.idx_of_pos[head_pos[0]], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// dynamic LDS of a tree launch: skewed index of the last entry (n) of the shape, + 1, rounded up to keep the u32 regions
// 16-byte aligned; the bytes that go with it; the most any launch asks for (the opt-in beyond 64 KiB)
template <int PER>
inline uint32_t tree_lds_entries(uint32_t n) { return std::min<uint32_t>(TREE_LDS_ENTRIES, ((SKT<PER>(n + 1) + 2) + 3u) & ~3u); }
inline size_t tree_lds_bytes(uint32_t entries) { return sizeof(uint64_t) * ((size_t)entries + 18) + sizeof(uint32_t) * (2 * (size_t)entries + 16); }
constexpr size_t TREE_LDS_MAX = sizeof(uint64_t) * (TREE_LDS_ENTRIES + 18) + sizeof(uint32_t) * (2 * TREE_LDS_ENTRIES + 16);

// ------------------------------------------------------------------ bitfield union
// One wave per group.  The members' bitfields are read straight from the caller's arena as uploaded (byte offsets:
// an aligned dword pair + v_alignbyte_b32), so the host packs nothing.  Besides the OR and its popcount the wave sums
// the members' own popcounts: sum > popcount(OR) <=> two members share a bit (A.8: such aggregates are not merged --
// the aggregate signature would count that validator twice).
__device__ __forceinline__ void bits_union_body(const uint32_t g /* group of this WAVE */, const UnionArgs& a)
{
    const UnionGroup* __restrict__ groups = a.groups;
    const uint32_t* __restrict__ att_bytes = a.att_bytes;
    const uint8_t* __restrict__ bit_arena = a.bit_arena;
    uint32_t* __restrict__ out_arena = a.out_arena;
    uint32_t* __restrict__ out_info = a.out_info;
    uint32_t* __restrict__ host_arena = a.host_arena;
    uint32_t* __restrict__ host_info = a.host_info;
    uint32_t n_groups = a.n_groups;
    if (a.plan_dev) n_groups = a.plan_dev->n_groups;  // groups formed on the device: the grid covers an upper bound
    if (g >= n_groups) return;
    const int lane = threadIdx.x & 63;
    const UnionGroup d = groups[g];
    const uint32_t n_words = (d.n_bits + 31) >> 5;
    const uint32_t tail_mask = (d.n_bits & 31) ? ((1u << (d.n_bits & 31)) - 1u) : 0xFFFFFFFFu;
    const uint32_t* arena_w = reinterpret_cast<const uint32_t*>(bit_arena);  // staging block: 256-byte aligned
    uint32_t cnt = 0, member_sum = 0;
    for (uint32_t w = lane; w < n_words; w += 64) {
        uint32_t acc = 0;
        const uint32_t mask = (w == n_words - 1) ? tail_mask : 0xFFFFFFFFu;
        for (uint32_t k = 0; k < d.n_atts; ++k) {
            const uint32_t off = att_bytes[d.list_start + k] + 4u * w;
            const uint32_t lo = arena_w[off >> 2], hi = arena_w[(off >> 2) + 1];
            const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, off & 3u) & mask;
            member_sum += __builtin_popcount(v);
            acc |= v;
        }
        out_arena[d.out_word + w] = acc;
        if (host_arena) host_arena[d.out_word + w] = acc;
        cnt += __builtin_popcount(acc);
    }
    cnt = wave_sum(cnt);
    member_sum = wave_sum(member_sum);
    if (lane == 0) {
        if (out_info) {
            out_info[2 * g] = cnt;
            out_info[2 * g + 1] = member_sum - cnt;
        }
        if (host_info) {
            host_info[2 * g] = cnt;
            host_info[2 * g + 1] = member_sum - cnt;
        }
        if (a.cmpl) {  // by complement: more than half of a whole committee attests and the committee's sum is at hand
            const AttGroup& G = a.grp[g];
            uint32_t v = NONE32;
            if (G.status_agg == 0 && G.table < 2 && a.sums_ok[G.table & 1] && G.size == d.n_bits && 2 * cnt > G.size)
                v = G.pos | (G.table << 31);
            a.cmpl[g] = v;
            if (a.host_cmpl) a.host_cmpl[g] = v;
        }
    }
}

}  // namespace posevo
