// point_sum_tree.h -- what the slot-per-stripe point sums share, device only: k_g2_accumulate (g2_kernels.hip) and the two
// weighted accumulations (sigverify_kernels.hip).  Each of them gives every slot of a plan_g1 plan a stripe of its group's members,
// sums the stripe into an XYZZ partial and then adds the workgroup's partials with the tree below; k_g1_finish / k_g2_finish add
// what the workgroups leave.  (k_g1_accumulate and k_g1_tree of g1_kernels.hip have forms of their own: 13-limb partials.)
#pragma once
#include "fp_mem.h"
#include "kernels.h"

namespace posevo {

// ---------------------------------------------------------------- the slot task
__device__ __forceinline__ uint32_t plan_find_group(const G1Group* __restrict__ groups, uint32_t n_groups, uint32_t slot)
{
    uint32_t lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (groups[mid].slot_base <= slot) lo = mid; else hi = mid;
    }
    return lo;
}
// What a slot is to do: its stripe [member0, member0 + count) of the members array (count 0: a padding slot) and where its
// block's partial goes: `size` slots from the block's first make partial `out` (size 0: the slot is in no block).
struct slot_task {
    uint32_t member0, count, out, size;
};
// wg_slots: slots per workgroup of the calling kernel, the figure its plan was made for
__device__ __forceinline__ slot_task slot_task_of(const G1Group* __restrict__ groups, uint32_t n_groups, uint32_t n_slots,
                                                  uint32_t slot, uint32_t wg_slots)
{
    slot_task t = {0, 0, NONE32, 0};
    if (slot >= n_slots) return t;
    const G1Group d = groups[plan_find_group(groups, n_groups, slot)];
    const uint32_t s = slot - d.slot_base;
    const bool wide = d.log2_block > 8;
    const uint32_t block_slots = d.n_tasks == 0 ? 0u
                               : wide ? ((d.n_tasks + wg_slots - 1) / wg_slots) * wg_slots
                                      : (1u << d.log2_block);
    if (s < block_slots) {
        t.size = wide ? wg_slots : (1u << d.log2_block);
        t.out = d.out_base + (wide ? s / wg_slots : 0u);
    }
    if (s < d.n_tasks) {
        t.member0 = d.member_start + s * d.k;
        t.count = min(d.k, d.n_members - s * d.k);
    }
    return t;
}

// ---------------------------------------------------------------- the workgroup tree
// The point a tree adds: LANES lanes per slot (lane `role` of a pair holds its half), WORDS words per partial in global memory.
struct sum_g1 {
    using point = g1x;
    static constexpr int LANES = 1, WORDS = G1X_WORDS;
    static __device__ __forceinline__ void add(g1x& p, const g1x& q, bool) { g1x_add(p, q); }
    static __device__ __forceinline__ void store(uint32_t* __restrict__ dst, const g1x& p, bool) { g1x_st<fp_vec16>(dst, p); }
};
struct sum_g2 {
    using point = g2x;
    static constexpr int LANES = 2, WORDS = G2X_WORDS;
    static __device__ __forceinline__ void add(g2x& p, const g2x& q, bool role) { g2x_add(p, q, role); }
    static __device__ __forceinline__ void store(uint32_t* __restrict__ dst, const g2x& p, bool role)
    {
        g2x_st<fp_vec16>(dst, p, role);
    }
};
// LDS staging, limb-major over lane positions: word k of position L at lds[k * WG + L]; slot s = positions LANES s ...
template <int WG, class P>
__device__ __forceinline__ void xyzz_lds_store(uint32_t* lds, int pos, const P& p)
{
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        lds[k * WG + pos] = p.x.l[k];
        lds[(12 + k) * WG + pos] = p.y.l[k];
        lds[(24 + k) * WG + pos] = p.zz.l[k];
        lds[(36 + k) * WG + pos] = p.zzz.l[k];
    }
}
template <int WG, class P>
__device__ __forceinline__ void xyzz_lds_load(P& p, const uint32_t* lds, int pos)
{
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        p.x.l[k] = lds[k * WG + pos];
        p.y.l[k] = lds[(12 + k) * WG + pos];
        p.zz.l[k] = lds[(24 + k) * WG + pos];
        p.zzz.l[k] = lds[(36 + k) * WG + pos];
    }
}
// The compacting pairwise tree over a WG-lane workgroup's WG / LANES slot partials: at the level with n pairs, slot w < n adds
// slots 2w and 2w + 1 and takes their block's (out, size / 2); a block that has come down to one slot leaves the tree for
// wg_partials[out].  Blocks are powers of two and aligned, so a pair never straddles two.  Every lane of the workgroup calls this
// (it holds barriers): `acc` its slot's partial, (my_out, my_size) its task's.  lds: 48 * WG words, free to be overwritten;
// lds_out, lds_sz: WG / LANES words each.
template <class T, int WG>
__device__ __forceinline__ void point_sum_tree(uint32_t* lds, uint32_t* lds_out, uint32_t* lds_sz, const typename T::point& acc,
                                               uint32_t my_out, uint32_t my_size, uint32_t* __restrict__ wg_partials)
{
    const int tid = threadIdx.x;
    const bool role = T::LANES == 2 && (tid & 1);
    const int ws = tid / T::LANES;  // slot inside the workgroup
    if (my_size == 1) {
        T::store(wg_partials + (size_t)T::WORDS * my_out, acc, role);
        my_size = 0;
    }
    xyzz_lds_store<WG>(lds, tid, acc);
    if (!role) {
        lds_out[ws] = my_out;
        lds_sz[ws] = my_size;
    }
    __syncthreads();
    for (int n = WG / T::LANES / 2; n >= 1; n >>= 1) {
        const bool active = ws < n;
        typename T::point p1;
        uint32_t out = NONE32, sz = 0;
        bool store_lds = false;
        if (active) {
            sz = lds_sz[2 * ws];
            out = lds_out[2 * ws];
            if (sz >= 2) {
                typename T::point p2;
                xyzz_lds_load<WG>(p1, lds, T::LANES * 2 * ws + (role ? 1 : 0));
                xyzz_lds_load<WG>(p2, lds, T::LANES * (2 * ws + 1) + (role ? 1 : 0));
                T::add(p1, p2, role);
                sz >>= 1;
                if (sz == 1) {
                    T::store(wg_partials + (size_t)T::WORDS * out, p1, role);
                    sz = 0;
                } else {
                    store_lds = true;
                }
            } else {
                sz = 0;
            }
        }
        __syncthreads();
        if (active) {
            if (store_lds) xyzz_lds_store<WG>(lds, tid, p1);
            if (!role) {
                lds_out[ws] = out;
                lds_sz[ws] = sz;
            }
        }
        __syncthreads();
    }
}

}  // namespace posevo
