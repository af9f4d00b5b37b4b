// deposit_kernels.hip -- process_deposit (pe:139-175) over the resident registry, for gfx950.
//   k_deposit_index_build  open-addressing table over 32-byte pubkey leaves: the registry's (kept on the handle, appended
//                          validators inserted incrementally) and, per call, the batch's own over the keys the registry lacks
//   k_deposit_leaves       one lane per deposit: the pubkey's leaf, hash_tree_root(DepositData), the 33-node branch walk and
//                          the comparison with the deposit root; the signing root for pe_deposit_signing_roots
//   k_deposit_probe        a deposit's leaf looked up in the registry's table: a hit compares all 32 bytes
//   k_deposit_resolve      duplicates inside the batch: per new key the first position with a valid signature, every deposit's
//                          status (deposit_row.h) and the new indices by an ordered count -- one workgroup that scans the
//                          batch in tiles with a running carry, as k_registry_scan does over its workgroups' counts
//   k_deposit_apply        64-bit atomic adds onto the resident balances, the appended validators' rows
// What ONE deposit asks is deposit_row.h, shared with the host.  Integer work: 43 hashes per deposit at most, a few table
// probes; no MFMA, no LDS beyond the scan's wave totals.
#include <hip/hip_runtime.h>

#include "deposit_row.h"
#include "kernels.h"

namespace posevo {

namespace {

constexpr int DEPOSIT_WG = 256;

__device__ __forceinline__ bool leaf_equal(const uint32_t* a, const uint32_t* b)
{
    bool same = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) same = same && a[k] == b[k];
    return same;
}

}  // namespace

__global__ void __launch_bounds__(DEPOSIT_WG)
k_deposit_index_build(const uint32_t* __restrict__ leaves, uint64_t first, uint64_t end, const uint32_t* __restrict__ only_if_none,
                      uint32_t* __restrict__ tab, uint32_t mask, uint32_t* __restrict__ out_slot)
{
    const uint64_t v = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= end) return;
    if (only_if_none && only_if_none[v] != NONE32) {
        if (out_slot) out_slot[v] = NONE32;
        return;
    }
    const uint32_t* mine = leaves + 8 * v;
    uint32_t slot = deposit_slot(mine[0], mask);
    uint32_t found = NONE32;
    for (uint32_t probes = 0; probes <= mask; ++probes) {  // bounded: the table keeps empty slots
        const uint32_t cur = atomicCAS(&tab[slot], NONE32, (uint32_t)v);
        if (cur == NONE32) { found = slot; break; }
        // an occupied slot's entries all carry ONE leaf: whichever of them is read, the comparison says the same
        if (leaf_equal(leaves + 8ull * cur, mine)) {
            atomicMin(&tab[slot], (uint32_t)v);
            found = slot;
            break;
        }
        slot = (slot + 1) & mask;
    }
    if (out_slot) out_slot[v] = found;
}

void launch_deposit_index_build(hipStream_t s, const uint32_t* leaves, uint64_t first, uint64_t end, const uint32_t* only_if_none,
                                uint32_t* tab, uint32_t mask, uint32_t* out_slot)
{
    if (end <= first) return;
    const uint64_t n = end - first;
    hipLaunchKernelGGL(k_deposit_index_build, dim3((unsigned)((n + DEPOSIT_WG - 1) / DEPOSIT_WG)), dim3(DEPOSIT_WG), 0, s, leaves,
                       first, end, only_if_none, tab, mask, out_slot);
}

__global__ void __launch_bounds__(DEPOSIT_WG)
k_deposit_leaves(const DepositLeavesArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t* row = a.rows + (size_t)DEPOSIT_ROW_WORDS * i;
    DepositRoots r;
    deposit_roots(row, r);
#pragma unroll
    for (int k = 0; k < 8; ++k) a.leaf[8ull * i + k] = __builtin_bswap32(r.pubkey_leaf[k]);
    if (a.signing_roots) {
        uint32_t sr[8];
        deposit_signing_root(r.message_root, a.domain, sr);
#pragma unroll
        for (int k = 0; k < 8; ++k) a.signing_roots[8ull * i + k] = __builtin_bswap32(sr[k]);
    }
    uint32_t ok = 1;
    if (a.proofs) ok = deposit_branch_ok(r.data_root, a.proofs + (size_t)8 * DEPOSIT_PROOF_NODES * i, a.index0 + i, a.root) ? 1u : 0u;
    a.proof_ok[i] = ok;
}

void launch_deposit_leaves(hipStream_t s, const DepositLeavesArgs& a)
{
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_deposit_leaves, dim3((a.n + DEPOSIT_WG - 1) / DEPOSIT_WG), dim3(DEPOSIT_WG), 0, s, a);
}

__global__ void __launch_bounds__(DEPOSIT_WG)
k_deposit_probe(const uint32_t* __restrict__ dep_leaf, uint32_t n, const uint32_t* __restrict__ reg_leaves,
                const uint32_t* __restrict__ tab, uint32_t mask, uint32_t* __restrict__ reg_index)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* mine = dep_leaf + 8ull * i;
    uint32_t slot = deposit_slot(mine[0], mask);
    uint32_t hit = NONE32;
    for (uint32_t probes = 0; probes <= mask; ++probes) {
        const uint32_t cur = tab[slot];
        if (cur == NONE32) break;
        if (leaf_equal(reg_leaves + 8ull * cur, mine)) { hit = cur; break; }
        slot = (slot + 1) & mask;
    }
    reg_index[i] = hit;
}

void launch_deposit_probe(hipStream_t s, const uint32_t* dep_leaf, uint32_t n, const uint32_t* reg_leaves, const uint32_t* tab,
                          uint32_t mask, uint32_t* reg_index)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_deposit_probe, dim3((n + DEPOSIT_WG - 1) / DEPOSIT_WG), dim3(DEPOSIT_WG), 0, s, dep_leaf, n, reg_leaves, tab,
                       mask, reg_index);
}

// grid: ONE workgroup.  Three passes over the batch in tiles of the workgroup's width; the workgroup meets between them, so
// what a pass wrote to device memory is what the next one reads.
__global__ void __launch_bounds__(DEPOSIT_WG)
k_deposit_resolve(const DepositResolveArgs a)
{
    constexpr int WAVES = DEPOSIT_WG / 64;
    __shared__ uint32_t wave_total[WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // 1. per new key: the first position whose signature verifies
    for (uint32_t i = threadIdx.x; i < a.n; i += DEPOSIT_WG)
        if (a.reg_index[i] == NONE32 && a.key_slot[i] != NONE32 && a.sig_ok[i]) atomicMin(&a.first_valid[a.key_slot[i]], i);
    __threadfence();
    __syncthreads();
    // 2. the creators' ranks in batch order: an exclusive scan with the carry of the tiles before
    uint32_t carry = 0;
    for (uint32_t tile = 0; tile < a.n; tile += DEPOSIT_WG) {
        const uint32_t i = tile + threadIdx.x;
        uint32_t creates = 0;
        if (i < a.n && a.reg_index[i] == NONE32 && a.key_slot[i] != NONE32)
            creates = __hip_atomic_load(&a.first_valid[a.key_slot[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i ? 1u : 0u;
        uint32_t inclusive = creates;
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
        if (i < a.n) a.rank[i] = before + inclusive - creates;
        carry += all;
        __syncthreads();  // wave_total is rewritten by the next tile
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) a.counts[0] = carry;
    // 3. status and the validator credited
    for (uint32_t i = threadIdx.x; i < a.n; i += DEPOSIT_WG) {
        const uint32_t reg = a.reg_index[i];
        uint32_t fv = NONE32;
        if (reg == NONE32 && a.key_slot[i] != NONE32)
            fv = __hip_atomic_load(&a.first_valid[a.key_slot[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int32_t st = deposit_status(a.proof_ok[i] != 0, reg, i, fv);
        uint32_t credited = NONE32;
        if (st == DEPOSIT_TOPUP) credited = reg != NONE32 ? reg : a.n_val + a.rank[fv];
        else if (st == DEPOSIT_APPENDED) credited = a.n_val + a.rank[i];
        a.status[i] = st;
        a.out_index[i] = credited;
    }
}

void launch_deposit_resolve(hipStream_t s, const DepositResolveArgs& a)
{
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_deposit_resolve, dim3(1), dim3(DEPOSIT_WG), 0, s, a);
}

__global__ void __launch_bounds__(DEPOSIT_WG)
k_deposit_apply(const DepositApplyArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int32_t st = a.status[i];
    if (st != DEPOSIT_TOPUP && st != DEPOSIT_APPENDED) return;
    const uint32_t v = a.out_index[i];
    if (v == NONE32) return;
    const uint32_t* row = a.rows + (size_t)DEPOSIT_ROW_WORDS * i;
    const uint64_t amount = deposit_amount(row);
    atomicAdd(reinterpret_cast<unsigned long long*>(a.balances) + v, (unsigned long long)amount);  // increase_balance | balances.append
    if (st != DEPOSIT_APPENDED) return;
    DepositParams P;
    P.effective_balance_increment = a.increment;
    P.max_effective_balance = a.max_effective_balance;
    P.far_future_epoch = a.far_future_epoch;
    const DepositValidator val = deposit_validator(amount, P);
    a.eff_balance[v] = val.effective_balance;
    a.sflags[v] = 0;  // not active in either epoch, not slashed
    a.increments[v] = (uint16_t)val.increments;
    a.activation_eligibility[v] = val.activation_eligibility_epoch;
    a.activation_epoch[v] = val.activation_epoch;
    a.exit_epoch[v] = val.exit_epoch;
    a.withdrawable_epoch[v] = val.withdrawable_epoch;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        a.pubkey_leaf[8ull * v + k] = a.dep_leaf[8ull * i + k];
        a.withdrawal_credentials[8ull * v + k] = row[12 + k];
    }
}

void launch_deposit_apply(hipStream_t s, const DepositApplyArgs& a)
{
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_deposit_apply, dim3((a.n + DEPOSIT_WG - 1) / DEPOSIT_WG), dim3(DEPOSIT_WG), 0, s, a);
}

}  // namespace posevo
