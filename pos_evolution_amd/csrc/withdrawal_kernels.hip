// withdrawal_kernels.hip -- Capella's withdrawal sweep and BLS-to-execution changes over the resident registry, for gfx950.
// The rules are withdrawals_row.h; the host steps are engine_withdrawals.cpp (pe_process_withdrawals,
// pe_process_bls_to_execution_changes, pe_bls_change_signing_roots).
//
// The sweep: one lane per POSITION j < bound, WD_WG of them per workgroup; position j visits validator (start + j) mod n.
//   k_withdrawals_flag    read-only: what every position yields (WD_NONE / _FULL / _PARTIAL) from the four columns, and per
//                         workgroup the number of hits (wave ballots, summed over the waves in LDS)
//   k_withdrawals_scan    ONE workgroup walks the counts (k_active_scan's and k_block_ops_scan's form): the exclusive offset
//                         of every workgroup and the total
//   k_withdrawals_select  read-only: a hit's rank = its workgroup's offset + the waves before + the lanes before; the hits of
//                         rank < k write their withdrawal record, rank-th of the call's workspace.  Workgroups whose offset
//                         has reached k return at once
//   k_withdrawals_apply   the only writing pass, one lane per record (at most 64): balance -= amount.  bound <= n, so the
//                         records name different validators: one writer per balance, no atomic
// The changes: one lane per change.
//   k_bls_changes_claim   read-only: every check that reads the change and the credentials before the call (SHA-256 of the 48
//                         key bytes among them); a change that passes them all takes its validator's entry of a table by a
//                         MINIMUM over positions
//   k_bls_changes_resolve read-only: the statuses -- a change behind its validator's entry fails the prefix check
//   k_bls_changes_apply   the valid changes write the new credentials: one writer per validator
//   k_bls_change_signing_roots  compute_signing_root of every change
// The selection is a function of the data alone: no order comes from an atomic, no workgroup waits for another (plain
// launches on one stream), no scratch.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave64.h"
#include "withdrawals_row.h"

namespace posevo {

namespace {

constexpr int WD_WAVES = WD_WG / 64;
static_assert(WD_WG % 64 == 0, "whole waves");
static_assert(WD_MAX_PER_PAYLOAD <= 64, "k_withdrawals_apply is one wave");

__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

}  // namespace

__global__ void __launch_bounds__(WD_WG)
k_withdrawals_flag(const WithdrawalsColumns C, const WithdrawalsSweep S, uint8_t* __restrict__ pos_kind, uint32_t* __restrict__ wg_count)
{
    __shared__ uint32_t wave_hits[WD_WAVES];
    const uint32_t j = blockIdx.x * WD_WG + threadIdx.x;
    uint32_t kind = WD_NONE;
    if (j < S.bound) {
        const uint64_t v = withdrawals_validator(S.start, j, S.n);
        kind = withdrawals_kind(C.credentials[8 * v], S.prefix, C.withdrawable[v], C.eff_balance[v], C.balances[v], S.current_epoch,
                                S.max_effective_balance);
        pos_kind[j] = (uint8_t)kind;
    }
    const unsigned long long hits = __ballot(kind != WD_NONE);
    if ((threadIdx.x & 63) == 0) wave_hits[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(hits);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < WD_WAVES; ++w) c += wave_hits[w];
        wg_count[blockIdx.x] = c;
    }
}

// grid: ONE workgroup.  The carry is uniform across it; the loop's trip count depends on n_wg alone.
__global__ void __launch_bounds__(WD_WG)
k_withdrawals_scan(const uint32_t* __restrict__ wg_count, uint32_t n_wg, uint32_t* __restrict__ wg_offset, uint32_t* __restrict__ total)
{
    __shared__ uint32_t wave_total[WD_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t tile = 0; tile < n_wg; tile += WD_WG) {
        const uint32_t i = tile + threadIdx.x;
        const uint32_t c = i < n_wg ? wg_count[i] : 0u;
        const uint32_t incl = wave_incl_scan(c);
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < WD_WAVES; ++w) {
            before += (uint32_t)w < wave ? wave_total[w] : 0u;
            all += wave_total[w];
        }
        if (i < n_wg) wg_offset[i] = before + incl - c;
        carry += all;
        __syncthreads();  // the wave totals are rewritten by the next tile
    }
    if (threadIdx.x == 0) *total = carry;
}

// records: S.k entries of WD_RECORD_WORDS words in the call's workspace
__global__ void __launch_bounds__(WD_WG)
k_withdrawals_select(const WithdrawalsColumns C, const WithdrawalsSweep S, const uint8_t* __restrict__ pos_kind,
                     const uint32_t* __restrict__ wg_offset, uint32_t* __restrict__ records)
{
    __shared__ uint32_t wave_hits[WD_WAVES];
    const uint32_t off = wg_offset[blockIdx.x];
    if (off >= S.k) return;  // uniform over the workgroup: every selected hit lies before it
    const uint32_t j = blockIdx.x * WD_WG + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t kind = j < S.bound ? pos_kind[j] : WD_NONE;
    const unsigned long long hits = __ballot(kind != WD_NONE);
    if (lane == 0) wave_hits[wave] = (uint32_t)__builtin_popcountll(hits);
    __syncthreads();
    uint32_t rank = off;
#pragma unroll
    for (int w = 0; w < WD_WAVES; ++w) rank += (uint32_t)w < wave ? wave_hits[w] : 0u;
    rank += lanes_below(hits);
    if (kind == WD_NONE || rank >= S.k) return;
    const uint64_t v = withdrawals_validator(S.start, j, S.n);
    uint32_t cred[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cred[k] = C.credentials[8 * v + k];
    uint32_t* const r = records + (size_t)WD_RECORD_WORDS * rank;
    withdrawals_record(r, S.next_index + rank, v, cred, withdrawals_amount(kind, C.balances[v], S.max_effective_balance));
    r[WD_WORDS] = kind;
}

// grid: ONE wave; count <= WD_MAX_PER_PAYLOAD.  decrease_balance(validator_index, amount) with amount <= balance
__global__ void __launch_bounds__(64)
k_withdrawals_apply(const uint32_t* __restrict__ records, uint32_t count, uint64_t n, unsigned long long* __restrict__ balances)
{
    const uint32_t i = threadIdx.x;
    if (i >= count) return;
    const uint32_t* const r = records + (size_t)WD_RECORD_WORDS * i;
    const uint64_t v = withdrawals_u64(r + 2), amount = withdrawals_u64(r + 9);
    if (v >= n) return;  // a record is the select pass's: never taken
    const unsigned long long b = balances[v];
    balances[v] = amount > b ? 0 : b - amount;
}

__global__ void __launch_bounds__(WD_WG)
k_bls_changes_claim(const uint32_t* __restrict__ changes, uint32_t n_changes, const uint32_t* __restrict__ credentials, uint64_t n,
                    uint32_t* __restrict__ first, uint32_t* __restrict__ checks)
{
    const uint32_t p = blockIdx.x * WD_WG + threadIdx.x;
    if (p >= n_changes) return;
    uint32_t c[CRED_CHANGE_WORDS], cred[8] = {};
#pragma unroll
    for (int k = 0; k < (int)CRED_CHANGE_WORDS; ++k) c[k] = changes[(size_t)CRED_CHANGE_WORDS * p + k];
    const uint64_t v = bls_change_index(c);
    const bool index_ok = v < n;
    if (index_ok) {
#pragma unroll
        for (int k = 0; k < 8; ++k) cred[k] = credentials[8 * v + k];
    }
    const uint32_t ok = bls_change_checks(c, index_ok, cred);
    checks[p] = ok;
    if (ok == CRED_CHECK_ALL) atomicMin(&first[v], p);
}

__global__ void __launch_bounds__(WD_WG)
k_bls_changes_resolve(const uint32_t* __restrict__ changes, uint32_t n_changes, const uint32_t* __restrict__ checks,
                      const uint32_t* __restrict__ first, uint32_t* __restrict__ status)
{
    const uint32_t p = blockIdx.x * WD_WG + threadIdx.x;
    if (p >= n_changes) return;
    const uint32_t ok = checks[p];
    const bool earlier = (ok & CRED_CHECK_INDEX) && first[bls_change_index(changes + (size_t)CRED_CHANGE_WORDS * p)] < p;
    status[p] = bls_change_status(ok, earlier);
}

__global__ void __launch_bounds__(WD_WG)
k_bls_changes_apply(const uint32_t* __restrict__ changes, uint32_t n_changes, const uint32_t* __restrict__ status, uint64_t n,
                    uint32_t* __restrict__ credentials)
{
    const uint32_t p = blockIdx.x * WD_WG + threadIdx.x;
    if (p >= n_changes || status[p] != CRED_OK) return;
    const uint32_t* const c = changes + (size_t)CRED_CHANGE_WORDS * p;
    const uint64_t v = bls_change_index(c);
    if (v >= n) return;  // a valid change names a validator: never taken
    uint32_t cred[8];
    bls_change_credentials(c, cred);
#pragma unroll
    for (int k = 0; k < 8; ++k) credentials[8 * v + k] = cred[k];
}

struct SigningDomain {
    uint32_t w[8];
};
__global__ void __launch_bounds__(WD_WG)
k_bls_change_signing_roots(const uint32_t* __restrict__ changes, uint32_t n_changes, const SigningDomain domain,
                           uint32_t* __restrict__ roots)
{
    const uint32_t p = blockIdx.x * WD_WG + threadIdx.x;
    if (p >= n_changes) return;
    uint32_t c[CRED_CHANGE_WORDS], out[8];
#pragma unroll
    for (int k = 0; k < (int)CRED_CHANGE_WORDS; ++k) c[k] = changes[(size_t)CRED_CHANGE_WORDS * p + k];
    bls_change_signing_root(c, domain.w, out);
#pragma unroll
    for (int k = 0; k < 8; ++k) roots[8 * (size_t)p + k] = __builtin_bswap32(out[k]);
}

uint32_t withdrawals_workgroups(uint32_t bound) { return (bound + WD_WG - 1) / WD_WG; }

void launch_withdrawals_sweep(hipStream_t s, const WithdrawalsColumns& C, const WithdrawalsSweep& S, uint8_t* d_pos_kind,
                              uint32_t* d_wg_count, uint32_t* d_wg_offset, uint32_t* d_total, uint32_t* d_records)
{
    const uint32_t n_wg = withdrawals_workgroups(S.bound);
    hipLaunchKernelGGL(k_withdrawals_flag, dim3(n_wg), dim3(WD_WG), 0, s, C, S, d_pos_kind, d_wg_count);
    hipLaunchKernelGGL(k_withdrawals_scan, dim3(1), dim3(WD_WG), 0, s, (const uint32_t*)d_wg_count, n_wg, d_wg_offset, d_total);
    hipLaunchKernelGGL(k_withdrawals_select, dim3(n_wg), dim3(WD_WG), 0, s, C, S, (const uint8_t*)d_pos_kind,
                       (const uint32_t*)d_wg_offset, d_records);
}

void launch_withdrawals_apply(hipStream_t s, const uint32_t* d_records, uint32_t count, uint64_t n, uint64_t* d_balances)
{
    if (count == 0) return;
    hipLaunchKernelGGL(k_withdrawals_apply, dim3(1), dim3(64), 0, s, d_records, count, n,
                       reinterpret_cast<unsigned long long*>(d_balances));
}

void launch_bls_changes_resolve(hipStream_t s, const uint32_t* d_changes, uint32_t n_changes, const uint8_t* d_credentials, uint64_t n,
                                uint32_t* d_first, uint32_t* d_checks, uint32_t* d_status)
{
    const dim3 grid((n_changes + WD_WG - 1) / WD_WG);
    hipLaunchKernelGGL(k_bls_changes_claim, grid, dim3(WD_WG), 0, s, d_changes, n_changes,
                       reinterpret_cast<const uint32_t*>(d_credentials), n, d_first, d_checks);
    hipLaunchKernelGGL(k_bls_changes_resolve, grid, dim3(WD_WG), 0, s, d_changes, n_changes, (const uint32_t*)d_checks,
                       (const uint32_t*)d_first, d_status);
}

void launch_bls_changes_apply(hipStream_t s, const uint32_t* d_changes, uint32_t n_changes, const uint32_t* d_status, uint64_t n,
                              uint8_t* d_credentials)
{
    hipLaunchKernelGGL(k_bls_changes_apply, dim3((n_changes + WD_WG - 1) / WD_WG), dim3(WD_WG), 0, s, d_changes, n_changes, d_status,
                       n, reinterpret_cast<uint32_t*>(d_credentials));
}

void launch_bls_change_signing_roots(hipStream_t s, const uint32_t* d_changes, uint32_t n_changes, const uint32_t domain[8],
                                     uint32_t* d_roots)
{
    SigningDomain d;
    for (int k = 0; k < 8; ++k) d.w[k] = domain[k];
    hipLaunchKernelGGL(k_bls_change_signing_roots, dim3((n_changes + WD_WG - 1) / WD_WG), dim3(WD_WG), 0, s, d_changes, n_changes, d,
                       d_roots);
}

}  // namespace posevo
