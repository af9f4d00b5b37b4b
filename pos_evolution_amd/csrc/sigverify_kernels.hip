// sigverify_kernels.hip -- the weighted sums of pe_verify_signatures, for gfx950 (host side: engine_sigverify.cpp).
//
//   e(sum_j r_j pk_j, H(m)) * e(-g1, sum_j r_j sig_j) == 1,   r_j secret 64-bit scalars, j over one committee's members
//
//   k_g2_weighted_accumulate  sum_j r_j sig_j per group: the slot layout of k_g2_accumulate (a lane pair per stripe of k members,
//                             128 slots per workgroup, the compacting LDS tree, k_g2_finish behind it)
//   k_g1_weighted_accumulate  sum_j r_j pk_j per group over registry rows: a lane per stripe, 256 slots per workgroup, the same
//                             tree over single lanes, k_g1_finish behind it
//                             (the slot's task and the tree: point_sum_tree.h, one source for these two and k_g2_accumulate)
//   k_sv_mark_identity        a decoded signature at infinity gets its own status (it is no signature)
//   k_sv_rows_g1 / _g2        listed Montgomery rows back to wire bytes: the pairs of the locate pass
//
// A stripe is NOT scaled point by point (64 doublings and up to 64 additions each, k_bls_scale_g2).  One Horner pass over the 64
// bit planes serves the whole stripe:  for b = 63 .. 0:  acc = 2 acc;  acc += P_j for the stripe's j whose r_j has bit b.
// That is 64 doublings per STRIPE (64 / k per point) and 32 additions per point on random scalars.  Lanes of a wave hold different
// scalars, so a per-member `if (bit)` would run for nearly every member in every plane: instead each plane's set members are
// compacted per slot (a k-bit mask per plane, transposed from the scalars into LDS once) and the slot walks its mask; the wave
// then runs max-over-its-slots additions per plane (k = 16: 12.1 of 16 for the 32 slots of a G2 wave, 12.6 for the 64 of a G1
// wave, against a mean of 8: tests/verify_signatures_model.py wave_max_adds).
// The point forms are the complete ones of g1.h / g2.h: acc = 2 acc followed by + P meets acc = +-P on structured keys.
#include "g2.h"
#include "kernels.h"
#include "point_sum_tree.h"

namespace posevo {

namespace {

constexpr int SV_WG = 256;
constexpr int SV_PLANES = 64;

// The stripe's scalars, transposed: bit j of masks[b * n_slots_wg + ws] = bit b of the scalar of the stripe's member j.
// `planes` = [lo, hi): the planes this lane writes (the two lanes of a G2 pair take half each).
__device__ __forceinline__ void sv_plane_masks(uint16_t* masks, int wg_slots, int ws, const uint64_t* __restrict__ scalars,
                                               const slot_task& t, int lo, int hi)
{
    for (int b = lo; b < hi; ++b) masks[b * wg_slots + ws] = 0;
    for (uint32_t j = 0; j < t.count; ++j) {
        const uint64_t r = scalars[t.member0 + j];
        for (int b = lo; b < hi; ++b) masks[b * wg_slots + ws] |= (uint16_t)(((r >> b) & 1) << j);
    }
}

}  // namespace

// ---------------------------------------------------------------- sum_j r_j sig_j
// pts: the decoded signatures (48 Montgomery words a row, the (0, 0) row = infinity = left out); member m's row is index[m] (or m),
// its scalar scalars[m].  wg_partials: as k_g2_accumulate's.
// (two waves per SIMD: 252 registers, no scratch -- the accumulator is the only point that lives across the doubling)
__global__ void __launch_bounds__(SV_WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_g2_weighted_accumulate(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ index, const uint64_t* __restrict__ scalars,
                         const G1Group* __restrict__ groups, uint32_t n_groups, uint32_t n_slots, uint32_t* __restrict__ wg_partials)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[48 * SV_WG];  // the plane masks, then the tree's staging
    __shared__ uint32_t lds_out[G2_WG_SLOTS];
    __shared__ uint32_t lds_sz[G2_WG_SLOTS];
    uint16_t* masks = reinterpret_cast<uint16_t*>(lds);

    const int tid = threadIdx.x;
    const bool role = tid & 1;
    const int ws = tid >> 1;
    const slot_task t = slot_task_of(groups, n_groups, n_slots, blockIdx.x * G2_WG_SLOTS + ws, G2_WG_SLOTS);
    sv_plane_masks(masks, G2_WG_SLOTS, ws, scalars, t, role ? 32 : 0, role ? 64 : 32);
    __syncthreads();

    g2x acc;
    g2x_set_inf(acc);
#pragma unroll 1
    for (int b = SV_PLANES - 1; b >= 0; --b) {
        acc = g2x_double(acc, role);
        uint32_t m = masks[b * G2_WG_SLOTS + ws];  // the same word in both lanes of the pair: they walk it together
#pragma unroll 1
        while (m) {
            const uint32_t member = t.member0 + (uint32_t)__builtin_ctz(m);
            m &= m - 1;
            const uint32_t row = index ? index[member] : member;
            const uint32_t* p = pts + 48ull * row + (role ? 12 : 0);
            fp qx, qy;
            fp_vec16::ld(qx, p);
            fp_vec16::ld(qy, p + 24);
            const bool q_inf = pair_and(fp_is_zero(qx) && fp_is_zero(qy));
            g2x_add_affine(acc, qx, qy, q_inf, role);
        }
    }
    __syncthreads();  // the masks are done with: the same LDS now stages the tree

    point_sum_tree<sum_g2, SV_WG>(lds, lds_out, lds_sz, acc, t.out, t.size, wg_partials);
}

// ---------------------------------------------------------------- sum_j r_j pk_j
// pts: the registry (G1_ROW_WORDS words a row: x | y in Montgomery form, (0, 0) = infinity); member m's row is signer[m].
// wg_partials: one 48-word XYZZ partial per (group, workgroup), as k_g1_tree writes them for k_g1_finish.
__global__ void __launch_bounds__(SV_WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_g1_weighted_accumulate(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ signer, const uint64_t* __restrict__ scalars,
                         const G1Group* __restrict__ groups, uint32_t n_groups, uint32_t n_slots, uint32_t* __restrict__ wg_partials)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[48 * SV_WG];
    __shared__ uint32_t lds_out[SV_WG];
    __shared__ uint32_t lds_sz[SV_WG];
    uint16_t* masks = reinterpret_cast<uint16_t*>(lds);

    const int ws = threadIdx.x;
    const slot_task t = slot_task_of(groups, n_groups, n_slots, blockIdx.x * SV_WG + ws, SV_WG);
    sv_plane_masks(masks, SV_WG, ws, scalars, t, 0, SV_PLANES);
    __syncthreads();

    g1x acc;
    g1x_set_inf(acc);
#pragma unroll 1
    for (int b = SV_PLANES - 1; b >= 0; --b) {
        acc = g1x_double(acc);
        uint32_t m = masks[b * SV_WG + ws];
#pragma unroll 1
        while (m) {
            const uint32_t member = t.member0 + (uint32_t)__builtin_ctz(m);
            m &= m - 1;
            const uint32_t* p = pts + (uint64_t)G1_ROW_WORDS * signer[member];
            fp qx, qy;
            fp_vec16::ld(qx, p);
            fp_vec16::ld(qy, p + 12);
            g1x_add_affine(acc, qx, qy, fp_is_zero(qx) && fp_is_zero(qy));
        }
    }
    __syncthreads();

    point_sum_tree<sum_g1, SV_WG>(lds, lds_out, lds_sz, acc, t.out, t.size, wg_partials);
}

// ---------------------------------------------------------------- the identity, and rows back to wire bytes
// k_g2_decompress accepts the encoding of infinity (status 0, the (0, 0) row).  It is no BLSSignature: status `code`.
__global__ void __launch_bounds__(256)
k_sv_mark_identity(const uint32_t* __restrict__ pts, uint64_t n, int32_t* __restrict__ status, int32_t code)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || status[i] != 0) return;
    const uint4* p = reinterpret_cast<const uint4*>(pts + 48ull * i);
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const uint4 v = p[j];
        any |= v.x | v.y | v.z | v.w;
    }
    if (!any) status[i] = code;
}

// out[t] = row rows[t] of the registry as 96 wire bytes (x | y), infinity as the 0x40 flag
__global__ void __launch_bounds__(256)
k_sv_rows_g1(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ rows, uint32_t n, uint8_t* __restrict__ out_be96)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const uint32_t* p = pts + (uint64_t)G1_ROW_WORDS * rows[t];
    fp x, y, px, py;
    fp_vec16::ld(x, p);
    fp_vec16::ld(y, p + 12);
    const bool inf = fp_is_zero(x) && fp_is_zero(y);
    fp_from_mont(px, x);
    fp_from_mont(py, y);
    uint8_t* o = out_be96 + 96ull * t;
    fp_store_be48(o, px);
    fp_store_be48(o + 48, py);
    if (inf) o[0] = 0x40;
}
// out[t] = row rows[t] of the decoded signatures as 192 wire bytes (x.c1 | x.c0 | y.c1 | y.c0)
__global__ void __launch_bounds__(256)
k_sv_rows_g2(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ rows, uint32_t n, uint8_t* __restrict__ out_be192)
{
    const uint32_t gid = blockIdx.x * 256 + threadIdx.x;  // a lane per Fp element
    const uint32_t t = gid >> 2, e = gid & 3;             // stored element: 0 x0, 1 x1, 2 y0, 3 y1
    if (t >= n) return;
    const uint32_t* p = pts + 48ull * rows[t];
    uint32_t any = 0;
    for (int j = 0; j < 48; ++j) any |= p[j];
    fp v, pv;
    fp_vec16::ld(v, p + 12 * e);
    fp_from_mont(pv, v);
    uint8_t* o = out_be192 + 192ull * t;
    fp_store_be48(o + 48 * ((e & 2) | ((e & 1) ^ 1)), pv);
    if (!any && e == 1) o[0] = 0x40;
}

// ---------------------------------------------------------------- launchers
void launch_g2_weighted_accumulate(hipStream_t s, const uint32_t* points_mont48, const uint32_t* index, const uint64_t* scalars,
                                   const G1Group* groups, uint32_t n_groups, uint32_t n_slots, uint32_t* wg_partials96)
{
    if (n_groups == 0 || n_slots == 0) return;
    hipLaunchKernelGGL(k_g2_weighted_accumulate, dim3((n_slots + G2_WG_SLOTS - 1) / G2_WG_SLOTS), dim3(SV_WG), 0, s, points_mont48,
                       index, scalars, groups, n_groups, n_slots, wg_partials96);
}
void launch_g1_weighted_accumulate(hipStream_t s, const uint32_t* points_mont, const uint32_t* signer, const uint64_t* scalars,
                                   const G1Group* groups, uint32_t n_groups, uint32_t n_slots, uint32_t* wg_partials48)
{
    if (n_groups == 0 || n_slots == 0) return;
    hipLaunchKernelGGL(k_g1_weighted_accumulate, dim3((n_slots + SV_WG - 1) / SV_WG), dim3(SV_WG), 0, s, points_mont, signer, scalars,
                       groups, n_groups, n_slots, wg_partials48);
}
void launch_sv_mark_identity(hipStream_t s, const uint32_t* points_mont48, uint64_t n, int32_t* status, int32_t code)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_sv_mark_identity, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, points_mont48, n, status, code);
}
void launch_sv_rows_g1(hipStream_t s, const uint32_t* points_mont, const uint32_t* rows, uint32_t n, uint8_t* out_be96)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_sv_rows_g1, dim3((n + 255) / 256), dim3(256), 0, s, points_mont, rows, n, out_be96);
}
void launch_sv_rows_g2(hipStream_t s, const uint32_t* points_mont48, const uint32_t* rows, uint32_t n, uint8_t* out_be192)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_sv_rows_g2, dim3((unsigned)((4ull * n + 255) / 256)), dim3(256), 0, s, points_mont48, rows, n, out_be192);
}

}  // namespace posevo
