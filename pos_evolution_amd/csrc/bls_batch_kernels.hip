// bls_batch_kernels.hip -- batch verification of BLS aggregates by random linear combination, for gfx950.
//
//   prod_i e(r_i pk_i, H(m_i)) * e(-g1, sum_i r_i sig_i) == 1,   r_i secret 64-bit scalars
//
// Only the message pairs still pay a Miller loop each; the signatures of a chunk collapse into one pair and the whole call
// into one final exponentiation (the unchanged k_bls_miller / k_bls_final_exp of bls_kernels.hip; host side: engine_batch.cpp).
//
//   k_bls_batch_settle  a lane pair per group: wire bytes -> Montgomery form, the three curve equations, the identity flags.
//                       What it settles never enters the batch (k_g2_subgroup_check then settles the signatures outside G2).
//   k_bls_scale_g1      a lane per live group: r pk, 64-bit left-to-right double-and-add, one inversion, written as the
//                       group's row of the Miller workspace (Q = T = H(m), P = r pk)
//   k_bls_scale_g2      a lane pair per live group: r sig as an XYZZ point
//   k_bls_chunk_sig     a lane pair per chunk: the sum of the chunk's r sig, affine, as the chunk's last row (P = -g1)
//   k_bls_gt_product    a 16-lane row per output: the product of up to BLS_BATCH_FAN Fp12 values (one level of the tree)
//
// Shared with bls_kernels.hip: the wire decoders (wire_points.h), the workspace row's layout (kernels.h), f12_one_coeff (fp12.h),
// the dword movers (fp_mem.h: these rows are written and read word by word).
// The point formulas are the complete ones of g1.h / g2.h (infinity, P = Q, P = -Q): the inputs are curve points, not
// necessarily subgroup points, and r P may meet P again or infinity on a point of small order.
#include "fp12.h"
#include "fp_mem.h"
#include "fp_sqrt.h"
#include "kernels.h"
#include "wire_points.h"

namespace posevo {

// ---------------------------------------------------------------- settle
// status[g]: BLS_BATCH_LIVE stays a candidate, BLS_BATCH_IDENTITY an identity key, message point or signature (verdict 0),
// BLS_BATCH_BAD a point off its curve (verdict 2, whatever else holds: pe_fast_aggregate_verify's order)
__global__ void __launch_bounds__(256) k_bls_batch_settle(const uint8_t* __restrict__ pk96, const uint8_t* __restrict__ msg192,
                                                           const uint8_t* __restrict__ sig192, uint32_t n_groups,
                                                           uint32_t* __restrict__ pk_mont24, uint32_t* __restrict__ msg_mont48,
                                                           uint32_t* __restrict__ sig_mont48, int32_t* __restrict__ status)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t g = gid >> 1;
    if (g >= n_groups) return;  // whole lane pairs leave together
    const bool role = (gid & 1) != 0;
    fp px, py, mx, my, sx, sy;
    bool p_inf, m_inf, s_inf;
    bool bad = wire_load_g1(px, py, p_inf, pk96 + (size_t)96 * g);
    bad |= wire_load_g2(mx, my, m_inf, msg192 + (size_t)192 * g, role);
    bad |= wire_load_g2(sx, sy, s_inf, sig192 + (size_t)192 * g, role);
    fp_words::st(pk_mont24 + (size_t)24 * g + 12 * (int)role, role ? py : px);
    fp_words::st(msg_mont48 + (size_t)48 * g + 12 * (int)role, mx);
    fp_words::st(msg_mont48 + (size_t)48 * g + 12 * (2 + (int)role), my);
    fp_words::st(sig_mont48 + (size_t)48 * g + 12 * (int)role, sx);
    fp_words::st(sig_mont48 + (size_t)48 * g + 12 * (2 + (int)role), sy);
    if (!role) status[g] = bad ? BLS_BATCH_BAD : (p_inf || m_inf || s_inf) ? BLS_BATCH_IDENTITY : BLS_BATCH_LIVE;
}

// ---------------------------------------------------------------- r pk
// Live group i (group live[i] of the call) becomes row (i / c) (c + 1) + i % c of the workspace: a chunk is c message pairs
// and the signature pair k_bls_chunk_sig writes behind them.
__global__ void __launch_bounds__(64) k_bls_scale_g1(const uint32_t* __restrict__ live, uint32_t n_live, uint32_t chunk,
                                                      const uint64_t* __restrict__ scalars, const uint32_t* __restrict__ pk_mont24,
                                                      const uint32_t* __restrict__ msg_mont48, uint32_t* __restrict__ ws,
                                                      int32_t* __restrict__ pair_flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_live) return;
    const uint32_t g = live[i];
    const uint64_t r = scalars[g];
    fp px, py;
    fp_words::ld(px, pk_mont24 + (size_t)24 * g);
    fp_words::ld(py, pk_mont24 + (size_t)24 * g + 12);
    g1x acc;
    g1x_set_inf(acc);
#pragma unroll 1
    for (int bit = 63; bit >= 0; --bit) {
        acc = g1x_double(acc);
        if ((r >> bit) & 1) g1x_add_affine(acc, px, py, false);
    }
    // affine, Montgomery: 1 / ZZ = ZZZ / (ZZ ZZZ), 1 / ZZZ = ZZ / (ZZ ZZZ); infinity (a key of small order) gives zeros
    const bool inf = g1x_is_inf(acc);
    fp t, inv, x, y;
    fp_mul(t, acc.zz, acc.zzz);
    fp_inv_inline(inv, t);
    fp_mul(t, inv, acc.zzz);
    fp_mul(x, acc.x, t);
    fp_mul(t, inv, acc.zz);
    fp_mul(y, acc.y, t);
    const uint32_t row_idx = (i / chunk) * (chunk + 1) + i % chunk;
    uint32_t* row = ws + (size_t)BLS_PAIR_WORDS * row_idx;
    const uint32_t* q = msg_mont48 + (size_t)48 * g;
#pragma unroll 1
    for (int j = 0; j < 48; ++j) {
        const uint32_t w = q[j];
        row[j] = w;                  // Q
        row[12 * BLS_WS_T + j] = w;  // T = (Q.x, Q.y, 1)
    }
    fp_words::st(row + 12 * BLS_WS_P, x);
    fp_words::st(row + 12 * (BLS_WS_P + 1), y);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        row[12 * (BLS_WS_T + 4) + j] = fp_r1_limb(j);
        row[12 * (BLS_WS_T + 5) + j] = 0;
    }
    pair_flag[row_idx] = inf ? BLS_PAIR_SKIP : BLS_PAIR_LIVE;
}

// ---------------------------------------------------------------- r sig
// The scalar is the point's own, so the addition is data-dependent: it is taken under a BRANCH, not computed and selected.  The
// two lanes of a pair share the scalar and take the branch together (the exchanges inside stay defined); across the wave the
// body runs once per bit when any pair has the bit set and not at all otherwise -- never more than the select form, which runs
// it for every bit and keeps a second XYZZ point (96 registers) alive across it.
// (one wave per SIMD: at two the doubling with the branch's live values around it spilled 56 bytes per lane)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_bls_scale_g2(const uint32_t* __restrict__ live, uint32_t n_live, const uint64_t* __restrict__ scalars,
               const uint32_t* __restrict__ sig_mont48, uint32_t* __restrict__ scaled96)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = gid >> 1;
    if (i >= n_live) return;
    const bool role = (gid & 1) != 0;
    const uint32_t g = live[i];
    const uint64_t r = scalars[g];
    fp qx, qy;
    fp_words::ld(qx, sig_mont48 + (size_t)48 * g + (role ? 12 : 0));
    fp_words::ld(qy, sig_mont48 + (size_t)48 * g + 24 + (role ? 12 : 0));
    g2x acc;
    g2x_set_inf(acc);
#pragma unroll 1
    for (int bit = 63; bit >= 0; --bit) {
        acc = g2x_double(acc, role);
        if ((r >> bit) & 1) g2x_add_affine(acc, qx, qy, false, role);
    }
    g2x_st<fp_words>(scaled96 + (size_t)G2X_WORDS * i, acc, role);
}

// The chunk's signature pair: Q = T = the sum of its scaled signatures, P = -g1 (wire bytes, converted here).  A sum at
// infinity contributes 1, as it must: the message pairs alone then have to multiply to 1.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_bls_chunk_sig(const uint32_t* __restrict__ scaled96, uint32_t n_live, uint32_t chunk, uint32_t n_chunks,
                const uint8_t* __restrict__ neg_g1_be96, uint32_t* __restrict__ ws, int32_t* __restrict__ pair_flag)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = gid >> 1;
    if (j >= n_chunks) return;
    const bool role = (gid & 1) != 0;
    const uint32_t first = j * chunk;
    const uint32_t cnt = min(chunk, n_live - first);
    g2x acc;
    g2x_set_inf(acc);
#pragma unroll 1
    for (uint32_t t = 0; t < cnt; ++t) {
        g2x p;
        g2x_ld<fp_words>(p, scaled96 + (size_t)G2X_WORDS * (first + t), role);
        g2x_add(acc, p, role);
    }
    const bool inf = g2x_is_inf(acc);
    fp t, inv, x, y, one, pc, pm;
    f2_mul(t, acc.zz, acc.zzz, role);
    f2_inv(inv, t, role);
    f2_mul(t, inv, acc.zzz, role);
    f2_mul(x, acc.x, t, role);
    f2_mul(t, inv, acc.zz, role);
    f2_mul(y, acc.y, t, role);
    f2_set_one(one, role);
    fp_load_be48(pc, neg_g1_be96 + (role ? 48 : 0));  // the leading bytes of -g1 carry no flag bits
    fp_to_mont(pm, pc);
    const uint32_t row_idx = j * (chunk + 1) + cnt;
    uint32_t* row = ws + (size_t)BLS_PAIR_WORDS * row_idx;  // (k_bls_prepare's six stores: see the comment there)
    fp_words::st(row + 12 * (0 + (int)role), x);
    fp_words::st(row + 12 * (2 + (int)role), y);
    fp_words::st(row + 12 * (BLS_WS_P + (int)role), pm);
    fp_words::st(row + 12 * (BLS_WS_T + 0 + (int)role), x);
    fp_words::st(row + 12 * (BLS_WS_T + 2 + (int)role), y);
    fp_words::st(row + 12 * (BLS_WS_T + 4 + (int)role), one);
    if (!role) pair_flag[row_idx] = inf ? BLS_PAIR_SKIP : BLS_PAIR_LIVE;
}

// ---------------------------------------------------------------- the product of the chunk values
// One level of the tree: out[o] = in[o F] ... in[o F + F - 1] (what lies past n_in is 1).  Two slots of the LDS slot file per
// wave (6 KB): the running product and the next factor; a lane holds a handful of fp values, as everywhere in fp12.h.
__global__ void __launch_bounds__(64) k_bls_gt_product(const uint32_t* __restrict__ in, uint32_t n_in, uint32_t* __restrict__ out,
                                                        uint32_t n_out)
{
    __shared__ uint32_t lds[2 * 12 * 64];
    const bls_lane c = bls_lane_init(lds);
    const uint32_t o = blockIdx.x * BLS_GROUPS_PER_WAVE + (uint32_t)(c.lane >> 4);
    const bool valid = o < n_out;
#pragma unroll 1
    for (uint32_t t = 0; t < BLS_BATCH_FAN; ++t) {
        const uint64_t idx = (uint64_t)o * BLS_BATCH_FAN + t;
        fp a;
        f12_one_coeff(a, c);
        if (valid && c.act && idx < n_in) fp_words::ld(a, in + (size_t)BLS_GT_WORDS * idx + 12 * (2 * c.k + (int)c.role));
        if (c.act) slot_st(lds, t == 0 ? 0 : 1, c.lane, a);
        if (t == 0) continue;
        fp r;
        __syncthreads();
        f12_mul(r, c, 0, 1);
        __syncthreads();
        if (c.act) slot_st(lds, 0, c.lane, r);
    }
    __syncthreads();
    if (!valid || !c.act) return;
    fp r;
    slot_ld(r, lds, 0, c.lane);
    fp_words::st(out + (size_t)BLS_GT_WORDS * o + 12 * (2 * c.k + (int)c.role), r);
}

// ---------------------------------------------------------------- launchers
void launch_bls_batch_settle(hipStream_t s, const uint8_t* pk96, const uint8_t* msg192, const uint8_t* sig192, uint32_t n_groups,
                             uint32_t* pk_mont24, uint32_t* msg_mont48, uint32_t* sig_mont48, int32_t* status)
{
    if (n_groups == 0) return;
    hipLaunchKernelGGL(k_bls_batch_settle, dim3((unsigned)((2 * (uint64_t)n_groups + 255) / 256)), dim3(256), 0, s, pk96, msg192,
                       sig192, n_groups, pk_mont24, msg_mont48, sig_mont48, status);
}
void launch_bls_scale_g1(hipStream_t s, const uint32_t* live, uint32_t n_live, uint32_t chunk, const uint64_t* scalars,
                         const uint32_t* pk_mont24, const uint32_t* msg_mont48, uint32_t* ws, int32_t* pair_flag)
{
    if (n_live == 0) return;
    hipLaunchKernelGGL(k_bls_scale_g1, dim3((n_live + 63) / 64), dim3(64), 0, s, live, n_live, chunk, scalars, pk_mont24,
                       msg_mont48, ws, pair_flag);
}
void launch_bls_scale_g2(hipStream_t s, const uint32_t* live, uint32_t n_live, const uint64_t* scalars, const uint32_t* sig_mont48,
                         uint32_t* scaled96)
{
    if (n_live == 0) return;
    hipLaunchKernelGGL(k_bls_scale_g2, dim3((unsigned)((2 * (uint64_t)n_live + 63) / 64)), dim3(64), 0, s, live, n_live, scalars,
                       sig_mont48, scaled96);
}
void launch_bls_chunk_sig(hipStream_t s, const uint32_t* scaled96, uint32_t n_live, uint32_t chunk, uint32_t n_chunks,
                          const uint8_t* neg_g1_be96, uint32_t* ws, int32_t* pair_flag)
{
    if (n_chunks == 0) return;
    hipLaunchKernelGGL(k_bls_chunk_sig, dim3((2 * n_chunks + 63) / 64), dim3(64), 0, s, scaled96, n_live, chunk, n_chunks,
                       neg_g1_be96, ws, pair_flag);
}
void launch_bls_gt_product(hipStream_t s, const uint32_t* in, uint32_t n_in, uint32_t* out, uint32_t n_out)
{
    if (n_out == 0) return;
    hipLaunchKernelGGL(k_bls_gt_product, dim3((n_out + BLS_GROUPS_PER_WAVE - 1) / BLS_GROUPS_PER_WAVE), dim3(64), 0, s, in, n_in,
                       out, n_out);
}

}  // namespace posevo
