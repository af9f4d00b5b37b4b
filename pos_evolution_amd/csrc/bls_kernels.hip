// bls_kernels.hip -- the pairing-product check e(P_1, Q_1) ... e(P_n, Q_n) == 1 per group, for gfx950.
//
// The step is_valid_indexed_attestation ends with (pe:736, 976, 1456): FastAggregateVerify's e(pk_agg, H(m)) == e(g1, sig),
// as the product e(pk_agg, H(m)) e(-g1, sig) == 1.
//
//   k_bls_prepare    a lane pair per (P, Q): wire bytes -> Montgomery form, both curve equations checked, T = Q (the decode is
//                    wire_points.h's, kept written out here; the workspace row: BLS_WS_* / BLS_PAIR_* of kernels.h)
//   k_bls_miller     a 16-lane row per group (fp12.h: lane pair k = coefficient k): the optimal-ate Miller loop over
//                    |z| = 0xd201000000010000, 63 doublings and 5 additions, ONE accumulator f per group: every pair of the
//                    group contributes its lines to it, so a group pays the 63 Fp12 squarings once; conjugated at the end (z < 0)
//   k_bls_final_exp  a row per group: f^((p^12 - 1) / r * 3) -- easy part (p^6 - 1)(p^2 + 1), hard part by
//                    3 (p^4 - p^2 + 1) / r = (z - 1)^2 (z + p)(z^2 + p^2 - 1) + 3 with cyclotomic squarings -- compared with 1
//
// The final power is c = 3 times the reduced pairing's; gcd(3, r) = 1, so the verdict is the same.
//
// The point steps of the Miller loop and the whole final exponentiation are OP TABLES (bls_consts.inc, generated from
// tests/pairing_model.py, which runs the same tables): each kernel is a loop around one switch, so every field operation is
// inlined exactly once per kernel (an Fp product is ~5 KB of code; written out, the 369 Fp12 operations of the final exponentiation
// would be megabytes) and there is no call that could keep state in scratch.  Operands live in the LDS slot file of fp12.h.
//
// In the Miller loop lane pair k of a row works the point steps of the group's pairs k, k + 6, ... (T in device memory between
// steps, Q and P read where needed), then all six lane pairs multiply f by each line in turn.
#include "fp12.h"
#include "fp_mem.h"
#include "fp_sqrt.h"
#include "kernels.h"
#include "wire_points.h"

namespace posevo {

#include "bls_consts.inc"

enum { BLS_OP_MUL = 0, BLS_OP_SQR, BLS_OP_ADD, BLS_OP_SUB, BLS_OP_NEG, BLS_OP_MULFP, BLS_OP_LD };
enum { BLS_FE_MUL = 0, BLS_FE_CSQR, BLS_FE_CONJ, BLS_FE_FROB, BLS_FE_INVSCALE };
static_assert(BLS_SLOT_L2 == BLS_SLOT_L0 + 1 && BLS_SLOT_L3 == BLS_SLOT_L0 + 2, "the line's slots are consecutive");

// ---------------------------------------------------------------- prepare
__global__ void __launch_bounds__(256) k_bls_prepare(const uint8_t* __restrict__ g1_be96, const uint8_t* __restrict__ g2_be192,
                                                      uint64_t n_pairs, uint32_t* __restrict__ ws, int32_t* __restrict__ pair_flag)
{
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t pair = gid >> 1;
    if (pair >= n_pairs) return;  // n_pairs counts whole lane pairs: both lanes leave together
    const bool role = (gid & 1) != 0;
    // (wire_load_g1 / wire_load_g2 of wire_points.h, open-coded around ONE Montgomery 4: through them 155 -> 154 or 156 VGPRs)
    const uint8_t* a = g1_be96 + 96 * pair;
    const uint8_t* b = g2_be192 + 192 * pair;
    const bool p_inf = (a[0] & 0x40) != 0, q_inf = (b[0] & 0x40) != 0;
    bool bad = false;
    fp four, px, py, qx, qy;
    fp_set_small_mont(four, 4);
    fp_set_zero(px); fp_set_zero(py); fp_set_zero(qx); fp_set_zero(qy);
    if (!p_inf) {  // y^2 = x^3 + 4 (both lanes compute it)
        fp x, y, t, u;
        fp_load_be48(x, a);
        fp_load_be48(y, a + 48);
        y.l[11] = __builtin_bswap32(reinterpret_cast<const uint32_t*>(a + 48)[0]);  // only the leading byte has flags
        bad |= (a[0] & 0x80) != 0 || !fp_is_canonical(x) || !fp_is_canonical(y);
        fp_to_mont(px, x);
        fp_to_mont(py, y);
        fp_sqr(t, px);
        fp_mul(t, t, px);
        fp_add(t, t, four);
        fp_sqr(u, py);
        bad |= !fp_eq(t, u);
    }
    if (!q_inf) {  // y^2 = x^3 + 4 (1 + u); wire order c1 first
        fp x, y, t, u;
        const uint8_t* xs = b + (role ? 0 : 48);
        const uint8_t* ys = b + 96 + (role ? 0 : 48);
        fp_load_be48(x, xs);
        if (!role) x.l[11] = __builtin_bswap32(reinterpret_cast<const uint32_t*>(xs)[0]);
        fp_load_be48(y, ys);
        y.l[11] = __builtin_bswap32(reinterpret_cast<const uint32_t*>(ys)[0]);
        bad |= (b[0] & 0x80) != 0 || !fp_is_canonical(x) || !fp_is_canonical(y);
        fp_to_mont(qx, x);
        fp_to_mont(qy, y);
        f2_sqr(t, qx, role);
        f2_mul(t, t, qx, role);
        fp_add(t, t, four);
        f2_sqr(u, qy, role);
        bad |= !fp_eq(t, u);
    }
    bad = !pair_and(!bad);
    uint32_t* row = ws + (uint64_t)BLS_PAIR_WORDS * pair;
    fp one;
    f2_set_one(one, role);
    // (the same six stores as k_bls_chunk_sig's: as one shared function they changed the registers of both kernels)
    fp_words::st(row + 12 * (0 + (int)role), qx);
    fp_words::st(row + 12 * (2 + (int)role), qy);
    fp_words::st(row + 12 * (BLS_WS_P + (int)role), role ? py : px);
    fp_words::st(row + 12 * (BLS_WS_T + 0 + (int)role), qx);
    fp_words::st(row + 12 * (BLS_WS_T + 2 + (int)role), qy);
    fp_words::st(row + 12 * (BLS_WS_T + 4 + (int)role), one);
    if (!role) pair_flag[pair] = bad ? BLS_PAIR_BAD : (p_inf || q_inf) ? BLS_PAIR_SKIP : BLS_PAIR_LIVE;
}

// ---------------------------------------------------------------- Miller loop
// One step (doubling or addition) of every pair of the wave's four groups: the point programs, then the line products.
__device__ __forceinline__ void bls_miller_step(const bls_lane& c, const uint32_t* __restrict__ prog, int prog_len,
                                                uint32_t* __restrict__ ws, const int32_t* __restrict__ pair_flag, uint32_t start,
                                                uint32_t n, uint32_t max_n)
{
#pragma unroll 1
    for (uint32_t done = 0; done < max_n; done += 6) {
        const uint32_t idx = done + (uint32_t)c.k;
        const bool has = c.act && idx < n;
        const uint64_t pidx = has ? (uint64_t)start + idx : 0;  // lanes without a pair compute on pair 0 and keep nothing
        const bool live = has && pair_flag[pidx] == BLS_PAIR_LIVE;
        uint32_t* row = ws + (uint64_t)BLS_PAIR_WORDS * pidx;
        {
            fp t;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                fp_words::ld(t, row + 12 * (BLS_WS_T + 2 * s + (int)c.role));
                slot_st(c.lds, s, c.lane, t);
            }
        }
#pragma unroll 1
        for (int pc = 0; pc < prog_len; ++pc) {
            const uint32_t w = prog[pc];
            const int op = (int)(w & 255), d = (int)(w >> 8 & 255), sa = (int)(w >> 16 & 255), sb = (int)(w >> 24);
            fp x, y, r;
            if (op == BLS_OP_LD) {
                fp_words::ld(r, row + 12 * (sa < 2 ? 2 * sa + (int)c.role : BLS_WS_P + sa - 2));
            } else {
                slot_ld(x, c.lds, sa, c.lane);
                slot_ld(y, c.lds, op == BLS_OP_SQR || op == BLS_OP_NEG ? sa : sb, c.lane);
                switch (op) {
                case BLS_OP_MUL: f2_mul(r, x, y, c.role); break;
                case BLS_OP_SQR: f2_sqr(r, x, c.role); break;
                case BLS_OP_ADD: fp_add(r, x, y); break;
                case BLS_OP_SUB: fp_sub(r, x, y); break;
                case BLS_OP_NEG: fp_neg(r, x); break;
                default: fp_mul(r, x, y); break;  // BLS_OP_MULFP: an Fp factor, the same in both lanes
                }
            }
            slot_st(c.lds, d, c.lane, r);
        }
        if (live) {
            fp t;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                slot_ld(t, c.lds, s, c.lane);
                fp_words::st(row + 12 * (BLS_WS_T + 2 * s + (int)c.role), t);
            }
        } else if (c.act) {  // no pair, infinity on a side or a bad point: the line is 1
            fp one, zero;
            f2_set_one(one, c.role);
            fp_set_zero(zero);
            slot_st(c.lds, BLS_SLOT_L0, c.lane, one);
            slot_st(c.lds, BLS_SLOT_L2, c.lane, zero);
            slot_st(c.lds, BLS_SLOT_L3, c.lane, zero);
        }
        const int cnt = (int)(max_n - done < 6 ? max_n - done : 6);
#pragma unroll 1
        for (int i = 0; i < cnt; ++i) {
            fp r;
            __syncthreads();
            f12_mul_line(r, c, BLS_SLOT_F, BLS_SLOT_L0, i);
            __syncthreads();
            if (c.act) slot_st(c.lds, BLS_SLOT_F, c.lane, r);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) k_bls_miller(uint32_t* __restrict__ ws, const int32_t* __restrict__ pair_flag,
                                                    const uint32_t* __restrict__ offsets, uint32_t n_groups,
                                                    uint32_t* __restrict__ gt, int32_t* __restrict__ group_bad)
{
    __shared__ uint32_t lds[BLS_N_SLOTS * 12 * 64];
    const bls_lane c = bls_lane_init(lds);
    const uint32_t g = blockIdx.x * BLS_GROUPS_PER_WAVE + (uint32_t)(c.lane >> 4);
    const bool gvalid = g < n_groups;
    const uint32_t start = gvalid ? offsets[g] : 0;
    const uint32_t n = gvalid ? offsets[g + 1] - start : 0;
    uint32_t max_n = n;
    max_n = max(max_n, (uint32_t)__shfl_xor((int)max_n, 16, 64));
    max_n = max(max_n, (uint32_t)__shfl_xor((int)max_n, 32, 64));
    max_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)max_n);
    {
        fp one;
        f12_one_coeff(one, c);
        if (c.act) slot_st(lds, BLS_SLOT_F, c.lane, one);
    }
    // a bad point anywhere in the group (lane pair k looks at pairs k, k + 6, ...)
    int bad = 0;
    for (uint32_t idx = (uint32_t)c.k; c.act && idx < n; idx += 6) bad |= pair_flag[(uint64_t)start + idx] == BLS_PAIR_BAD;
#pragma unroll 1
    for (int bit = 62; bit >= 0; --bit) {
        fp r;
        __syncthreads();
        f12_sqr(r, c, BLS_SLOT_F);
        __syncthreads();
        if (c.act) slot_st(lds, BLS_SLOT_F, c.lane, r);
        bls_miller_step(c, BLS_DBL_PROG, BLS_DBL_PROG_LEN, ws, pair_flag, start, n, max_n);
        if ((BLS_Z_ABS >> bit) & 1) bls_miller_step(c, BLS_ADD_PROG, BLS_ADD_PROG_LEN, ws, pair_flag, start, n, max_n);
    }
    __syncthreads();
    fp r;
    f12_conj(r, c, BLS_SLOT_F);
    for (int m = 1; m < 16; m <<= 1) bad |= __shfl_xor(bad, m, 64);
    if (gvalid && c.act) {
        fp_words::st(gt + (uint64_t)BLS_GT_WORDS * g + 12 * (2 * c.k + (int)c.role), r);
        if ((c.lane & 15) == 0) group_bad[g] = bad;
    }
}

// ---------------------------------------------------------------- final exponentiation
__global__ void __launch_bounds__(64) k_bls_final_exp(const uint32_t* __restrict__ gt, const int32_t* __restrict__ group_bad,
                                                       uint32_t n_groups, int32_t* __restrict__ verdict,
                                                       uint8_t* __restrict__ out576)
{
    __shared__ uint32_t lds[BLS_N_FE_REGS * 12 * 64];
    const bls_lane c = bls_lane_init(lds);
    const uint32_t g = blockIdx.x * BLS_GROUPS_PER_WAVE + (uint32_t)(c.lane >> 4);
    const bool gvalid = g < n_groups;
    {
        fp a;
        f12_one_coeff(a, c);  // rows past the last group work on 1
        if (gvalid && c.act) fp_words::ld(a, gt + (uint64_t)BLS_GT_WORDS * g + 12 * (2 * c.k + (int)c.role));
        if (c.act) slot_st(lds, 0, c.lane, a);
    }
    const int cj = BLS_CYCLO_J[c.k], part = BLS_CYCLO_PART[c.k];
    const bool plus = BLS_CYCLO_PLUS[c.k] != 0;
#pragma unroll 1
    for (int pc = 0; pc < BLS_FE_PROG_LEN; ++pc) {
        const uint32_t w = BLS_FE_PROG[pc];
        const int op = (int)(w & 255), d = (int)(w >> 8 & 255), sa = (int)(w >> 16 & 255), sb = (int)(w >> 24);
        fp r;
        __syncthreads();
        switch (op) {
        case BLS_FE_MUL: f12_mul(r, c, sa, sb); break;
        case BLS_FE_CSQR: f12_cyclo_sqr(r, c, sa, cj, part, plus); break;
        case BLS_FE_CONJ: f12_conj(r, c, sa); break;
        case BLS_FE_FROB: f12_frobenius(r, c, sa, sb, BLS_FROB[sb - 1]); break;
        default: f12_scale_inv(r, c, sa, sb); break;  // BLS_FE_INVSCALE
        }
        __syncthreads();
        if (c.act) slot_st(lds, d, c.lane, r);
    }
    __syncthreads();
    fp r, want;
    slot_ld(r, lds, 0, c.lane);
    f12_one_coeff(want, c);
    int is_one = !c.act || fp_eq(r, want);
    for (int m = 1; m < 16; m <<= 1) is_one &= __shfl_xor(is_one, m, 64);
    if (!gvalid || !c.act) return;
    if ((c.lane & 15) == 0) verdict[g] = group_bad[g] ? 2 : is_one;
    if (out576) {
        fp plain;
        fp_from_mont(plain, r);
        fp_store_be48(out576 + (uint64_t)576 * g + 48 * (2 * c.k + (int)c.role), plain);
    }
}

// ---------------------------------------------------------------- launchers
void launch_bls_prepare(hipStream_t s, const uint8_t* g1_be96, const uint8_t* g2_be192, uint64_t n_pairs, uint32_t* ws,
                        int32_t* pair_flag)
{
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(k_bls_prepare, dim3((unsigned)((2 * n_pairs + 255) / 256)), dim3(256), 0, s, g1_be96, g2_be192, n_pairs, ws,
                       pair_flag);
}
void launch_bls_miller(hipStream_t s, uint32_t* ws, const int32_t* pair_flag, const uint32_t* offsets, uint32_t n_groups,
                       uint32_t* gt, int32_t* group_bad)
{
    if (n_groups == 0) return;
    hipLaunchKernelGGL(k_bls_miller, dim3((n_groups + BLS_GROUPS_PER_WAVE - 1) / BLS_GROUPS_PER_WAVE), dim3(64), 0, s, ws, pair_flag,
                       offsets, n_groups, gt, group_bad);
}
void launch_bls_final_exp(hipStream_t s, const uint32_t* gt, const int32_t* group_bad, uint32_t n_groups, int32_t* verdict,
                          uint8_t* out576)
{
    if (n_groups == 0) return;
    hipLaunchKernelGGL(k_bls_final_exp, dim3((n_groups + BLS_GROUPS_PER_WAVE - 1) / BLS_GROUPS_PER_WAVE), dim3(64), 0, s, gt,
                       group_bad, n_groups, verdict, out576);
}

}  // namespace posevo
