// bls_resident_kernels.hip -- what feeds the pairing check from the resident aggregate and what settles its result, for gfx950
// (host side: engine_resident_verify.cpp).
//
// pe_aggregate_signed over device rows leaves, per group, the aggregate key (k_g1_finish's XYZZ words), the aggregate signature
// (k_g2_aggregate_rows' affine Montgomery row) and the count of members left out of it in device memory.  Between two small
// kernels of this file run the unchanged k_bls_miller and k_bls_final_exp of bls_kernels.hip:
//
//   k_bls_resident_prepare  a lane pair per pair, two pairs per group: 2g = (aggregate key, H(m)), 2g + 1 = (-g1, aggregate
//                           signature), written as k_bls_prepare writes them (BLS_PAIR_WORDS / BLS_WS_P / BLS_WS_T of kernels.h).
//                           The key is normalised here (one inversion per group: the finish kernel keeps its XYZZ output as it
//                           is); the message point goes through wire_load_g2 (canonical coordinates, the curve equation); the
//                           signature is copied.  Pair flags as k_bls_miller reads them: infinity on a side contributes 1, a bad
//                           message point flags the group.  Offsets: group g = pairs [2g, 2g + 2).
//   k_bls_resident_settle   a lane per group: the rule table of pe_verify_resident (include/posevo.h; tests/verify_resident_model.py
//                           restates it), first matching row wins; the verdict, the deciding row's counter and, under
//                           PE_VERIFY_APPLY, AttGroup::sig_valid.
//
// Neither kernel calls anything that is not inlined (no scratch) and neither touches its wave priority.
#include "fp12.h"
#include "fp_mem.h"
#include "fp_sqrt.h"
#include "kernels.h"
#include "wire_points.h"

namespace posevo {

// ---------------------------------------------------------------- prepare
__global__ void __launch_bounds__(256) k_bls_resident_prepare(const BlsResidentArgs a)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t pair = gid >> 1;
    const uint32_t g = pair >> 1;
    if (g >= a.n_groups) return;  // whole lane pairs leave together
    const bool role = (gid & 1) != 0;
    const bool sig_pair = (pair & 1) != 0;  // the same in both lanes of a pair: the exchanges below stay defined
    fp qx, qy, pc;
    int32_t flag;
    uint32_t id;
    if (!sig_pair) {
        // P = the aggregate key: x = X / ZZ, y = Y / ZZZ through 1 / (ZZ ZZZ); ZZ = 0 (no member, or a sum that cancelled) gives zeros
        // (role 0 carries x and needs 1 / ZZ = ZZZ / (ZZ ZZZ); role 1 carries y and needs 1 / ZZZ = ZZ / (ZZ ZZZ))
        const uint32_t* kw = a.pk_xyzz48 + (size_t)G1X_WORDS * g;
        fp zz, zzz, num, t, inv, u;
        fp_vec16::ld(zz, kw + 24);
        fp_vec16::ld(zzz, kw + 36);
        fp_vec16::ld(num, kw + (role ? 12 : 0));
        const bool k_inf = fp_is_zero(zz);
        fp_mul(t, zz, zzz);
        fp_inv_inline(inv, t);
        fp_select(u, role, zz, zzz);
        fp_mul(t, inv, u);
        fp_mul(pc, num, t);
        // Q = H(m) of the group's representative row
        const uint32_t pt = a.point_of_row ? a.point_of_row[a.grp[g].rep] : g;
        bool m_inf;
        const bool bad = wire_load_g2(qx, qy, m_inf, a.msg192 + (size_t)192 * pt, role);
        flag = bad ? BLS_PAIR_BAD : (k_inf || m_inf) ? BLS_PAIR_SKIP : BLS_PAIR_LIVE;
        id = (k_inf ? (uint32_t)BLS_RES_ID_KEY : 0u) | (m_inf ? (uint32_t)BLS_RES_ID_MSG : 0u);
    } else {
        // P = -g1 (its leading bytes carry no flag bits); Q = the aggregate signature, the zero row at infinity
        fp w;
        fp_load_be48(w, a.neg_g1_be96 + (role ? 48 : 0));
        fp_to_mont(pc, w);
        const uint32_t* s = a.sig_mont48 + (size_t)48 * g + (role ? 12 : 0);
        fp_vec16::ld(qx, s);
        fp_vec16::ld(qy, s + 24);
        const bool s_inf = pair_and(fp_is_zero(qx) && fp_is_zero(qy));
        flag = s_inf ? BLS_PAIR_SKIP : BLS_PAIR_LIVE;
        id = s_inf ? (uint32_t)BLS_RES_ID_SIG : 0u;
    }
    fp one;
    f2_set_one(one, role);
    uint32_t* row = a.ws + (size_t)BLS_PAIR_WORDS * pair;
    fp_words::st(row + 12 * (0 + (int)role), qx);
    fp_words::st(row + 12 * (2 + (int)role), qy);
    fp_words::st(row + 12 * (BLS_WS_P + (int)role), pc);
    fp_words::st(row + 12 * (BLS_WS_T + 0 + (int)role), qx);
    fp_words::st(row + 12 * (BLS_WS_T + 2 + (int)role), qy);
    fp_words::st(row + 12 * (BLS_WS_T + 4 + (int)role), one);
    // the two pairs of a group sit in neighbouring lane pairs of one wave (4 | 64): the group's identity word is the OR of both
    const uint32_t id_other = (uint32_t)__shfl_xor((int)id, 2, 64);
    if (role) return;
    a.pair_flag[pair] = flag;
    if (sig_pair) return;
    a.ident[g] = id | id_other;
    a.offsets[g] = 2 * g;
    if (g + 1 == a.n_groups) a.offsets[g + 1] = 2 * (g + 1);
}

// ---------------------------------------------------------------- settle
__global__ void __launch_bounds__(256) k_bls_resident_settle(const BlsResidentArgs a)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_groups) return;
    const uint32_t id = a.ident[g];
    const int32_t fe = a.fe_verdict[g];
    int32_t v = 0;
    uint32_t why;
    if (a.grp[g].status_agg != 0) { v = BLS_UNDECIDED; why = BLS_RES_NO_COMMITTEE; }
    else if (fe == 2) { v = 2; why = BLS_RES_BAD_MESSAGE; }
    else if (a.union_info[2 * g + 1] != 0) why = BLS_RES_OVERLAP;
    else if (a.sig_bad[g] != 0) why = BLS_RES_BAD_MEMBER;
    else if (id & BLS_RES_ID_KEY) why = BLS_RES_EMPTY_KEY;
    else if (id & BLS_RES_ID_SIG) why = BLS_RES_IDENTITY_SIG;
    else if (id & BLS_RES_ID_MSG) why = BLS_RES_IDENTITY_MSG;
    else if (a.sig_status[g] != 0) why = BLS_RES_NOT_G2;
    else { v = fe == 1 ? 1 : 0; why = BLS_RES_PAIRING; }
    a.verdict[g] = v;
    // one atomic per wave and deciding row (an honest slot puts every lane on the same counter)
#pragma unroll 1
    for (uint32_t r = 0; r < BLS_RES_REASONS; ++r) {
        const unsigned long long m = __ballot(why == r);
        if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(a.stats + r, (uint32_t)__popcll(m));
    }
    if (a.apply && why != BLS_RES_NO_COMMITTEE && v != 1) a.grp[g].sig_valid = 0;  // sig_valid &= (verdict == 1)
}

// ---------------------------------------------------------------- launchers
void launch_bls_resident_prepare(hipStream_t s, const BlsResidentArgs& a)
{
    if (a.n_groups == 0) return;
    hipLaunchKernelGGL(k_bls_resident_prepare, dim3((unsigned)((4 * (uint64_t)a.n_groups + 255) / 256)), dim3(256), 0, s, a);
}
void launch_bls_resident_settle(hipStream_t s, const BlsResidentArgs& a)
{
    if (a.n_groups == 0) return;
    hipLaunchKernelGGL(k_bls_resident_settle, dim3((a.n_groups + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace posevo
