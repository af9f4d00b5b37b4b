// engine_resident_verify.cpp -- pe_verify_resident: every group of the resident aggregate decided by the pairing check, from the
// points where they lie.
//
// pe_aggregate_signed over device rows leaves each group's aggregate key, aggregate signature and left-out count in the arena's
// d_res_points (engine_g1.cpp).  This call brings in the message points and, optionally, which point each input row names, and
// runs on the engine's stream over a workspace in d_bls laid out as pairing_run lays it out:
//     k_bls_resident_prepare -> [k_g2_subgroup_check over the aggregate signatures] -> k_bls_miller -> k_bls_final_exp
//     -> k_bls_resident_settle
// No per-group point crosses to the host: in go the message points, point_of_row and one 256-byte header (-g1); out come 4 bytes
// per group and the 64 bytes of counters behind pe_profile_verify_resident_stats.  Under PE_VERIFY_APPLY the settle pass writes
// AttGroup::sig_valid, which the device-row handlers (engine_resident.cpp) read as they always did.
// Synchronous; completes open pipelines first; one GPU.
#include "engine_internal.h"

using namespace posevo;

static_assert(BLS_RES_REASONS + 2 == PE_VERIFY_RESIDENT_STATS, "the counters of pe_profile_verify_resident_stats");
static_assert(BLS_UNDECIDED == PE_BLS_UNDECIDED, "kernels.h restates the verdict");

extern "C" {

int pe_verify_resident(pe_engine* h, const uint8_t* message_points192, uint32_t n_points, const uint32_t* point_of_row,
                       uint32_t flags, uint32_t cap, int32_t* verdict)
{
    if (!h || (flags & ~(uint32_t)PE_VERIFY_APPLY) || (cap && !verdict)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));  // open pipelines complete: the aggregate's points, unions and groups are written
    if (h->dist_ready()) return refuse_dist(h, "pe_verify_resident");
    const pe_engine::ResidentVerify& rv = h->rv;
    if (!rv.valid || !h->rr.valid || h->rr.generation != rv.rr_generation || h->res_generation != rv.res_generation ||
        h->rr.set != 0 || h->rr.arena != rv.arena || h->rr.n_groups == NONE32)
        return fail(h, PE_ERR_STATE, "pe_verify_resident: the handle's last aggregate is not a completed pe_aggregate_signed over "
                                     "rows in device memory with aggregate pubkeys requested");
    PE_TRY(resident_precheck(h, "pe_verify_resident"));
    const uint32_t ng = h->rr.n_groups, n_in = rv.n_in;
    if (point_of_row) {
        for (uint32_t i = 0; i < n_in; ++i)
            if (point_of_row[i] >= n_points) return fail(h, PE_ERR_INVALID_ARG, "pe_verify_resident: point_of_row names a point beyond n_points");
    } else if (n_points < ng) {
        return fail(h, PE_ERR_INVALID_ARG, "pe_verify_resident: fewer message points than groups");
    }
    if (ng && !message_points192) return fail(h, PE_ERR_INVALID_ARG, "pe_verify_resident: no message points");
    if (cap < ng) return fail(h, PE_ERR_CAPACITY, "pe_verify_resident: verdict capacity below the groups formed");
    uint32_t* stats = h->verify_resident_stats;
    if (ng == 0) {
        memset(stats, 0, sizeof(h->verify_resident_stats));
        if (cap) memset(verdict, 0, 4ull * cap);
        return PE_OK;
    }
    ResidentParts P;
    PE_TRY(resident_parts(h, &P));
    const ResPoints kept = res_points_layout(h->arena[rv.arena].d_res_points.p, n_in);
    // the message points: read in place from 16-byte aligned device memory, copied otherwise
    const MemKind msg_kind = mem_kind(message_points192);
    const bool msg_in_place = msg_kind == MemKind::Device && (reinterpret_cast<uintptr_t>(message_points192) & 15) == 0;
    const size_t o_head = 0, o_por = o_head + 256, o_msg = o_por + up256(point_of_row ? 4 * (size_t)n_in : 0),
                 o_off = o_msg + up256(msg_in_place ? 0 : 192 * (size_t)n_points), o_ws = o_off + up256(4 * ((size_t)ng + 1)),
                 o_flag = o_ws + up256(4 * (size_t)BLS_PAIR_WORDS * 2 * ng), o_gt = o_flag + up256(8 * (size_t)ng),
                 o_gbad = o_gt + up256(4 * (size_t)BLS_GT_WORDS * ng), o_fe = o_gbad + up256(4 * (size_t)ng),
                 o_ident = o_fe + up256(4 * (size_t)ng), o_sub = o_ident + up256(4 * (size_t)ng),
                 o_out = o_sub + up256(4 * (size_t)ng), total = o_out + 64 + 4 * (size_t)ng;  // counters | verdicts: one copy out
    HIP_TRY(h, h->d_bls.ensure(total));
    uint8_t* d = h->d_bls.as<uint8_t>();
    hipStream_t s = h->stream;
    std::vector<uint8_t>& head = h->verify_head;  // -g1 | point_of_row, one copy in; the handle's, so that no return frees it early
    head.assign(256 + (point_of_row ? 4 * (size_t)n_in : 0), 0);
    memcpy(head.data(), NEG_G1_BE96, 96);
    if (point_of_row) memcpy(head.data() + 256, point_of_row, 4 * (size_t)n_in);
    HIP_TRY(h, hipMemcpyAsync(d + o_head, head.data(), head.size(), hipMemcpyHostToDevice, s));
    if (!msg_in_place)
        HIP_TRY(h, hipMemcpyAsync(d + o_msg, message_points192, 192 * (size_t)n_points,
                                  msg_kind == MemKind::Device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemsetAsync(d + o_sub, 0, 4 * (size_t)ng, s));
    HIP_TRY(h, hipMemsetAsync(d + o_out, 0, 64, s));
    BlsResidentArgs a{};
    a.pk_xyzz48 = kept.pk_xyzz48;
    a.sig_mont48 = kept.sig_mont48;
    a.sig_bad = kept.sig_bad;
    a.msg192 = msg_in_place ? message_points192 : d + o_msg;
    a.point_of_row = point_of_row ? reinterpret_cast<const uint32_t*>(d + o_por) : nullptr;
    a.neg_g1_be96 = d + o_head;
    a.grp = P.grp;
    a.union_info = P.res_info;
    a.n_groups = ng;
    a.ws = reinterpret_cast<uint32_t*>(d + o_ws);
    a.pair_flag = reinterpret_cast<int32_t*>(d + o_flag);
    a.offsets = reinterpret_cast<uint32_t*>(d + o_off);
    a.ident = reinterpret_cast<uint32_t*>(d + o_ident);
    a.sig_status = reinterpret_cast<const int32_t*>(d + o_sub);
    a.fe_verdict = reinterpret_cast<const int32_t*>(d + o_fe);
    a.stats = reinterpret_cast<uint32_t*>(d + o_out);
    a.verdict = reinterpret_cast<int32_t*>(d + o_out + 64);
    a.apply = (flags & PE_VERIFY_APPLY) ? 1u : 0u;
    uint32_t* gt = reinterpret_cast<uint32_t*>(d + o_gt);
    int32_t* gbad = reinterpret_cast<int32_t*>(d + o_gbad);
    launch_bls_resident_prepare(s, a);
    // sums of members of G2 lie in G2: the pass runs exactly when the leg did not check its members
    const bool subgroup_pass = !rv.checked_subgroup;
    if (subgroup_pass) launch_g2_subgroup_check(s, kept.sig_mont48, ng, reinterpret_cast<int32_t*>(d + o_sub));
    launch_bls_miller(s, a.ws, a.pair_flag, a.offsets, ng, gt, gbad);
    launch_bls_final_exp(s, gt, gbad, ng, reinterpret_cast<int32_t*>(d + o_fe), nullptr);
    launch_bls_resident_settle(s, a);
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> out(16 + (size_t)ng);
    HIP_TRY(h, hipMemcpyAsync(out.data(), d + o_out, 4 * out.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    memcpy(verdict, out.data() + 16, 4ull * ng);
    if (cap > ng) memset(verdict + ng, 0, 4ull * (cap - ng));
    memcpy(stats, out.data(), 4 * BLS_RES_REASONS);
    stats[BLS_RES_REASONS] = subgroup_pass ? 1u : 0u;
    stats[BLS_RES_REASONS + 1] = ng;
    return PE_OK;
}

int pe_profile_verify_resident_stats(const pe_engine* h, uint32_t out[PE_VERIFY_RESIDENT_STATS])
{
    if (!h || !out) return PE_ERR_INVALID_ARG;
    memcpy(out, h->verify_resident_stats, sizeof(h->verify_resident_stats));
    return PE_OK;
}

}  // extern "C"
