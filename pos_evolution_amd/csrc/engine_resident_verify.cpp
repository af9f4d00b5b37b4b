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
    const bool msg_in_place = reads_in_place(msg_kind, message_points192);
    const size_t G = ng, por_bytes = point_of_row ? 4 * (size_t)n_in : 0;
    Layout L;
    const auto r_head = L.take_bytes(256 + por_bytes);  // -g1 in 256 bytes | point_of_row: one copy in
    const auto r_por = r_head.part<uint32_t>(256, por_bytes / 4);
    const auto r_msg = L.take<uint8_t>(msg_in_place ? 0 : 192 * (size_t)n_points);
    const auto r_off = L.take<uint32_t>(G + 1), r_ws = L.take<uint32_t>((size_t)BLS_PAIR_WORDS * 2 * G);
    const auto r_flag = L.take<int32_t>(2 * G);
    const auto r_gt = L.take<uint32_t>((size_t)BLS_GT_WORDS * G);
    const auto r_gbad = L.take<int32_t>(G), r_fe = L.take<int32_t>(G);
    const auto r_ident = L.take<uint32_t>(G);
    const auto r_sub = L.take<int32_t>(G);
    const auto r_out = L.take_bytes<uint32_t>(64 + 4 * G);  // counters | verdicts: one copy out
    const auto r_stats = r_out.part<uint32_t>(0, 16);
    const auto r_verdict = r_out.part<int32_t>(64, G);
    hipStream_t s = h->stream;
    Workspace w;
    HIP_TRY(h, w.bind(h->d_bls, L, s));
    std::vector<uint8_t>& head = h->verify_head;  // the handle's, so that no return frees it before the copy has read it
    head.assign(256 + por_bytes, 0);
    memcpy(head.data(), NEG_G1_BE96, 96);
    if (point_of_row) memcpy(head.data() + 256, point_of_row, por_bytes);
    HIP_TRY(h, w.put(r_head, head.data(), head.size()));
    BlsResidentArgs a{};
    HIP_TRY(h, device_view(w, r_msg, msg_kind, message_points192, 192 * (size_t)n_points, &a.msg192));
    HIP_TRY(h, w.zero(r_sub, G));
    HIP_TRY(h, w.zero(r_stats, 16));
    a.pk_xyzz48 = kept.pk_xyzz48;
    a.sig_mont48 = kept.sig_mont48;
    a.sig_bad = kept.sig_bad;
    a.point_of_row = point_of_row ? w(r_por) : nullptr;
    a.neg_g1_be96 = w(r_head);
    a.grp = P.grp;
    a.union_info = P.res_info;
    a.n_groups = ng;
    a.ws = w(r_ws);
    a.pair_flag = w(r_flag);
    a.offsets = w(r_off);
    a.ident = w(r_ident);
    a.sig_status = w(r_sub);
    a.fe_verdict = w(r_fe);
    a.stats = w(r_stats);
    a.verdict = w(r_verdict);
    a.apply = (flags & PE_VERIFY_APPLY) ? 1u : 0u;
    launch_bls_resident_prepare(s, a);
    // sums of members of G2 lie in G2: the pass runs exactly when the leg did not check its members
    const bool subgroup_pass = !rv.checked_subgroup;
    if (subgroup_pass) launch_g2_subgroup_check(s, kept.sig_mont48, ng, w(r_sub));
    launch_bls_miller(s, a.ws, a.pair_flag, a.offsets, ng, w(r_gt), w(r_gbad));
    launch_bls_final_exp(s, w(r_gt), w(r_gbad), ng, w(r_fe), nullptr);
    launch_bls_resident_settle(s, a);
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> out(16 + G);
    HIP_TRY(h, w.get(r_out, out.data(), out.size()));
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
