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
//
// pe_verify_resident_data is the same call with the messages taken from the groups themselves: in front of the
// prepare pass, on the same stream and in the same workspace,
//     k_att_signing_roots over AttGroup::rep -> k_h2c_expand -> k_h2c_map -> k_h2c_finish
// write the message points where the caller's would have been copied.  In go the 72 bytes of pe_attester_domains and the tag;
// nothing about the messages comes back before the verdicts, beside which the roots travel if the caller asks for them.
#include "att_signing_row.h"
#include "engine_internal.h"

using namespace posevo;

static_assert(BLS_RES_REASONS + 2 == PE_VERIFY_RESIDENT_STATS, "the counters of pe_profile_verify_resident_stats");
static_assert(BLS_UNDECIDED == PE_BLS_UNDECIDED, "kernels.h restates the verdict");

namespace {

// Where a group's message comes from: the caller's points (pe_verify_resident), or the groups' own AttestationData under the
// caller's domains (pe_verify_resident_data), in which case the points are made here, in the same workspace.
struct ResidentMessages {
    const uint8_t* points192 = nullptr;
    uint32_t n_points = 0;
    const uint32_t* point_of_row = nullptr;
    const pe_attester_domains* dom = nullptr;
    uint8_t* out_roots32 = nullptr;  // nullable, host, 32 x cap
};

const char ETH2_DST[] = PE_ETH2_DST;

int verify_resident_run(pe_engine* h, const std::string& who, const ResidentMessages& m, uint32_t flags, uint32_t cap,
                        int32_t* verdict)
{
    const bool from_data = m.dom != nullptr;
    const uint8_t* message_points192 = m.points192;
    const uint32_t n_points = m.n_points;
    const uint32_t* point_of_row = m.point_of_row;
    PE_TRY(enter(h));  // open pipelines complete: the aggregate's points, unions and groups are written
    if (h->dist_ready()) return refuse_dist(h, who.c_str());
    const pe_engine::ResidentVerify& rv = h->rv;
    if (!rv.valid || !h->rr.valid || h->rr.generation != rv.rr_generation || h->res_generation != rv.res_generation ||
        h->rr.set != 0 || h->rr.arena != rv.arena || h->rr.n_groups == NONE32)
        return fail(h, PE_ERR_STATE, who + ": the handle's last aggregate is not a completed pe_aggregate_signed over "
                                     "rows in device memory with aggregate pubkeys requested");
    PE_TRY(resident_precheck(h, who.c_str()));
    const uint32_t ng = h->rr.n_groups, n_in = rv.n_in;
    if (!from_data) {
        if (point_of_row) {
            for (uint32_t i = 0; i < n_in; ++i)
                if (point_of_row[i] >= n_points) return fail(h, PE_ERR_INVALID_ARG, who + ": point_of_row names a point beyond n_points");
        } else if (n_points < ng) {
            return fail(h, PE_ERR_INVALID_ARG, who + ": fewer message points than groups");
        }
        if (ng && !message_points192) return fail(h, PE_ERR_INVALID_ARG, who + ": no message points");
    }
    if (cap < ng) return fail(h, PE_ERR_CAPACITY, who + ": verdict capacity below the groups formed");
    uint32_t* stats = h->verify_resident_stats;
    if (ng == 0) {
        memset(stats, 0, sizeof(h->verify_resident_stats));
        if (cap) memset(verdict, 0, 4ull * cap);
        if (cap && m.out_roots32) memset(m.out_roots32, 0, 32ull * cap);
        return PE_OK;
    }
    ResidentParts P;
    PE_TRY(resident_parts(h, &P));
    const ResPoints kept = res_points_layout(h->arena[rv.arena].d_res_points.p, n_in);
    // the caller's message points: read in place from 16-byte aligned device memory, copied otherwise
    const MemKind msg_kind = from_data ? MemKind::Device : mem_kind(message_points192);
    const bool msg_in_place = !from_data && reads_in_place(msg_kind, message_points192);
    const size_t G = ng, por_bytes = point_of_row ? 4 * (size_t)n_in : 0;
    Layout L;
    const ResidentVerifyLayout r = resident_verify_layout(L, G, por_bytes, from_data ? 192 * G : (msg_in_place ? 0 : 192 * (size_t)n_points),
                                                          BLS_PAIR_WORDS, BLS_GT_WORDS, from_data ? sizeof(ETH2_DST) - 1 : 0,
                                                          H2C_POINT_WORDS);
    hipStream_t s = h->stream;
    Workspace w;
    HIP_TRY(h, w.bind(h->d_bls, L, s));
    std::vector<uint8_t>& head = h->verify_head;  // the handle's, so that no return frees it before the copy has read it
    head.assign(256 + por_bytes, 0);
    memcpy(head.data(), NEG_G1_BE96, 96);
    if (point_of_row) memcpy(head.data() + 256, point_of_row, por_bytes);
    HIP_TRY(h, w.put(r.head, head.data(), head.size()));
    BlsResidentArgs a{};
    if (from_data) {
        // the groups' messages, made where they are read: signing roots of the first rows -> (u0, u1) -> points -> wire bytes
        AttDomains dom;
        att_domains_load(m.dom->fork_epoch, m.dom->domain_previous, m.dom->domain_current, dom);
        HIP_TRY(h, w.put(r.dst, ETH2_DST, sizeof(ETH2_DST) - 1));
        launch_att_signing_roots(s, P.rows, n_in, P.grp, P.plan, ng, dom, w(r.roots));
        launch_h2c_expand(s, w(r.roots), ng, 32, w(r.dst), (uint32_t)(sizeof(ETH2_DST) - 1), w(r.h2c.u));
        launch_h2c_map(s, w(r.h2c.u), 2 * ng, w(r.h2c.pts));
        launch_h2c_finish(s, w(r.h2c.pts), ng, w(r.msg), nullptr);
        a.msg192 = w(r.msg);
    } else {
        HIP_TRY(h, device_view(w, r.msg, msg_kind, message_points192, 192 * (size_t)n_points, &a.msg192));
    }
    HIP_TRY(h, w.zero(r.sub, G));
    HIP_TRY(h, w.zero(r.stats, 16));
    a.pk_xyzz48 = kept.pk_xyzz48;
    a.sig_mont48 = kept.sig_mont48;
    a.sig_bad = kept.sig_bad;
    a.point_of_row = point_of_row ? w(r.por) : nullptr;
    a.neg_g1_be96 = w(r.head);
    a.grp = P.grp;
    a.union_info = P.res_info;
    a.n_groups = ng;
    a.ws = w(r.ws);
    a.pair_flag = w(r.flag);
    a.offsets = w(r.off);
    a.ident = w(r.ident);
    a.sig_status = w(r.sub);
    a.fe_verdict = w(r.fe);
    a.stats = w(r.stats);
    a.verdict = w(r.verdict);
    a.apply = (flags & PE_VERIFY_APPLY) ? 1u : 0u;
    launch_bls_resident_prepare(s, a);
    // sums of members of G2 lie in G2: the pass runs exactly when the leg did not check its members
    const bool subgroup_pass = !rv.checked_subgroup;
    if (subgroup_pass) launch_g2_subgroup_check(s, kept.sig_mont48, ng, w(r.sub));
    launch_bls_miller(s, a.ws, a.pair_flag, a.offsets, ng, w(r.gt), w(r.gbad));
    launch_bls_final_exp(s, w(r.gt), w(r.gbad), ng, w(r.fe), nullptr);
    launch_bls_resident_settle(s, a);
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> out(16 + G);
    HIP_TRY(h, w.get(r.out, out.data(), out.size()));
    std::vector<uint8_t> roots(m.out_roots32 ? 32 * G : 0);  // staged: an error below writes nothing of the caller's
    if (m.out_roots32) HIP_TRY(h, w.get(r.roots, roots.data(), roots.size()));
    HIP_TRY(h, hipStreamSynchronize(s));
    memcpy(verdict, out.data() + 16, 4ull * ng);
    if (cap > ng) memset(verdict + ng, 0, 4ull * (cap - ng));
    if (m.out_roots32) {
        memcpy(m.out_roots32, roots.data(), roots.size());
        if (cap > ng) memset(m.out_roots32 + 32ull * ng, 0, 32ull * (cap - ng));
    }
    memcpy(stats, out.data(), 4 * BLS_RES_REASONS);
    stats[BLS_RES_REASONS] = subgroup_pass ? 1u : 0u;
    stats[BLS_RES_REASONS + 1] = ng;
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_verify_resident(pe_engine* h, const uint8_t* message_points192, uint32_t n_points, const uint32_t* point_of_row,
                       uint32_t flags, uint32_t cap, int32_t* verdict)
{
    if (!h || (flags & ~(uint32_t)PE_VERIFY_APPLY) || (cap && !verdict)) return PE_ERR_INVALID_ARG;
    ResidentMessages m;
    m.points192 = message_points192;
    m.n_points = n_points;
    m.point_of_row = point_of_row;
    return verify_resident_run(h, "pe_verify_resident", m, flags, cap, verdict);
}

int pe_verify_resident_data(pe_engine* h, const pe_attester_domains* dom, uint32_t flags, uint32_t cap, int32_t* verdict,
                            uint8_t* out_roots32)
{
    if (!h || (flags & ~(uint32_t)PE_VERIFY_APPLY) || (cap && !verdict)) return PE_ERR_INVALID_ARG;
    if (!dom) return fail(h, PE_ERR_INVALID_ARG, "pe_verify_resident_data: no domains");
    ResidentMessages m;
    m.dom = dom;
    m.out_roots32 = out_roots32;
    return verify_resident_run(h, "pe_verify_resident_data", m, flags, cap, verdict);
}

int pe_profile_verify_resident_stats(const pe_engine* h, uint32_t out[PE_VERIFY_RESIDENT_STATS])
{
    if (!h || !out) return PE_ERR_INVALID_ARG;
    memcpy(out, h->verify_resident_stats, sizeof(h->verify_resident_stats));
    return PE_OK;
}

}  // extern "C"
