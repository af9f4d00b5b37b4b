// engine_sigverify.cpp -- every unaggregated signature of an epoch decided, one pairing check per committee.
//   pe_verify_signatures      per group g (one committee's votes for one AttestationData: one message), secret weights r_j:
//                                 e(sum_j r_j pk_j, H(m_g)) * e(-g1, sum_j r_j sig_j) == 1
//   pe_profile_verify_*       the stripe knob, what the last call did, and its two weighted sums per group
//
// One call:  settle (decompression, the G2 subgroup test, the identity: such members get verdict 0 and a zero weight, so they
// are in neither sum) -> the two weighted sums (sigverify_kernels.hip, the existing finish kernels) -> ONE pairing run, a group of
// two pairs per committee (pairing_run, unchanged) -> only for the groups that failed: every member left as its own two-pair
// group, all of them in ONE further run (no recursion, no bisection) -> the plain aggregate of the members with verdict 1
// (k_g2_accumulate / k_g2_finish over the survivors' list).
// Synchronous; completes open pipelines first (enter); one GPU: PE_ERR_STATE under pe_dist_init*.
#include "engine_internal.h"
#include "../../include/posevo_profile.h"

using namespace posevo;

extern "C" {

int pe_verify_signatures(pe_engine* h, const uint8_t* signatures96, uint64_t n, const uint32_t* index, const uint32_t* signer,
                         const uint32_t* offsets, uint32_t n_groups, const uint8_t* message_points192, const uint64_t* scalars,
                         int32_t* member_verdict, int32_t* sig_status, int32_t* group_verdict, uint8_t* out_signatures96)
{
    if (!h || !offsets || (n && !signatures96)) return PE_ERR_INVALID_ARG;
    if (n_groups && (!message_points192 || !group_verdict)) return PE_ERR_INVALID_ARG;
    const uint32_t total = n_groups ? offsets[n_groups] : 0;
    if (total && (!signer || !member_verdict)) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));  // open pipelines complete
    const char* who = "pe_verify_signatures";
    if (h->dist_ready()) return refuse_dist(h, who);
    if (!h->have_points) return fail(h, PE_ERR_STATE, "pe_verify_signatures: no pubkeys loaded");
    if (n >= 0xFFFFFFFFull / 48) return fail(h, PE_ERR_CAPACITY, "pe_verify_signatures: too many signatures");
    for (uint32_t g = 0; g < n_groups; ++g)
        if (offsets[g + 1] < offsets[g]) return fail(h, PE_ERR_INVALID_ARG, "pe_verify_signatures: offsets not monotone");
    if (!index && total > n) return fail(h, PE_ERR_INVALID_ARG, "pe_verify_signatures: offsets exceed the number of signatures");
    for (uint32_t j = 0; j < total; ++j) {
        if (index && index[j] >= n) return fail(h, PE_ERR_INVALID_ARG, "pe_verify_signatures: signature index out of range");
        if (signer[j] >= h->n_val) return fail(h, PE_ERR_INVALID_ARG, "pe_verify_signatures: signer outside the registry");
        if (scalars && scalars[j] == 0) return fail(h, PE_ERR_INVALID_ARG, "pe_verify_signatures: a zero scalar");
    }
    const uint32_t k = h->verify_stripe;
    uint32_t* stats = h->verify_stats;
    std::fill(stats, stats + 5, 0u);
    stats[4] = k;
    h->verify_sums_pk.assign((size_t)96 * n_groups, 0);
    h->verify_sums_sig.assign((size_t)192 * n_groups, 0);
    if (n_groups == 0) return PE_OK;
    std::vector<uint64_t> weight(total);
    if (scalars) std::copy(scalars, scalars + total, weight.begin());
    else PE_TRY(draw_scalars(h, weight));

    // ---- settle: what never enters a sum
    hipStream_t s = h->stream;
    SettledSigs settled;  // the subgroup test always: the combination is sound over G2 only
    PE_TRY(settle_signatures(h, signatures96, n, 0, true, true, nullptr, &settled));
    uint32_t* const d_pts = settled.pts;
    HIP_TRY(h, hipGetLastError());
    std::vector<int32_t> row_status(n);
    if (n) HIP_TRY(h, hipMemcpyAsync(row_status.data(), settled.status, 4ull * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    auto row_of = [&](uint32_t j) { return index ? index[j] : j; };
    std::vector<int32_t> mstatus(total), mverdict(total, 0);
    for (uint32_t j = 0; j < total; ++j) {
        mstatus[j] = row_status[row_of(j)];
        if (mstatus[j] != 0) {
            weight[j] = 0;  // in neither sum
            ++stats[0];
        }
    }

    // ---- the two weighted sums
    std::vector<G1Group> gr2(n_groups), gr1(n_groups);
    G1Plan plan2, plan1;
    auto size_of = [&](uint32_t g) { return offsets[g + 1] - offsets[g]; };
    plan_g1(n_groups, size_of, gr2.data(), &plan2, G2_WG_SLOTS, G1_TARGET_LANES / 2, k);
    plan_g1(n_groups, size_of, gr1.data(), &plan1, G1_WG, G1_TARGET_LANES, k);
    for (uint32_t g = 0; g < n_groups; ++g) gr2[g].member_start = gr1[g].member_start = offsets[g];
    Workspace w;  // d_verify, bound to each phase's layout in turn: a later phase starts over from offset 0
    {
        Layout L;
        const auto r_index = L.take<uint32_t>(total), r_signer = L.take<uint32_t>(total);
        const auto r_scal = L.take<uint64_t>(total);
        const auto r_gr2 = L.take<G1Group>(n_groups), r_gr1 = L.take<G1Group>(n_groups);
        const auto r_part2 = L.take<uint32_t>(96ull * plan2.n_partials), r_part1 = L.take<uint32_t>(48ull * plan1.n_partials);
        const auto r_pk = L.take<uint8_t>(96ull * n_groups), r_sig = L.take<uint8_t>(192ull * n_groups);
        HIP_TRY(h, w.bind(h->d_verify, L, s));
        if (total) {
            if (index) HIP_TRY(h, w.put(r_index, index, total));
            HIP_TRY(h, w.put(r_signer, signer, total));
            HIP_TRY(h, w.put(r_scal, weight.data(), total));
        }
        HIP_TRY(h, w.put(r_gr2, gr2.data(), n_groups));
        HIP_TRY(h, w.put(r_gr1, gr1.data(), n_groups));
        launch_g2_weighted_accumulate(s, d_pts, index ? w(r_index) : nullptr, w(r_scal), w(r_gr2), n_groups, plan2.n_slots, w(r_part2));
        launch_g2_finish(s, w(r_part2), w(r_gr2), n_groups, w(r_sig));
        launch_g1_weighted_accumulate(s, h->d_points.as<uint32_t>(), w(r_signer), w(r_scal), w(r_gr1), n_groups, plan1.n_slots, w(r_part1));
        launch_g1_finish(s, w(r_part1), w(r_gr1), n_groups, 0, 0, w(r_pk), nullptr);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, w.get(r_pk, h->verify_sums_pk.data(), 96ull * n_groups));
        HIP_TRY(h, w.get(r_sig, h->verify_sums_sig.data(), 192ull * n_groups));
    }
    HIP_TRY(h, hipStreamSynchronize(s));

    // ---- decide: the pairs (sum r pk, H(m_g)), (-g1, sum r sig), one group of two per committee
    std::vector<int32_t> combined(n_groups);
    const WireAt msg_of = [&](uint32_t g) { return message_points192 + (size_t)192 * g; };
    PE_TRY(verify_pairs_run(
        h, who, n_groups, [&](uint32_t g) { return &h->verify_sums_pk[(size_t)96 * g]; }, msg_of,
        [&](uint32_t g) { return &h->verify_sums_sig[(size_t)192 * g]; }, combined.data()));
    stats[3] = 1;
    std::vector<uint32_t> again;  // the members the locate pass decides
    std::vector<int32_t> gverdict(n_groups);
    for (uint32_t g = 0; g < n_groups; ++g) {
        const bool msg_identity = (message_points192[(size_t)192 * g] & 0x40) != 0;
        if (combined[g] == PE_BLS_BAD_POINT) {
            gverdict[g] = PE_BLS_BAD_POINT;
        } else if (msg_identity) {
            gverdict[g] = 0;
        } else if (combined[g] == PE_BLS_VALID) {
            gverdict[g] = 1;
            for (uint32_t j = offsets[g]; j < offsets[g + 1]; ++j) {
                mverdict[j] = mstatus[j] == 0;
                if (mstatus[j] != 0) gverdict[g] = 0;
            }
        } else {
            gverdict[g] = 0;
            ++stats[1];
            for (uint32_t j = offsets[g]; j < offsets[g + 1]; ++j)
                if (mstatus[j] == 0) again.push_back(j);
        }
    }

    // ---- locate: every member of a failing group on its own, unscaled, all of them in one run
    const uint32_t n_again = (uint32_t)again.size();
    stats[2] = n_again;
    if (n_again) {
        std::vector<uint32_t> rows(2 * (size_t)n_again), group_of(n_again);
        for (uint32_t t = 0, g = 0; t < n_again; ++t) {
            rows[t] = signer[again[t]];
            rows[(size_t)n_again + t] = row_of(again[t]);
            while (again[t] >= offsets[g + 1]) ++g;
            group_of[t] = g;
        }
        Layout L;  // (the sums' regions are done with)
        const auto r_rows = L.take<uint32_t>(2ull * n_again);
        const auto r_be96 = L.take<uint8_t>(96ull * n_again), r_be192 = L.take<uint8_t>(192ull * n_again);
        HIP_TRY(h, w.bind(h->d_verify, L, s));
        HIP_TRY(h, w.put(r_rows, rows.data(), 2ull * n_again));
        launch_sv_rows_g1(s, h->d_points.as<uint32_t>(), w(r_rows), n_again, w(r_be96));
        launch_sv_rows_g2(s, d_pts, w(r_rows) + n_again, n_again, w(r_be192));
        HIP_TRY(h, hipGetLastError());
        std::vector<uint8_t> pk((size_t)96 * n_again), sg((size_t)192 * n_again);
        HIP_TRY(h, w.get(r_be96, pk.data(), 96ull * n_again));
        HIP_TRY(h, w.get(r_be192, sg.data(), 192ull * n_again));
        HIP_TRY(h, hipStreamSynchronize(s));
        std::vector<int32_t> one_by_one(n_again);
        PE_TRY(verify_pairs_run(
            h, who, n_again, [&](uint32_t t) { return &pk[(size_t)96 * t]; }, [&](uint32_t t) { return msg_of(group_of[t]); },
            [&](uint32_t t) { return &sg[(size_t)192 * t]; }, one_by_one.data()));
        stats[3] = 2;
        for (uint32_t t = 0; t < n_again; ++t) mverdict[again[t]] = one_by_one[t] == PE_BLS_VALID;
    }

    // ---- aggregate: the plain sum of the members with verdict 1
    if (out_signatures96) {
        std::vector<uint32_t> keep, keep_off((size_t)n_groups + 1);
        keep.reserve(total);
        for (uint32_t g = 0; g < n_groups; ++g) {
            keep_off[g] = (uint32_t)keep.size();
            for (uint32_t j = offsets[g]; j < offsets[g + 1]; ++j)
                if (mverdict[j]) keep.push_back(row_of(j));
        }
        keep_off[n_groups] = (uint32_t)keep.size();
        G1Plan plan;
        plan_g1(n_groups, [&](uint32_t g) { return keep_off[g + 1] - keep_off[g]; }, gr2.data(), &plan, G2_WG_SLOTS, G1_TARGET_LANES / 2);
        for (uint32_t g = 0; g < n_groups; ++g) gr2[g].member_start = keep_off[g];
        Layout L;
        const auto r_keep = L.take<uint32_t>(keep.size());
        const auto r_g = L.take<G1Group>(n_groups);
        const auto r_part = L.take<uint32_t>(96ull * plan.n_partials);
        const auto r_out = L.take<uint8_t>(192ull * n_groups);
        HIP_TRY(h, w.bind(h->d_verify, L, s));
        if (!keep.empty()) HIP_TRY(h, w.put(r_keep, keep.data(), keep.size()));
        HIP_TRY(h, w.put(r_g, gr2.data(), n_groups));
        launch_g2_accumulate(s, d_pts, w(r_keep), w(r_g), n_groups, plan.n_slots, w(r_part));
        launch_g2_finish(s, w(r_part), w(r_g), n_groups, w(r_out));
        HIP_TRY(h, hipGetLastError());
        std::vector<uint8_t> out192((size_t)192 * n_groups);
        HIP_TRY(h, w.get(r_out, out192.data(), 192ull * n_groups));
        HIP_TRY(h, hipStreamSynchronize(s));
        PE_TRY(pe_g2_compress(out192.data(), n_groups, out_signatures96));
    }
    std::copy(mverdict.begin(), mverdict.end(), member_verdict);
    if (sig_status) std::copy(mstatus.begin(), mstatus.end(), sig_status);
    std::copy(gverdict.begin(), gverdict.end(), group_verdict);
    return PE_OK;
}

int pe_profile_verify_set_stripe(pe_engine* h, uint32_t k)
{
    if (!h) return PE_ERR_INVALID_ARG;
    if (k < 1 || k > PE_VERIFY_STRIPE_MAX) return fail(h, PE_ERR_INVALID_ARG, "pe_profile_verify_set_stripe: 1 .. PE_VERIFY_STRIPE_MAX");
    h->verify_stripe = k;
    return PE_OK;
}

int pe_profile_verify_stats(const pe_engine* h, uint32_t out[5])
{
    if (!h || !out) return PE_ERR_INVALID_ARG;
    std::copy(h->verify_stats, h->verify_stats + 5, out);
    return PE_OK;
}

int pe_profile_verify_sums(const pe_engine* h, uint32_t n_groups, uint8_t* out_pk96, uint8_t* out_sig192)
{
    if (!h || (n_groups && (!out_pk96 || !out_sig192))) return PE_ERR_INVALID_ARG;
    if ((size_t)96 * n_groups != h->verify_sums_pk.size()) return PE_ERR_INVALID_ARG;
    if (n_groups) {
        memcpy(out_pk96, h->verify_sums_pk.data(), h->verify_sums_pk.size());
        memcpy(out_sig192, h->verify_sums_sig.data(), h->verify_sums_sig.size());
    }
    return PE_OK;
}

}  // extern "C"

static_assert(PE_VERIFY_STRIPE_MAX == SV_STRIPE_MAX, "a plane's mask of set members is SV_STRIPE_MAX bits");
