// engine_batch.cpp -- batch verification of BLS aggregates by random linear combination.
//   pe_batch_verify                 per group (aggregate pubkey, H(m), signature): the verdict pe_fast_aggregate_verify gives,
//                                   reached in the honest case with ONE final exponentiation for the whole call:
//                                     prod_i e(r_i pk_i, H(m_i)) * e(-g1, sum_i r_i sig_i) == 1
//   pe_batch_fast_aggregate_verify  the same over registry indices: the aggregate pubkeys go the route of pe_g1_sum
//   pe_profile_batch_*              the chunk knob, what the last call did, and the value its verdict compared with 1
//
// One call:  settle (curve equations, identities, signatures outside G2: they never enter the batch) -> the live groups, c to a
// chunk -> r pk and r sig -> per chunk c message pairs and one signature pair = one group of the unchanged k_bls_miller -> the
// product of the chunk values, a tree of fan-in F -> k_bls_final_exp over that ONE value.  It is 1: every live group is valid.
// It is not: k_bls_final_exp over the chunk values (1 / c of the per-group work), then the per-group path (pairing_run, unscaled)
// over the live groups of the failing chunks.  No recursion, no loop.
// Both calls are synchronous and complete open pipelines first (enter); one GPU: PE_ERR_STATE under pe_dist_init*.
#include <sys/random.h>

#include "engine_internal.h"

using namespace posevo;

namespace posevo {

int draw_scalars(pe_engine* h, std::vector<uint64_t>& out)
{
    uint8_t* p = reinterpret_cast<uint8_t*>(out.data());
    size_t left = out.size() * sizeof(uint64_t);
    while (left) {
        const ssize_t got = getrandom(p, std::min<size_t>(left, 256), 0);  // up to 256 bytes are never interrupted
        if (got <= 0) return fail(h, PE_ERR_STATE, "getrandom failed");
        p += got;
        left -= (size_t)got;
    }
    for (uint64_t& r : out)
        while (r == 0)
            if (getrandom(&r, sizeof(r), 0) != (ssize_t)sizeof(r)) return fail(h, PE_ERR_STATE, "getrandom failed");
    return PE_OK;
}

}  // namespace posevo

namespace {

int batch_run(pe_engine* h, const char* who, const uint8_t* pk96, const uint8_t* msg192, const uint8_t* sig192, uint32_t n,
              const uint64_t* scalars, int32_t* verdict)
{
    const uint32_t c = h->batch_chunk, F = BLS_BATCH_FAN;
    uint32_t* st = h->batch_stats;
    std::fill(st, st + 8, 0u);
    st[6] = c;
    st[7] = F;
    memset(h->batch_gt, 0, sizeof(h->batch_gt));
    h->batch_gt[47] = 1;  // the empty product
    if (n == 0) return PE_OK;
    std::vector<uint64_t> drawn;
    if (!scalars) {
        drawn.resize(n);
        PE_TRY(draw_scalars(h, drawn));
        scalars = drawn.data();
    }
    for (uint32_t g = 0; g < n; ++g)
        if (scalars[g] == 0) return fail(h, PE_ERR_INVALID_ARG, std::string(who) + ": a zero scalar");

    const size_t max_chunks = ((size_t)n + c - 1) / c, rows = (size_t)n + max_chunks, lvl = (max_chunks + F - 1) / F;
    const size_t N = n;
    Layout L;
    const auto r_pk = L.take<uint8_t>(96 * N), r_msg = L.take<uint8_t>(192 * N), r_sig = L.take<uint8_t>(192 * N);
    const auto r_scal = L.take<uint64_t>(N);
    const auto r_neg = L.take_bytes(256);  // -g1, 96 wire bytes
    const auto r_status = L.take<int32_t>(N);
    const auto r_pkm = L.take<uint32_t>(24 * N), r_msgm = L.take<uint32_t>(48 * N), r_sigm = L.take<uint32_t>(48 * N);
    const auto r_live = L.take<uint32_t>(N), r_scaled = L.take<uint32_t>(96 * N);
    const auto r_ws = L.take<uint32_t>((size_t)BLS_PAIR_WORDS * rows);
    const auto r_flag = L.take<int32_t>(rows);
    const auto r_off = L.take<uint32_t>(max_chunks + 1), r_gt = L.take<uint32_t>((size_t)BLS_GT_WORDS * max_chunks);
    const auto r_lvl0 = L.take<uint32_t>((size_t)BLS_GT_WORDS * lvl), r_lvl1 = L.take<uint32_t>((size_t)BLS_GT_WORDS * lvl);
    const auto r_bad = L.take<int32_t>(max_chunks);
    const auto r_zero = L.take_bytes<int32_t>(256);  // the "no bad point" flag of the one product
    const auto r_verdict = L.take<int32_t>(max_chunks);
    const auto r_out = L.take<uint8_t>(576);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_batch, L, h->stream));
    HIP_TRY(h, w.put(r_pk, pk96, 96 * N));
    HIP_TRY(h, w.put(r_msg, msg192, 192 * N));
    HIP_TRY(h, w.put(r_sig, sig192, 192 * N));
    HIP_TRY(h, w.put(r_scal, scalars, N));
    HIP_TRY(h, w.put(r_neg, NEG_G1_BE96, 96));
    HIP_TRY(h, w.zero(r_zero, 1));

    // ---- settle: what never enters the batch
    launch_bls_batch_settle(h->stream, w(r_pk), w(r_msg), w(r_sig), n, w(r_pkm), w(r_msgm), w(r_sigm), w(r_status));
    launch_g2_subgroup_check(h->stream, w(r_sigm), n, w(r_status));  // the batch is sound over G2 only
    HIP_TRY(h, hipGetLastError());
    std::vector<int32_t> status(n);
    HIP_TRY(h, w.get(r_status, status.data(), N));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<uint32_t> live;
    live.reserve(n);
    for (uint32_t g = 0; g < n; ++g) {
        if (status[g] == BLS_BATCH_LIVE) live.push_back(g);
        verdict[g] = status[g] == BLS_BATCH_LIVE ? PE_BLS_VALID : status[g] == BLS_BATCH_BAD ? PE_BLS_BAD_POINT : PE_BLS_INVALID;
    }
    const uint32_t n_live = (uint32_t)live.size(), chunks = (n_live + c - 1) / c;
    st[0] = n_live;
    st[1] = chunks;
    if (n_live == 0) return PE_OK;

    // ---- scale, chunk, Miller loop, product, ONE final exponentiation
    std::vector<uint32_t> off((size_t)chunks + 1);
    for (uint32_t j = 0; j < chunks; ++j) off[j] = j * (c + 1);
    off[chunks] = n_live + chunks;
    HIP_TRY(h, w.put(r_live, live.data(), n_live));
    HIP_TRY(h, w.put(r_off, off.data(), (size_t)chunks + 1));
    launch_bls_scale_g1(h->stream, w(r_live), n_live, c, w(r_scal), w(r_pkm), w(r_msgm), w(r_ws), w(r_flag));
    launch_bls_scale_g2(h->stream, w(r_live), n_live, w(r_scal), w(r_sigm), w(r_scaled));
    launch_bls_chunk_sig(h->stream, w(r_scaled), n_live, c, chunks, w(r_neg), w(r_ws), w(r_flag));
    launch_bls_miller(h->stream, w(r_ws), w(r_flag), w(r_off), chunks, w(r_gt), w(r_bad));
    const uint32_t* top = w(r_gt);  // the chunk values stay where they are: the fallback needs them
    uint32_t m = chunks, side = 0;
    while (m > 1) {
        const uint32_t m_out = (m + F - 1) / F;
        uint32_t* out = w(side ? r_lvl1 : r_lvl0);
        launch_bls_gt_product(h->stream, top, m, out, m_out);
        top = out;
        m = m_out;
        side ^= 1;
        ++st[2];
    }
    launch_bls_final_exp(h->stream, top, w(r_zero), 1, w(r_verdict), w(r_out));
    st[3] = 1;
    HIP_TRY(h, hipGetLastError());
    int32_t all_valid = 0;
    HIP_TRY(h, w.get(r_verdict, &all_valid, 1));
    HIP_TRY(h, w.get(r_out, h->batch_gt, 576));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (all_valid == 1) return PE_OK;

    // ---- fallback: which chunks, then their live groups one by one
    std::vector<int32_t> chunk_ok(chunks);
    launch_bls_final_exp(h->stream, w(r_gt), w(r_bad), chunks, w(r_verdict), nullptr);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, w.get(r_verdict, chunk_ok.data(), chunks));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    st[4] = chunks;
    std::vector<uint32_t> again;
    for (uint32_t j = 0; j < chunks; ++j)
        if (chunk_ok[j] != 1)
            for (uint32_t i = j * c; i < std::min(n_live, (j + 1) * c); ++i) again.push_back(live[i]);
    const uint32_t k = (uint32_t)again.size();
    st[5] = k;
    if (k == 0) return PE_OK;
    std::vector<int32_t> one_by_one(k);
    PE_TRY(verify_pairs_run(
        h, who, k, [&](uint32_t t) { return pk96 + (size_t)96 * again[t]; },
        [&](uint32_t t) { return msg192 + (size_t)192 * again[t]; }, [&](uint32_t t) { return sig192 + (size_t)192 * again[t]; },
        one_by_one.data()));
    for (uint32_t t = 0; t < k; ++t) verdict[again[t]] = one_by_one[t];
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_batch_verify(pe_engine* h, const uint8_t* pubkeys96, const uint8_t* message_points192, const uint8_t* signatures192,
                    uint32_t n_groups, const uint64_t* scalars, int32_t* verdict)
{
    if (!h || (n_groups && (!pubkeys96 || !message_points192 || !signatures192 || !verdict))) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));  // open pipelines complete
    if (h->dist_ready()) return refuse_dist(h, "pe_batch_verify");
    return batch_run(h, "pe_batch_verify", pubkeys96, message_points192, signatures192, n_groups, scalars, verdict);
}

int pe_batch_fast_aggregate_verify(pe_engine* h, const uint32_t* index, const uint32_t* offsets, uint32_t n_groups,
                                   const uint8_t* message_points192, const uint8_t* signatures192, const uint64_t* scalars,
                                   int32_t* verdict)
{
    if (!h || !offsets || (n_groups && (!message_points192 || !signatures192 || !verdict))) return PE_ERR_INVALID_ARG;
    if (n_groups && offsets[n_groups] && !index) return PE_ERR_INVALID_ARG;
    PE_TRY(enter(h));
    if (h->dist_ready()) return refuse_dist(h, "pe_batch_fast_aggregate_verify");
    if (n_groups == 0) return batch_run(h, "pe_batch_fast_aggregate_verify", nullptr, nullptr, nullptr, 0, scalars, verdict);
    if (!h->have_points) return fail(h, PE_ERR_STATE, "pe_batch_fast_aggregate_verify: no pubkeys loaded");
    // the aggregate pubkeys, summed on the device as pe_fast_aggregate_verify sums them; an empty group's is the identity
    std::vector<uint8_t> sums((size_t)96 * n_groups);
    PE_TRY(pe_g1_sum(h, nullptr, 0, index, offsets, n_groups, sums.data()));
    return batch_run(h, "pe_batch_fast_aggregate_verify", sums.data(), message_points192, signatures192, n_groups, scalars,
                     verdict);
}

int pe_profile_batch_set_chunk(pe_engine* h, uint32_t chunk)
{
    if (!h) return PE_ERR_INVALID_ARG;
    if (chunk < 1 || chunk > PE_BATCH_CHUNK_MAX) return fail(h, PE_ERR_INVALID_ARG, "pe_profile_batch_set_chunk: 1 .. PE_BATCH_CHUNK_MAX");
    h->batch_chunk = chunk;
    return PE_OK;
}

int pe_profile_batch_stats(const pe_engine* h, uint32_t out[8])
{
    if (!h || !out) return PE_ERR_INVALID_ARG;
    std::copy(h->batch_stats, h->batch_stats + 8, out);
    return PE_OK;
}

int pe_profile_batch_gt(const pe_engine* h, uint8_t* out576)
{
    if (!h || !out576) return PE_ERR_INVALID_ARG;
    memcpy(out576, h->batch_gt, 576);
    return PE_OK;
}

}  // extern "C"
